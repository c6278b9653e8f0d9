"""tests/cross_entropy_oracle.py against torch on the CPU (`F.cross_entropy` in f64: 2-d and n-d inputs, ignore_index, label smoothing,
sum / mean, gradients), against the existing oracle's log_softmax + nll where that composition is defined, and the points where the
contract leaves torch or the composition, pinned explicitly."""
import os
import subprocess
import sys

import numpy as np

import cross_entropy_oracle as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _case(seed, shape, spread=3.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * spread).astype(np.float32)
    t = rng.integers(0, shape[1], (shape[0],) + tuple(shape[2:])).astype(np.float32)
    return x, t


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
import torch.nn.functional as F
sys.path.insert(0, sys.argv[1])
import cross_entropy_oracle as X
from test_oracle_cross_entropy import _case
cases = 0
for shape in [(1, 1), (5, 2), (64, 10), (7, 257), (3, 5, 4), (2, 6, 3, 5), (4, 3, 2, 2, 2)]:
    for red in ("sum", "mean"):
        for eps in (0.0, 0.1):
            for ignore in (-1, 1):
                if ignore >= shape[1]:
                    continue
                x, t = _case(sum(shape), shape)
                tx = torch.from_numpy(x.astype(np.float64)).requires_grad_()
                tt = torch.from_numpy(t.astype(np.int64))
                if ignore >= 0 and not (t == ignore).any():
                    t.reshape(-1)[0] = ignore; tt.reshape(-1)[0] = ignore
                if ignore >= 0 and (t == ignore).all():
                    continue                                    # the empty mean is pinned in its own test
                want = F.cross_entropy(tx, tt, reduction=red, ignore_index=ignore if ignore >= 0 else -100, label_smoothing=eps)
                want.backward(torch.tensor(0.75, dtype=torch.float64))
                loss, lse = X.forward(x, t, red, ignore, eps)
                assert abs(loss - want.item()) <= 1e-12 * max(1.0, abs(want.item())), (shape, red, eps, ignore, loss, want.item())
                assert np.allclose(lse, torch.logsumexp(tx.detach(), 1).numpy(), rtol=1e-13, atol=1e-13)
                dx = X.backward(x, t, lse, 0.75, red, ignore, eps)
                assert np.allclose(dx, tx.grad.numpy(), rtol=1e-11, atol=1e-13), (shape, red, eps, ignore)
                cases += 1
print("cases", cases)
"""


def test_against_torch():
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK, os.path.join(ROOT, "tests")], capture_output=True, text=True)
    assert r.returncode == 0 and "cases 52" in r.stdout, r.stdout + r.stderr


def test_against_the_composition_of_the_existing_oracle():
    """nll(log_softmax(x, 1), t): equal under Sum for any shape, under Mean for 2-d inputs with every position active"""
    from oracle import neuronika_oracle as O
    for shape, reds in (((6, 5), ("sum", "mean")), ((3, 4, 5), ("sum",)), ((2, 7, 2, 3), ("sum",))):
        x, t = _case(11, shape)
        x64 = x.astype(np.float64)
        y = np.zeros_like(x64)
        O.log_softmax_forward(x64, y, 1)
        for red in reds:
            loss, lse = X.forward(x, t, red)
            assert abs(loss - O.nll_forward(y, t, red)) <= 1e-12 * abs(loss)
            gy = np.zeros_like(x64)
            O.nll_backward(gy, 0.5, t, red)
            dx = np.zeros_like(x64)
            O.log_softmax_backward(dx, gy, y, 1)
            assert np.allclose(X.backward(x, t, lse, 0.5, red), dx, rtol=1e-11, atol=1e-14)
    # where they part: nll's Mean divides the forward by shape[0] and the backward by target.len(); the contract uses the active count
    x, t = _case(12, (3, 4, 5))
    y = np.zeros((3, 4, 5))
    O.log_softmax_forward(x.astype(np.float64), y, 1)
    assert abs(X.forward(x, t, "mean")[0] * 15 - O.nll_forward(y, t, "mean") * 3) <= 1e-11
    t[0, 0] = 99.0                                                # selects nothing: one position fewer in the divisor
    assert abs(X.forward(x, t, "mean")[0] * 14 - O.nll_forward(y, t, "sum")) <= 1e-11


def test_ids_are_read_as_the_device_reads_them():
    f = np.array([0.0, -0.0, 0.99, 1.0, 1.5, -3.0, np.nan, np.inf, -np.inf, 1e19, 3.0], np.float32)
    ids, on = X.active_mask(f, 3)
    assert ids[:7].tolist() == [0, 0, 0, 1, 1, 0, 0] and on.tolist() == [True] * 7 + [False, True, False, False]
    assert X.active_mask(f, 3, ignore_index=0)[1].tolist() == [False, False, False, True, True, False, False, False, False, False, False]


def test_inactive_positions_and_the_empty_mean():
    x, t = _case(5, (4, 3))
    t[:] = [3.0, 1.0, 7.5, 1.0]
    loss, lse = X.forward(x, t, "mean", ignore_index=1)
    assert loss == 0.0 and np.isfinite(lse).all()                  # nothing active: 0, where torch gives NaN
    assert not X.backward(x, t, lse, 1.0, "mean", ignore_index=1).any()
    loss, _ = X.forward(x, t, "mean")                              # two active positions: the divisor is 2, not 4
    per = X.pieces(x, t)[1]
    assert per[0] == 0.0 and per[2] == 0.0 and abs(loss - (per[1] + per[3]) / 2) < 1e-15
    dx = X.backward(x, t, None, 1.0, "mean")
    assert not dx[0].any() and not dx[2].any() and abs(dx[1].sum()) < 1e-15


def test_smoothing_and_gradient_against_a_finite_difference():
    x, t = _case(9, (3, 6, 2))
    for red in ("sum", "mean"):
        dx = X.backward(x, t, None, 1.0, red, 2, 0.2)
        h, num = 1e-6, np.zeros(x.shape)
        for i in np.ndindex(*x.shape):
            xp, xm = x.astype(np.float64), x.astype(np.float64)
            xp[i] += h; xm[i] -= h
            num[i] = (X.forward(xp, t, red, 2, 0.2)[0] - X.forward(xm, t, red, 2, 0.2)[0]) / (2 * h)
        assert np.allclose(dx, num, atol=1e-8)


def test_non_finite_logits():
    """-inf is an ordinary logit; a NaN or +inf logit makes its position's lse, loss and gradient row NaN (log_softmax + nll's pattern)"""
    x, t = _case(4, (4, 5))
    x[0, 2] = -np.inf; x[1, 3] = np.nan; x[2, 0] = np.inf
    t[:] = [1.0, 0.0, 2.0, 4.0]
    lse, per, _, _ = X.pieces(x, t)
    assert np.isfinite(lse[0, 0]) and np.isnan(lse[1, 0]) and np.isnan(lse[2, 0]) and np.isfinite(lse[3, 0])
    assert np.isfinite(per[0, 0]) and np.isnan(per[1, 0]) and np.isnan(per[2, 0])
    dx = X.backward(x, t, lse, 1.0, "sum")
    assert np.isfinite(dx[0]).all() and dx[0, 2] == 0 and np.isnan(dx[1]).all() and np.isnan(dx[2]).all() and np.isfinite(dx[3]).all()


def test_bounds_grow_with_the_inputs():
    a, b = X.bounds(10, 1.0, 4), X.bounds(50257, 20.0, 8192, 0.1)
    assert all(0 < a[k] < b[k] for k in a) and b["lse"] < 1e-3 and a["lse"] < 1e-5
