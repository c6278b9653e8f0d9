"""tests/group_norm_oracle.py pinned without a GPU: in f64 against torch.nn.functional.group_norm and instance_norm on the CPU in
f64, forward and the autograd gradients, over shapes that include G = 1, G = C, L = 1, D = 1 and the forms without an affine
part; the statistics against NumPy's own mean and variance; the f32 twin's dtypes."""
import os
import subprocess
import sys

import numpy as np

import group_norm_oracle as GN

TESTS = os.path.dirname(os.path.abspath(__file__))
EPS = 1e-5
# (N, C, L, G): G = 1, G = C, L = 1, D = 1, ragged sizes
SHAPES = [(4, 8, 16, 2), (3, 6, 5, 1), (2, 4, 9, 4), (5, 6, 1, 3), (2, 3, 1, 3), (3, 7, 5, 7), (1, 12, 33, 4)]


def _data(N, C, L, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, C, L)) * (0.5 + rng.random((1, C, 1))) + rng.standard_normal((1, C, 1))
    return x, rng.standard_normal((N, C, L)), 1.0 + 0.5 * rng.standard_normal(C), rng.standard_normal(C)


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well (a second HIP runtime
# in one address space aborts at exit; the suite's other torch users are child processes for the same reason)
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import group_norm_oracle as GN
EPS = 1e-5
n = 0
def close(a, b, tol):
    assert np.abs(a - b).max() <= tol * max(1.0, float(np.abs(b).max())), (np.abs(a - b).max(), tol)
def one(x, g, gamma, beta, G, torch_fn):
    st = GN.group_stats(x, G, EPS)
    y = GN.normalise(x, G, st, gamma, beta)
    dx, dgamma, dbeta = GN.backward(g, x, G, gamma, st)
    assert y.dtype == np.float64 and dx.dtype == np.float64 and st.shape == (x.shape[0] * G, 2)
    tx = torch.tensor(x, requires_grad=True)
    tw = torch.tensor(gamma, requires_grad=True) if gamma is not None else None
    tb = torch.tensor(beta, requires_grad=True) if beta is not None else None
    ty = torch_fn(tx, tw, tb)
    ty.backward(torch.tensor(g))
    close(y, ty.detach().numpy(), 1e-11)
    close(dx, tx.grad.numpy(), 1e-9)
    if gamma is not None:
        close(dgamma, tw.grad.numpy(), 1e-10)
        close(dbeta, tb.grad.numpy(), 1e-10)
for N, C, L, G in [(4, 8, 16, 2), (3, 6, 5, 1), (2, 4, 9, 4), (5, 6, 1, 3), (2, 3, 1, 3), (3, 7, 5, 7), (1, 12, 33, 4)]:
    for affine in (True, False):
        rng = np.random.default_rng(N + 10 * C + 100 * L + G)
        x = rng.standard_normal((N, C, L)) * (0.5 + rng.random((1, C, 1))) + rng.standard_normal((1, C, 1))
        g, gamma, beta = rng.standard_normal((N, C, L)), 1.0 + 0.5 * rng.standard_normal(C), rng.standard_normal(C)
        if not affine:
            gamma = beta = None
        one(x, g, gamma, beta, G, lambda tx, tw, tb: torch.nn.functional.group_norm(tx, G, tw, tb, EPS))
        n += 1
# one channel per group is torch's instance_norm (L > 1: torch refuses a single value per plane)
for N, C, L in [(2, 4, 9), (3, 5, 16), (1, 3, 7)]:
    for affine in (True, False):
        rng = np.random.default_rng(7 * N + C + L)
        x, g = rng.standard_normal((N, C, L)), rng.standard_normal((N, C, L))
        gamma, beta = (1.0 + 0.5 * rng.standard_normal(C), rng.standard_normal(C)) if affine else (None, None)
        one(x, g, gamma, beta, C, lambda tx, tw, tb: torch.nn.functional.instance_norm(tx, weight=tw, bias=tb, eps=EPS))
        n += 1
print("cases", n)
"""


def test_matches_torch_group_norm_and_instance_norm_in_f64():
    """y and the autograd gradients of x, weight and bias: 7 shapes x affine on / off against group_norm, 3 shapes x affine
    on / off at G = C against instance_norm"""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK, TESTS], capture_output=True, text=True)
    assert r.returncode == 0 and "cases 20" in r.stdout, r.stdout + r.stderr


def test_statistics_are_the_rows_mean_and_biased_variance():
    for N, C, L, G in SHAPES:
        x, _, _, _ = _data(N, C, L, N + C + L)
        st = GN.group_stats(x, G, EPS)
        rows = x.reshape(N * G, -1)
        np.testing.assert_allclose(st[:, 0], rows.mean(axis=1), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(st[:, 1], 1.0 / np.sqrt(rows.var(axis=1) + EPS), rtol=1e-12)


def test_matches_central_differences_in_f64():
    N, C, L, G, h = 2, 4, 3, 2, 1e-6
    x, g, gamma, beta = _data(N, C, L, 5)
    loss = lambda xx, ww, bb: float((GN.normalise(xx, G, GN.group_stats(xx, G, EPS), ww, bb) * g).sum())
    dx, dgamma, dbeta = GN.backward(g, x, G, gamma, GN.group_stats(x, G, EPS))
    for idx in np.ndindex(N, C, L):
        e = np.zeros_like(x); e[idx] = h
        assert abs((loss(x + e, gamma, beta) - loss(x - e, gamma, beta)) / (2 * h) - dx[idx]) <= 1e-6 * max(1.0, abs(dx[idx]))
    for j in range(C):
        e = np.zeros(C); e[j] = h
        assert abs((loss(x, gamma + e, beta) - loss(x, gamma - e, beta)) / (2 * h) - dgamma[j]) <= 1e-7 * max(1.0, abs(dgamma[j]))
        assert abs((loss(x, gamma, beta + e) - loss(x, gamma, beta - e)) / (2 * h) - dbeta[j]) <= 1e-7 * max(1.0, abs(dbeta[j]))


def test_one_element_rows_give_beta():
    x, g, gamma, beta = _data(2, 3, 1, 5)
    st = GN.group_stats(x, 3, EPS)
    assert np.array_equal(GN.normalise(x, 3, st, gamma, beta), np.broadcast_to(beta.reshape(1, 3, 1), (2, 3, 1)))
    assert np.array_equal(st[:, 0], x.ravel())
    assert np.array_equal(GN.backward(g, x, 3, gamma, st)[0], np.zeros_like(x))    # the three terms cancel exactly


def test_both_keeps_each_twin_in_its_dtype():
    x, g, gamma, beta = (a.astype(np.float32) for a in _data(3, 4, 10, 1))
    o64, o32 = GN.both(x, 2, gamma, beta, g, EPS)
    for k in ("y", "stats", "dx", "dgamma", "dbeta"):
        assert o64[k].dtype == np.float64 and o32[k].dtype == np.float32, k
        assert o64[k].shape == o32[k].shape
        np.testing.assert_allclose(o32[k], o64[k], rtol=1e-3, atol=1e-4)
    assert o64["stats"].shape == (6, 2) and o64["dx"].shape == (3, 4, 10)
