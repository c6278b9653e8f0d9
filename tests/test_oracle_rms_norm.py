"""tests/rms_norm_oracle.py pinned without a GPU: against torch autograd in f64 on the composed expression, against central
differences, and against the two properties of a scale-invariant map (y(a x) = y(x) and sum(dx * x) = 0 per row at eps = 0)."""
import os
import subprocess
import sys

import numpy as np

import rms_norm_oracle as RN

TESTS = os.path.dirname(os.path.abspath(__file__))


def _inputs(rows, D, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((rows, D)), rng.standard_normal((rows, D)), 1.0 + 0.5 * rng.standard_normal(D)


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well (a second HIP runtime
# in one address space aborts at exit; the suite's other torch users are child processes for the same reason)
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import rms_norm_oracle as RN
n = 0
scale = lambda a: max(1.0, float(np.abs(a).max()))
for rows, D, eps in [(1, 1, 1e-6), (3, 5, 1e-6), (7, 64, 1e-5), (4, 100, 0.0), (2, 1027, 1e-6)]:
    for affine in (True, False):
        rng = np.random.default_rng(rows * 1009 + D)
        x, g, w = rng.standard_normal((rows, D)), rng.standard_normal((rows, D)), 1.0 + 0.5 * rng.standard_normal(D)
        tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        tw = torch.tensor(w, dtype=torch.float64, requires_grad=True)
        ty = tx * torch.rsqrt((tx * tx).mean(dim=1, keepdim=True) + eps)         # the composed expression, x * rsqrt(mean(x^2) + eps) * w
        if affine:
            ty = ty * tw
        ty.backward(torch.tensor(g, dtype=torch.float64))
        y, st = RN.forward(x, w if affine else None, eps)
        dx, dg = RN.backward(g, x, w if affine else None, st)
        assert y.dtype == np.float64 and dx.dtype == np.float64 and st.shape == (rows,)
        assert np.abs(y - ty.detach().numpy()).max() <= 1e-12 * scale(y)
        assert np.abs(dx - tx.grad.numpy()).max() <= 1e-12 * scale(dx)
        assert np.abs(st - 1.0 / np.sqrt((x * x).mean(axis=1) + eps)).max() <= 1e-12 * scale(st)
        if affine:
            assert np.abs(dg - tw.grad.numpy()).max() <= 1e-12 * scale(dg)
        n += 1
print("cases", n)
"""


def test_matches_torch_autograd_in_f64():
    """y, stats and the autograd gradients of x and w at several (rows, D, eps), with and without the weight, to 1e-12"""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK, TESTS], capture_output=True, text=True)
    assert r.returncode == 0 and "cases 10" in r.stdout, r.stdout + r.stderr


def test_matches_central_differences_in_f64():
    rows, D, eps, h = 3, 9, 1e-6, 1e-6
    x, g, w = _inputs(rows, D, 5)
    loss = lambda xx, ww: float((RN.forward(xx, ww, eps)[0] * g).sum())
    dx, dg = RN.backward(g, x, w, RN.forward(x, w, eps)[1])
    for idx in np.ndindex(rows, D):
        e = np.zeros_like(x); e[idx] = h
        assert abs((loss(x + e, w) - loss(x - e, w)) / (2 * h) - dx[idx]) <= 1e-7 * max(1.0, abs(dx[idx]))
    for j in range(D):
        e = np.zeros_like(w); e[j] = h
        assert abs((loss(x, w + e) - loss(x, w - e)) / (2 * h) - dg[j]) <= 1e-7 * max(1.0, abs(dg[j]))


def test_output_is_scale_invariant_at_eps_zero():
    x, g, w = _inputs(6, 48, 8)
    y, st = RN.forward(x, w, 0.0)
    for a in (256.0, 1.0 / 256.0):                       # powers of two: exact in every step
        ya, sa = RN.forward(x * a, w, 0.0)
        assert np.array_equal(ya, y) and np.array_equal(sa * a, st)
    ya, _ = RN.forward(x * 3.7, w, 0.0)
    assert np.abs(ya - y).max() <= 1e-14 * np.abs(y).max()
    # hence the gradient has no component along x
    dx, _ = RN.backward(g, x, w, st)
    assert np.abs((dx * x).sum(axis=1)).max() <= 1e-13 * np.abs(dx).max() * np.abs(x).max() * x.shape[1]


def test_zero_row_and_f32_twin():
    x, g, w = _inputs(4, 16, 2)
    x[2] = 0.0
    y, st = RN.forward(x, w, 1e-6)
    assert (y[2] == 0).all() and st[2] == 1.0 / np.sqrt(1e-6)
    dx, dg = RN.backward(g, x, w, st)
    assert np.allclose(dx[2], st[2] * g[2] * w, rtol=1e-15)              # xhat = 0: dx = rstd * gh
    keep = np.arange(4) != 2
    assert np.array_equal(dg, RN.backward(g[keep], x[keep], w, st[keep])[1])   # the zero row adds nothing to dgamma
    y0, st0 = RN.forward(x, w, 0.0)
    assert np.isnan(y0[2]).all() and np.isfinite(y0[keep]).all() and np.isinf(st0[2])
    o64, o32 = RN.both(x.astype(np.float32), w.astype(np.float32), g.astype(np.float32))
    for k in ("y", "stats", "dx", "dgamma"):
        assert o64[k].dtype == np.float64 and o32[k].dtype == np.float32 and o64[k].shape == o32[k].shape
        assert np.abs(o32[k] - o64[k]).max() <= 1e-5 * max(1.0, np.abs(o64[k]).max())
    # a row whose sum of squares overflows f32: rstd = 0 in the f32 twin
    big = np.full((1, 8), 3e19, np.float32)
    assert RN.forward(big, None, 1e-6)[1][0] == 0.0
