"""tests/pooling_oracle.py against torch's f64 max_pool{1,2,3}d(return_indices=True), avg_pool{1,2,3}d(count_include_pad=..) and their
autograd gradients: overlapping and non-overlapping windows, padded, odd extents where floor drops the last column, ties on
integer data, the NaN / -inf rules of the header (torch keeps the LAST NaN of a window where the header says the first, so the
NaN rule is checked against a direct scan instead), flatten.  No GPU.  torch runs in a child process (this file run as a program): a
process that has loaded the HIP library must not import torch as well, a second HIP runtime in one address space aborts at exit."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import pooling_oracle as P

torch = F = None   # set in the child process only

# (x_shape, kernel, stride, padding)
GEOMETRIES = [
    ((2, 3, 16), (2,), (2,), (0,)), ((2, 3, 17), (3,), (2,), (1,)), ((1, 2, 9), (4,), (3,), (2,)), ((2, 2, 7), (7,), (7,), (0,)),
    ((2, 3, 8, 8), (2, 2), (2, 2), (0, 0)), ((2, 3, 12, 12), (3, 3), (2, 2), (1, 1)), ((2, 3, 12, 12), (3, 3), (2, 2), (0, 0)),
    ((2, 3, 8, 12), (3, 3), (1, 1), (1, 1)), ((1, 2, 9, 11), (3, 2), (2, 1), (1, 0)), ((2, 2, 7, 7), (7, 7), (7, 7), (0, 0)),
    ((1, 3, 13, 10), (5, 4), (3, 2), (2, 2)), ((2, 2, 5, 6), (1, 1), (1, 1), (0, 0)), ((1, 1, 5, 5), (3, 3), (4, 4), (0, 0)),
    ((2, 2, 6, 8, 8), (2, 2, 2), (2, 2, 2), (0, 0, 0)), ((1, 2, 5, 7, 9), (3, 2, 3), (2, 1, 2), (1, 1, 0)),
    ((1, 2, 4, 4, 4), (4, 4, 4), (4, 4, 4), (0, 0, 0)),
]
IDS = ["x".join(map(str, g[0])) + "-k" + "x".join(map(str, g[1])) + "s" + "x".join(map(str, g[2])) + "p" + "x".join(map(str, g[3])) for g in GEOMETRIES]


def _t(a):
    return torch.tensor(a, dtype=torch.float64, requires_grad=True)


def _torch_out_shape(geom):
    shape, k, s, p = geom
    nd = len(k)
    y = getattr(F, f"max_pool{nd}d")(torch.zeros(shape), k, s, p)
    assert P.out_shape(shape, k, s, p) == tuple(y.shape)


def _torch_max_pool(geom, integer):
    shape, k, s, p = geom
    nd = len(k)
    rng = np.random.default_rng(1)
    x = rng.integers(-2, 3, shape).astype(np.float64) if integer else rng.standard_normal(shape)
    y, idx = P.max_pool_fwd(x, k, s, p)
    xt = _t(x)
    yt, it = getattr(F, f"max_pool{nd}d")(xt, k, s, p, return_indices=True)
    assert y.dtype == np.float64 and idx.dtype == np.int32
    np.testing.assert_array_equal(y, yt.detach().numpy())
    np.testing.assert_array_equal(idx, it.numpy())
    g = rng.integers(-3, 4, y.shape).astype(np.float64) if integer else rng.standard_normal(y.shape)
    yt.backward(torch.tensor(g))
    np.testing.assert_allclose(P.max_pool_bwd(g, idx, shape), xt.grad.numpy(), rtol=0, atol=1e-12)
    y32, idx32 = P.max_pool_fwd(x.astype(np.float32), k, s, p)
    assert y32.dtype == np.float32
    if integer:
        np.testing.assert_array_equal(idx32, idx)


def _torch_avg_pool(geom, cip):
    shape, k, s, p = geom
    nd = len(k)
    rng = np.random.default_rng(2)
    x = rng.standard_normal(shape)
    xt = _t(x)
    yt = getattr(F, f"avg_pool{nd}d")(xt, k, s, p, count_include_pad=cip)
    y = P.avg_pool_fwd(x, k, s, p, cip)
    np.testing.assert_allclose(y, yt.detach().numpy(), rtol=0, atol=1e-13)
    g = rng.standard_normal(y.shape)
    yt.backward(torch.tensor(g))
    np.testing.assert_allclose(P.avg_pool_bwd(g, shape, k, s, p, cip), xt.grad.numpy(), rtol=0, atol=1e-13)
    assert P.avg_pool_fwd(x.astype(np.float32), k, s, p, cip).dtype == np.float32
    assert P.avg_pool_bwd(g.astype(np.float32), shape, k, s, p, cip).dtype == np.float32


def test_oracle_matches_torch_in_f64():
    """shapes, max pooling with indices (real data and integer ties), average pooling with both divisors and every autograd
    gradient, over GEOMETRIES"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True)
    assert r.returncode == 0 and "cases %d" % (5 * len(GEOMETRIES)) in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("geom", GEOMETRIES, ids=IDS)
def test_f32_twin_and_backward_shapes(geom):
    shape, k, s, p = geom
    x = np.random.default_rng(6).standard_normal(shape).astype(np.float32)
    y, idx = P.max_pool_fwd(x, k, s, p)
    assert y.dtype == np.float32 and idx.dtype == np.int32 and y.shape == P.out_shape(shape, k, s, p)
    assert np.array_equal(np.take_along_axis(x.reshape(shape[0], shape[1], -1), idx.reshape(shape[0], shape[1], -1).astype(np.int64), 2).reshape(y.shape), y)
    assert P.max_pool_bwd(y, idx, shape).shape == tuple(shape)
    assert P.avg_pool_bwd(y, shape, k, s, p, False).shape == tuple(shape)


def test_empty_stride_means_kernel():
    x = np.random.default_rng(3).standard_normal((2, 2, 9, 9))
    np.testing.assert_array_equal(P.max_pool_fwd(x, (3, 3))[0], P.max_pool_fwd(x, (3, 3), (3, 3), (0, 0))[0])
    np.testing.assert_array_equal(P.avg_pool_fwd(x, (3, 3)), P.avg_pool_fwd(x, (3, 3), (3, 3), (0, 0)))


def _scan(x, k, s, p):
    """the header's rule, one window at a time"""
    N, C, H, W = x.shape
    _, _, OH, OW = P.out_shape(x.shape, k, s, p)
    y, idx = np.empty((N, C, OH, OW), x.dtype), np.empty((N, C, OH, OW), np.int32)
    for n, c, oh, ow in itertools.product(range(N), range(C), range(OH), range(OW)):
        best, bi = -np.inf, None
        for h in range(oh * s[0] - p[0], oh * s[0] - p[0] + k[0]):
            for w in range(ow * s[1] - p[1], ow * s[1] - p[1] + k[1]):
                if 0 <= h < H and 0 <= w < W:
                    v = x[n, c, h, w]
                    if bi is None:
                        bi = h * W + w
                    if v > best or (np.isnan(v) and not np.isnan(best)):
                        best, bi = v, h * W + w
        y[n, c, oh, ow], idx[n, c, oh, ow] = best, bi
    return y, idx


def test_nan_inf_rules():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 2, 9, 10))
    x[rng.random(x.shape) < 0.15] = np.nan
    x[rng.random(x.shape) < 0.15] = -np.inf
    x[rng.random(x.shape) < 0.05] = np.inf
    x[0, 0, :4, :4] = -np.inf                     # whole windows of -inf: -inf and the first in-range offset
    x[1, 1, 2:5, 2:5] = np.nan                    # whole windows of NaN: the first one
    for k, s, p in [((3, 3), (2, 2), (1, 1)), ((2, 2), (2, 2), (0, 0)), ((3, 2), (1, 2), (1, 1))]:
        y, idx = P.max_pool_fwd(x, k, s, p)
        ys, is_ = _scan(x, k, s, p)
        np.testing.assert_array_equal(y, ys)
        np.testing.assert_array_equal(idx, is_)
    y, idx = P.max_pool_fwd(x, (3, 3), (2, 2), (1, 1))
    assert y[0, 0, 0, 0] == -np.inf and idx[0, 0, 0, 0] == 0
    assert np.isnan(y[1, 1, 2, 2])


def test_flatten():
    x = np.arange(2 * 3 * 4 * 5, dtype=np.float32).reshape(2, 3, 4, 5)
    f = P.flatten(x)
    assert f.shape == (2, 60) and f.dtype == np.float32
    np.testing.assert_array_equal(P.flatten_bwd(f, x.shape), x)
    np.testing.assert_array_equal(P.global_avg_pool_fwd(x.astype(np.float64))[:, :, 0, 0], x.astype(np.float64).mean(axis=(2, 3)))


@pytest.mark.parametrize("bad", [
    ((2, 3, 8, 8), (0, 2), (2, 2), (0, 0)), ((2, 3, 8, 8), (2, 2), (0, 2), (0, 0)), ((2, 3, 8, 8), (2, 2), (2, 2), (2, 0)),
    ((2, 3, 8, 8), (3, 3), (2, 2), (-1, 0)), ((2, 3, 2, 8), (5, 3), (1, 1), (1, 1)), ((2, 3, 0, 8), (2, 2), (2, 2), (1, 1)),
    ((2, 3), (), (), ()), ((2, 3, 4, 4, 4, 4), (1,) * 4, (1,) * 4, (0,) * 4), ((-1, 3, 8), (2,), (2,), (0,)),
    ((1, 1, 65536, 65536), (1, 1), (1, 1), (0, 0)),
])
def test_rejected(bad):
    with pytest.raises(ValueError):
        P.out_shape(*bad)


if __name__ == "__main__":
    import torch
    F = torch.nn.functional
    n = 0
    for geom in GEOMETRIES:
        _torch_out_shape(geom)
        for flag in (False, True):
            _torch_max_pool(geom, flag)
            _torch_avg_pool(geom, flag)
        n += 5
    print("cases", n)
