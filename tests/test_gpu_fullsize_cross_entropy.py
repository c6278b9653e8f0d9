"""nk_cross_entropy_* at the sizes of real models against the f64 oracle: GPT-2's head with 8 x 1024 tokens (8192, 50257) - odd C,
so three rows in four start off a 16-byte boundary - a (16384, 32000) head, uniform and Zipf targets, and a (16, 150, 128, 128)
segmentation shape through the generic kernels: loss, lse, sampled gradient rows, and assign equal to `+=` onto zeros bit for bit."""
import numpy as np
import pytest

import cross_entropy_oracle as X
from test_gpu_embedding import uniform_ids, zipf_ids

pytestmark = pytest.mark.gpu


def _lse_rows(x, rows=256):
    """per-row lse of a 2-d f32 array in f64, a slab of rows at a time"""
    out = np.empty(x.shape[0])
    for i in range(0, x.shape[0], rows):
        s = x[i:i + rows].astype(np.float64)
        m = s.max(axis=1)
        out[i:i + rows] = m + np.log(np.exp(s - m[:, None]).sum(axis=1))
    return out


@pytest.mark.parametrize("N,C", [(8192, 50257), (16384, 32000)])
def test_language_model_heads(dev, N, C):
    from neuronika_amd import capi as c
    rng = np.random.default_rng(N + C)
    x = rng.standard_normal((N, C), dtype=np.float32)
    x *= np.float32(2.0)
    XS, LSE, OUT, G = dev.array(x), dev.full(N, np.nan), dev.full(1, np.nan), dev.array(np.array([0.5], np.float32))
    want_lse = _lse_rows(x)
    xmax = float(np.abs(x).max())
    for ids in (uniform_ids, zipf_ids):
        t = ids(rng, N, C)
        t[::7] = 3.0                                                   # ignore_index = 3 is hit
        T = dev.array(t)
        on = t != 3.0
        count = int(on.sum())
        per = np.where(on, want_lse - x[np.arange(N), t.astype(np.int64)].astype(np.float64), 0.0)
        b = X.bounds(C, xmax, N, 0.0, 0.5, 1.0 / count)
        for red, want in (("mean", per.sum() / count), ("sum", per.sum())):
            c.cross_entropy_fwd(dev, XS, T, LSE, OUT, (N, C), red, 3)
            assert abs(OUT.item() - want) <= b["loss"] * (count if red == "sum" else 1), (red, OUT.item(), want)
        assert np.abs(LSE.numpy() - want_lse).max() <= b["lse"]
        DA = dev.full((N, C), np.nan)
        c.cross_entropy_bwd(dev, DA, G, XS, T, LSE, (N, C), "mean", 3, assign=True)
        da = DA.numpy()
        del DA
        rows = np.concatenate([[0, 1, 2, 3, 7, N - 1], rng.integers(0, N, 58)])
        want = X.backward(x[rows], t[rows], want_lse[rows], 0.5, "sum", 3) / count
        assert np.abs(da[rows] - want).max() <= b["dx"], np.abs(da[rows] - want).max()
        assert not da[~on].any() and da[on].any(axis=1).all()
        DX = dev.zeros((N, C))
        c.cross_entropy_bwd(dev, DX, G, XS, T, LSE, (N, C), "mean", 3)
        assert np.array_equal(DX.numpy().view(np.uint32), da.view(np.uint32)), "assign differs from += onto zeros"
        del DX, da


def test_segmentation_shape_through_the_generic_kernels(dev):
    from neuronika_amd import capi as c
    shape = (16, 150, 128, 128)
    rng = np.random.default_rng(7)
    x = rng.standard_normal(shape, dtype=np.float32)
    x *= np.float32(2.0)
    t = rng.integers(0, 150, (16, 128, 128)).astype(np.float32)
    t[:, ::4, ::3] = 255.0                                             # the usual "void" label: >= C, selects nothing
    XS, T, G = dev.array(x), dev.array(t), dev.array(np.array([0.5], np.float32))
    LSE, OUT = dev.full(t.shape, np.nan), dev.full(1, np.nan)
    want_loss, want_lse = X.forward(x, t, "mean")
    on = t < 150
    count = int(on.sum())
    b = X.bounds(150, float(np.abs(x).max()), t.size, 0.0, 0.5, 1.0 / count)
    c.cross_entropy_fwd(dev, XS, T, LSE, OUT, shape, "mean")
    assert abs(OUT.item() - want_loss) <= b["loss"] and np.abs(LSE.numpy() - want_lse).max() <= b["lse"]
    DA = dev.full(shape, np.nan)
    c.cross_entropy_bwd(dev, DA, G, XS, T, LSE, shape, "mean", assign=True)
    da = DA.numpy()
    want = X.backward(x[:2], t[:2], want_lse[:2], 0.5, "sum") / count
    assert np.abs(da[:2] - want).max() <= b["dx"]
    assert not da[np.broadcast_to(~on[:, None], shape)].any()
    DX = dev.zeros(shape)
    c.cross_entropy_bwd(dev, DX, G, XS, T, LSE, shape, "mean")
    assert np.array_equal(DX.numpy().view(np.uint32), da.view(np.uint32)), "assign differs from += onto zeros"
