"""The two pooling layers of a ResNet at their real sizes through the C ABI: (128, 64, 112, 112) through max pooling 3 / 2 / 1 and
(128, 512, 7, 7) through the global average, forward and backward against tests/pooling_oracle.py."""
import numpy as np
import pytest

import pooling_oracle as P

pytestmark = pytest.mark.gpu


def test_stem_max_pool_3_2_1(dev):
    from neuronika_amd import capi as c
    shape, k, s, p = (128, 64, 112, 112), (3, 3), (2, 2), (1, 1)
    rng = np.random.default_rng(0)
    x = np.maximum(rng.standard_normal(shape, dtype=np.float32), 0)          # after a ReLU: half the values tie at zero
    oshape = c.pool_out_shape(shape, k, s, p)
    assert oshape == (128, 64, 56, 56)
    X, Y, I = dev.array(x), dev.zeros(oshape), dev.int_zeros(oshape)
    c.max_pool_fwd(dev, X, shape, Y, I, k, s, p)
    want, idx = P.max_pool_fwd(x, k, s, p)
    assert np.array_equal(Y.numpy(), want)
    assert np.array_equal(I.numpy(), idx)
    g = rng.integers(-4, 5, oshape).astype(np.float32)
    G, DX = dev.array(g), dev.full(shape, np.nan)
    c.max_pool_bwd(dev, DX, shape, G, I, k, s, p, assign=True)
    dx = P.max_pool_bwd(g, idx, shape)
    assert np.array_equal(DX.numpy(), dx)
    c.max_pool_bwd(dev, DX, shape, G, I, k, s, p)
    assert np.array_equal(DX.numpy(), 2 * dx)


def test_global_average_pool_7x7(dev):
    from neuronika_amd import capi as c
    from conftest import record_margin
    shape = (128, 512, 7, 7)
    k = s = shape[2:]
    rng = np.random.default_rng(1)
    x = rng.standard_normal(shape, dtype=np.float32)
    X, Y = dev.array(x), dev.zeros((128, 512, 1, 1))
    c.avg_pool_fwd(dev, X, shape, Y, k, s, (0, 0))
    want, want32 = x.astype(np.float64).mean(axis=(2, 3), keepdims=True), P.global_avg_pool_fwd(x)
    err_gpu, err_cpu = float(np.abs(Y.numpy() - want).max()), float(np.abs(want32 - want).max())
    scale = float(np.abs(x).max())
    record_margin("pooling:fullsize global avg y", err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale)
    g = rng.standard_normal((128, 512, 1, 1), dtype=np.float32)
    DX = dev.full(shape, np.nan)
    c.avg_pool_bwd(dev, DX, shape, dev.array(g), k, s, (0, 0), assign=True)
    assert np.array_equal(DX.numpy(), np.broadcast_to(g / np.float32(49), shape))
