"""RMS normalisation at a model's size: an (8192, 4096) activation (8192 tokens of a d_model = 4096 decoder), the block-per-row
kernels.  y, stats and dx under the suite's rule against the f64 oracle, dgamma - a sum over 8192 rows, the first stage split over
the rows - through tolerance.assert_contraction with K = rows."""
import numpy as np
import pytest

import rms_norm_oracle as RN
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu


def test_model_sized_activation(dev):
    from conftest import record_margin
    from neuronika_amd import capi as c
    rows, D = 8192, 4096
    rng = np.random.default_rng(2025)
    x = rng.standard_normal((rows, D), dtype=np.float32) * (np.float32(0.5) + 2 * rng.random((rows, 1), dtype=np.float32))
    g = rng.standard_normal((rows, D), dtype=np.float32)
    gamma = (1.0 + 0.5 * rng.standard_normal(D)).astype(np.float32)
    o64, o32 = RN.both(x, gamma, g, 1e-6)
    X, G, W = dev.array(x), dev.array(g), dev.array(gamma)
    Y, S, DX, DG = dev.full((rows, D), np.nan), dev.full((rows,), np.nan), dev.full((rows, D), np.nan), dev.full((D,), np.nan)
    c.rms_norm_fwd(dev, X, W, Y, S, rows, D, 1e-6)
    c.rms_norm_bwd(dev, DX, G, X, W, S, rows, D, assign=True)
    c.rms_norm_bwd_gamma(dev, DG, G, X, S, rows, D, assign=True)
    for name, got in (("y", Y.numpy()), ("stats", S.numpy()), ("dx", DX.numpy())):
        want, want32 = o64[name], o32[name]
        scale = float(np.abs(want).max())
        err_gpu, err_cpu = float(np.abs(got - want).max()), float(np.abs(want32 - want).max())
        print("rmsnorm:fullsize %s err_gpu=%.3e err_cpu32=%.3e abs=%.3e" % (name, err_gpu, err_cpu, 1e-6 * scale))
        record_margin("rmsnorm:fullsize " + name, err_gpu, err_cpu, 1e-6 * scale)
        assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (name, err_gpu, err_cpu, scale)
    xhat_max = float((np.abs(x).max(axis=1) * o64["stats"]).max())
    assert_contraction("rmsnorm:fullsize dgamma", DG.numpy(), o64["dgamma"], rows, np.abs(g).max(), xhat_max, cpu32=o32["dgamma"])
