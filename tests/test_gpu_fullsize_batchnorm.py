"""Batch normalisation at the size the C3 convolution step produces: its (128, 128, 56, 56) output, 401 408 values per channel,
205 MB per tensor.  Training forward and backward on the whole tensor; sampled channels (the first, the last, some between)
against the f64 oracle: y, stats, the running statistics and dx under the suite's rule, the channel sums and the parameter
gradients through tolerance.assert_contraction with K = N * L."""
import numpy as np
import pytest

import batchnorm_oracle as BN
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu


def test_c3_output(dev):
    from conftest import record_margin
    from neuronika_amd import capi as c
    N, C, L = 128, 128, 56 * 56
    rng = np.random.default_rng(2025)
    x = rng.standard_normal((N, C, L), dtype=np.float32)
    x *= (0.5 + rng.random((1, C, 1), dtype=np.float32))
    x += rng.standard_normal((1, C, 1), dtype=np.float32)
    g = rng.standard_normal((N, C, L), dtype=np.float32)
    gamma, beta = (1.0 + 0.5 * rng.standard_normal(C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    running = (rng.standard_normal(C).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32))
    X, G, W, B, RM, RV = dev.array(x), dev.array(g), dev.array(gamma), dev.array(beta), dev.array(running[0]), dev.array(running[1])
    Y, S, SUMS, DX = dev.full((N, C, L), np.nan), dev.full((C, 2), np.nan), dev.full((C, 2), np.nan), dev.full((N, C, L), np.nan)
    DG, DB = dev.full((C,), np.nan), dev.full((C,), np.nan)
    c.batch_norm_fwd(dev, X, W, B, Y, S, RM, RV, N, C, L, 1e-5, 0.1)
    c.batch_norm_bwd_sums(dev, SUMS, G, X, S, N, C, L)
    c.batch_norm_bwd(dev, DX, G, X, W, S, SUMS, N, C, L, assign=True)
    c.batch_norm_bwd_params(dev, DG, DB, SUMS, C, assign=True)
    got = dict(y=Y.numpy(), stats=S.numpy(), running_mean=RM.numpy(), running_var=RV.numpy(), sums=SUMS.numpy(), dx=DX.numpy(),
               dgamma=DG.numpy(), dbeta=DB.numpy())
    assert np.isfinite(got["y"]).all() and np.isfinite(got["dx"]).all()
    ch = [0, 1, 37, 64, 126, 127]
    o64, o32 = BN.both(x[:, ch], gamma[ch], beta[ch], g[:, ch], 1e-5, 0.1, (running[0][ch], running[1][ch]))
    for name in ("y", "dx"):
        want, want32 = o64[name], o32[name]
        scale = max(1.0, float(np.abs(want).max()))
        err_gpu, err_cpu = float(np.abs(got[name][:, ch] - want).max()), float(np.abs(want32 - want).max())
        record_margin("batchnorm:fullsize " + name, err_gpu, err_cpu, 1e-6 * scale)
        assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (name, err_gpu, err_cpu, scale)
    for name in ("stats", "running_mean", "running_var"):
        want, want32 = o64[name], o32[name]
        scale = max(1.0, float(np.abs(want).max()))
        err_gpu, err_cpu = float(np.abs(got[name][ch] - want).max()), float(np.abs(want32 - want).max())
        record_margin("batchnorm:fullsize " + name, err_gpu, err_cpu, 1e-6 * scale)
        assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (name, err_gpu, err_cpu, scale)
    gmax, ymax = float(np.abs(g).max()), float(np.abs(o64["y"]).max()) + 5.0
    assert_contraction("batchnorm:fullsize s0", got["sums"][ch, 0], o64["sums"][:, 0], N * L, gmax, 1.0, cpu32=o32["sums"][:, 0])
    assert_contraction("batchnorm:fullsize s1", got["sums"][ch, 1], o64["sums"][:, 1], N * L, gmax, ymax, cpu32=o32["sums"][:, 1])
    assert_contraction("batchnorm:fullsize dgamma", got["dgamma"][ch], o64["dgamma"], N * L, gmax, ymax, cpu32=o32["dgamma"])
    assert_contraction("batchnorm:fullsize dbeta", got["dbeta"][ch], o64["dbeta"], N * L, gmax, 1.0, cpu32=o32["dbeta"])
