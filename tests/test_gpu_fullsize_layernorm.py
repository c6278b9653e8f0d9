"""Layer normalisation at the size `bench.py --workload mha` works on: the (32768, 1024) activation of C5 (B = 64, S = 512,
d_model = 1024).  y and dx under the suite's rule against the f64 oracle, dgamma and dbeta - sums over 32768 rows, the first
stage split over the rows - through tolerance.assert_contraction with K = rows."""
import numpy as np
import pytest

import layernorm_oracle as LN
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu


def test_c5_activation(dev):
    from conftest import record_margin
    from neuronika_amd import capi as c
    rows, D = 32768, 1024
    rng = np.random.default_rng(2024)
    x = (rng.standard_normal((rows, D), dtype=np.float32) * np.float32(1.5) + rng.standard_normal((rows, 1), dtype=np.float32))
    g = rng.standard_normal((rows, D), dtype=np.float32)
    gamma, beta = (1.0 + 0.5 * rng.standard_normal(D)).astype(np.float32), rng.standard_normal(D).astype(np.float32)
    o64, o32 = LN.both(x, gamma, beta, g, 1e-5)
    X, G, W, B = dev.array(x), dev.array(g), dev.array(gamma), dev.array(beta)
    Y, S, DX = dev.full((rows, D), np.nan), dev.full((rows, 2), np.nan), dev.full((rows, D), np.nan)
    DG, DB = dev.full((D,), np.nan), dev.full((D,), np.nan)
    c.layer_norm_fwd(dev, X, W, B, Y, S, rows, D, 1e-5)
    c.layer_norm_bwd(dev, DX, G, X, W, S, rows, D, assign=True)
    c.layer_norm_bwd_params(dev, DG, DB, G, X, S, rows, D, assign=True)
    for name, got in (("y", Y.numpy()), ("stats", S.numpy()), ("dx", DX.numpy())):
        want, want32 = o64[name], o32[name]
        scale = float(np.abs(want).max())
        err_gpu, err_cpu = float(np.abs(got - want).max()), float(np.abs(want32 - want).max())
        record_margin("layernorm:fullsize " + name, err_gpu, err_cpu, 1e-6 * scale)
        assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (name, err_gpu, err_cpu, scale)
    assert_contraction("layernorm:fullsize dgamma", DG.numpy(), o64["dgamma"], rows, np.abs(g).max(), np.abs(o64["y"]).max(), cpu32=o32["dgamma"])
    assert_contraction("layernorm:fullsize dbeta", DB.numpy(), o64["dbeta"], rows, np.abs(g).max(), 1.0, cpu32=o32["dbeta"])
