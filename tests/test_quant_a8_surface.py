"""The surface of the int8-activation quantised Linear without a GPU - header, exported symbol, ctypes signature, null-device refusal,
nn.QuantLinear.act_bits - and the oracle's own error against the f64 product of f32 x with w^, held to the derived bound

    0.5 * sx[m] * sum_k |w^[n][k]|  +  (spans + 3) * 2^-24 * (sum_k |x^[m][k] w^[n][k]| + |bias[n]|)

The first term is the half step of the activation rounding; the second is one f32 rounding per span product-and-add, the final scale
and the bias add, each relative to a partial sum that the sum of magnitudes bounds (x^ = xq * sx)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import quant_a8_oracle as A
import quant_oracle as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_ctypes_and_host_layer():
    import neuronika_amd
    from neuronika_amd import capi
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuronika_hip.h")).read(), flags=re.S))
    assert ("int nk_quant_a8_linear_fwd(nk_device* dev, const float* x, int ldx, const float* qw, const float* scales, const float* bias, "
            "float* y, int ldy, int M, int N, int K, int bits, int group);") in flat
    VP, I = C.c_void_p, C.c_int
    assert "nk_quant_a8_linear_fwd" in capi.EXPORTED and hasattr(capi.lib, "nk_quant_a8_linear_fwd") and hasattr(capi, "quant_a8_linear_fwd")
    assert capi._SIGS["nk_quant_a8_linear_fwd"] == [VP, VP, I, VP, VP, VP, VP, I, I, I, I, I, I]
    assert capi.lib.nk_quant_a8_linear_fwd(None, None, 0, None, None, None, None, 0, 0, 0, 0, 0, 0) == 1   # before anything else
    assert hasattr(neuronika_amd.tape.nn.QuantLinear, "act_bits")


@pytest.mark.parametrize("bits", (8, 4))
@pytest.mark.parametrize("group,K", ((64, 192), (128, 2176), (0, 96), (0, 4224)))
def test_oracle_stays_within_the_derived_bound(bits, group, K):
    rng = np.random.default_rng(K + bits)
    M, N = 9, 33
    x = (rng.standard_normal((M, K)) * np.exp(rng.standard_normal((M, 1)))).astype(np.float32)
    x[4] = 0
    b, s = Q.pack((rng.standard_normal((N, K)) * np.exp(rng.standard_normal((N, 1)))).astype(np.float32), bits, group)
    bias = rng.standard_normal(N).astype(np.float32)
    y = A.forward(x, b, s, bias, bits, group)
    assert (y[4].view(np.uint32) == bias.view(np.uint32)).all()                       # a zero row gives exactly the bias
    xq, sx = Q.quantise(x, 8, 0)
    w = np.abs(Q.unpack(b, s, bits, group, K).astype(np.float64))
    xhat = np.abs(xq.astype(np.float64) * sx.astype(np.float64))
    bound = 0.5 * sx.astype(np.float64) * w.sum(axis=1)[None, :] + (len(A.spans(K, group)) + 3) * 2.0 ** -24 * (xhat @ w.T + np.abs(bias)[None, :])
    err = np.abs(y.astype(np.float64) - Q.forward64(x, b, s, bias, bits, group))
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
