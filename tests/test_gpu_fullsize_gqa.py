"""Grouped-query attention at a model's size: d_model = 1024, 16 query heads over 4 kv heads (dh = 64), batch 4, a prefill of 512
positions (the causal core on the repeated rows) and 4 single-token steps (the grouped decode kernels, two chunks of keys).  Sampled
rows - the first, a tile seam, the last of the prefill, and every step - against tests/gqa_oracle.py over each sample's whole prefix.
The output projection, a contraction of K = d_model = 1024, is last: held as tests/test_gpu_fullsize_causal.py holds the module
output at this size, through tolerance.assert_contraction with K = d_model, max|context| and max|Wo| and the bias epilogue.
(Under the elementwise form 1e-6 * max|ref| alone the same run measured err_gpu 8.99e-7, err_cpu32 3.53e-7 against 8.68e-7: that
form has no term for the length of the last contraction.)"""
import numpy as np
import pytest

import gqa_oracle as GO
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu


def test_model_sized_prefill_and_steps():
    import neuronika_amd
    nk = neuronika_amd.tape
    tdev = nk.Device(0)
    d, H, Hkv, B, T0, steps = 1024, 16, 4, 4, 512, 4
    S = T0 + steps
    mha = nk.nn.MultiheadAttention(tdev, d, H, 0.0, 3, kv_heads=Hkv)
    mha.causal = True
    rng = np.random.default_rng(11)
    x = (rng.random((B * S, d), dtype=np.float32) * 2 - 1).astype(np.float32)
    rows = lambda lo, hi: np.ascontiguousarray(np.concatenate([x[b * S + lo:b * S + hi] for b in range(B)]))
    cache = nk.nn.KvCache(tdev, B, Hkv, d // H, S)
    got = np.zeros((B, S, d), np.float32)
    y = mha.forward_step(nk.from_ndarray(tdev, rows(0, T0)), B, cache); y.forward()
    got[:, :T0] = y.data().reshape(B, T0, d)
    for s in range(steps):
        y = mha.forward_step(nk.from_ndarray(tdev, rows(T0 + s, T0 + s + 1)), B, cache); y.forward()
        got[:, T0 + s] = y.data()
    assert cache.lens() == [S] * B
    sampled = [0, 31, 32, 255, T0 - 1] + list(range(T0, S))
    refs = {}
    for dt in (np.float64, np.float32):
        W = [getattr(mha, n).weight.data().astype(dt) for n in "qkvo"]
        Bs = [getattr(mha, n).bias.data().astype(dt) for n in "qkvo"]
        out, ctx = GO.mha_forward(x.astype(dt), W, Bs, H, Hkv, B, causal=True, with_context=True)
        refs[dt] = (out.reshape(B, S, d)[:, sampled], float(np.abs(ctx).max()), float(np.abs(W[3]).max()))
    (want, ctx_max, wmax), want32 = refs[np.float64], refs[np.float32][0]
    assert np.isfinite(got).all()
    ratio = assert_contraction("mha_gqa:fullsize output", got[:, sampled], want, d, ctx_max, wmax, cpu32=want32, epilogue=True)
    print("mha_gqa:fullsize err / bound %.3g" % ratio)
