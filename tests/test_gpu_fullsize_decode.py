"""The decode kernels at model size, once: B = 8, H = 16, dh = 64, a cache of 4096 positions (134 MB each for keys and values),
lengths 4095 and 4096 - the last chunk one key short and full, the longest length equal to the capacity - one new token per sample.
Every output is finite; 32 sampled (sample, head) problems are compared with f64 dot products under the rule of
tests/test_gpu_attention_decode.py."""
import numpy as np
import pytest

import decode_oracle as DO
from test_gpu_attention_decode import _check, _scale

pytestmark = pytest.mark.gpu


def _uniform(rng, shape, lo, hi):
    a = rng.random(shape, dtype=np.float32)
    a *= np.float32(hi - lo)
    a += np.float32(lo)
    return a


def test_model_size_step(dev):
    from neuronika_amd import capi as c
    B, H, dh, cap, T = 8, 16, 64, 4096, 1
    rng = np.random.default_rng(11)
    kc, vc = _uniform(rng, (B, H, cap, dh), -1, 1), _uniform(rng, (B, H, cap, dh), -1, 1)
    q = _uniform(rng, (B * T, H * dh), -1, 1)
    lens = np.array([4095, 4096] * (B // 2))
    start = (lens - 1).astype(np.int32)
    for b in range(B):                                                    # what lies past a sample's length is never read
        kc[b, :, lens[b]:] = np.nan
        vc[b, :, lens[b]:] = np.nan
    Q, Kc, Vc, S = dev.array(q), dev.array(kc), dev.array(vc), dev.int_array(start)
    out = dev.full((B * T, H * dh), np.nan)
    ws = dev.full((c.attention_decode_workspace(B, T, H, dh, cap),), np.nan)
    c.attention_decode_fwd(dev, Q, H * dh, Kc, Vc, S, out, ws, B, T, H, dh, cap, _scale(dh))
    got = out.numpy()
    assert np.all(np.isfinite(got))
    picks = np.random.default_rng(12).choice(B * H, size=32, replace=False)
    for pick in picks:
        b, h = divmod(int(pick), H)
        qs = np.ascontiguousarray(q[b:b + 1, h * dh:(h + 1) * dh])
        ks, vs = kc[b:b + 1, h:h + 1], vc[b:b + 1, h:h + 1]
        ref, ref32 = (DO.decode_forward(qs.astype(dt), ks.astype(dt), vs.astype(dt), start[b:b + 1], T, _scale(dh)) for dt in (np.float64, np.float32))
        _check(got[b:b + 1, h * dh:(h + 1) * dh], ref, ref32, float(np.abs(vs[0, 0, :lens[b]]).max()), "model size [b %d h %d]" % (b, h))
