"""The window kernels at a model's size, once per slice length: B = 4, 32 query heads over 8 kv heads, dh = 128, W = 4096, on a
rolling cache of the smallest legal capacity for T = 16, 4096 + 15 slots (67 MB each for keys and values), at lengths around 20000 -
the ring has wrapped four times, every window spans 33 chunks of 128 keys and straddles the wrap - with T = 1 and T = 16 new rows
per sample; one sample is shorter than the window.  Every output is finite; 32 sampled (sample, head, row) problems are compared with
f64 dot products through tolerance.assert_contraction: the context row is a contraction over the K = min(n, W) keys of the window of
the probabilities (max|a| = the largest probability of the f64 oracle) with the values (max|b| = max|v|)."""
import numpy as np
import pytest

import window_oracle as WO
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu


def _uniform(rng, shape, lo, hi):
    a = rng.random(shape, dtype=np.float32)
    a *= np.float32(hi - lo)
    a += np.float32(lo)
    return a


def _probabilities(q, kc, start, W, cap, scale):
    """the f64 probabilities of one (sample, kv head) problem on the ring: for max|a|"""
    lo, n = WO.window_rows(start, 0, W, cap, True)
    s = (kc[[p % cap for p in range(lo, n)]].astype(np.float64) @ q.astype(np.float64)) * scale
    e = np.exp(s - s.max())
    return e / e.sum()


@pytest.mark.parametrize("T", [1, 16])
def test_model_size_step_on_a_rolling_cache(dev, T):
    from neuronika_amd import capi as c
    B, H, Hkv, dh, W = 4, 32, 8, 128, 4096
    cap, G = W + 15, H // Hkv
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    rng = np.random.default_rng(11)
    kc, vc = _uniform(rng, (B, Hkv, cap, dh), -1, 1), _uniform(rng, (B, Hkv, cap, dh), -1, 1)      # the ring after the step's append
    q = _uniform(rng, (B * T, H * dh), -1, 1)
    start = np.array([19999, 19998, 20036, 1000], dtype=np.int32)        # first-row lengths 20000, 19999, 20037 and 1001 < W
    Q, Kc, Vc, S = dev.array(q), dev.array(kc), dev.array(vc), dev.int_array(start)
    out = dev.full((B * T, H * dh), np.nan)
    ws = dev.full((c.attention_decode_window_workspace(B, T, H, dh, W),), np.nan)
    c.attention_decode_window_fwd(dev, Q, H * dh, Kc, Vc, S, out, ws, B, T, H, Hkv, dh, cap, W, 1, scale)
    got = out.numpy()
    assert np.all(np.isfinite(got))
    picks = np.random.default_rng(12).choice(B * H * T, size=32, replace=False)
    for pick in picks:
        b, rest = divmod(int(pick), H * T)
        h, t = divmod(rest, T)
        row, kv = b * T + t, h // G
        qs = np.ascontiguousarray(q[row:row + 1, h * dh:(h + 1) * dh])
        ks, vs, st = kc[b:b + 1, kv:kv + 1], vc[b:b + 1, kv:kv + 1], start[b:b + 1] + t     # row t alone: a T = 1 problem at start + t
        ref, ref32 = (WO.decode_forward(qs.astype(dt), ks.astype(dt), vs.astype(dt), st, 1, W, True, scale=scale) for dt in (np.float64, np.float32))
        pmax = float(_probabilities(qs[0], ks[0, 0], int(st[0]), W, cap, scale).max())
        keys = min(int(st[0]) + 1, W)
        ratio = assert_contraction("attention_window:fullsize T %d" % T, got[row:row + 1, h * dh:(h + 1) * dh], ref, keys, pmax,
                                   float(np.abs(vs).max()), cpu32=ref32)
        print("model size [T %d b %d h %d t %d] err / bound %.3g" % (T, b, h, t, ratio))
