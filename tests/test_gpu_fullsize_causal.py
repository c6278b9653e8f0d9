"""The causal attention at the C5 geometry (B = 32, S = 1024, H = 16, dh = 64, p = 0.1: blocks of one head walk 4 .. 32 key tiles,
4096 blocks, eight dK / dV strips per head): the module's output and input gradient for one sample, and the attention core's
gradients for sample / head pairs at both ends of the batch, against the f64 oracle fed the device's Philox mask - through the
suite's contraction bound (`tolerance.assert_contraction`), margins recorded as `C5_causal_full_size:*`."""
import numpy as np
import pytest

from oracle import neuronika_oracle as O
import causal_oracle as CO

pytestmark = pytest.mark.gpu

B, S, H, DH, P = 32, 1024, 16, 64, 0.1
D = H * DH


def rnd(seed, shape, lo, hi):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(hi - lo) + np.float32(lo), dtype=np.float32)


def test_causal_core_at_c5_geometry(dev):
    from neuronika_amd import capi as c
    from tolerance import assert_contraction
    seed, offset = 2024, 11
    scale = float(np.float32(1.0 / np.sqrt(DH)))
    q, k, v, g = (rnd(s, (B * S, D), -1, 1) for s in (1, 2, 3, 4))
    Q, K, V, G = (dev.array(t) for t in (q, k, v, g))
    scores, stats, out = dev.full((B * H, S, S), np.nan), dev.zeros((B * H, S, 2)), dev.zeros((B * S, D))
    bits = dev.zeros((B * H, S, S // 32))
    c.attention_fwd(dev, Q, K, V, scores, stats, bits, out, B, S, H, DH, scale, P, True, seed, offset, causal=True)
    dS, dropped = dev.full((B * H, S, S), np.nan), dev.full((B * H, S, S), np.nan)
    dQ, dK, dV = (dev.full((B * S, D), np.nan) for _ in range(3))
    c.attention_bwd(dev, dQ, dK, dV, dS, dropped, G, out, scores, stats, bits, Q, K, V, B, S, H, DH, scale, P, True, assign=(True, True, True),
                    causal=True)
    got = dict(out=out.numpy(), dq=dQ.numpy(), dk=dK.numpy(), dv=dV.numpy())
    for name, t in got.items():
        assert np.isfinite(t).all(), name
    calls = O.dropout_draws_calls(S * S)   # draws of one (sample, head): S*S / 8 calls, consecutive per bh
    for b, h in ((0, 0), (17, 5), (31, 15)):
        bh = b * H + h
        noise = O.dropout_noise(S * S, P, seed, offset + bh * calls).reshape(1, S, S)
        rows, cols = slice(b * S, (b + 1) * S), slice(h * DH, (h + 1) * DH)
        ref = {}
        for dt in (np.float64, np.float32):
            o, cache = CO.attention_core_forward(q[rows, cols].astype(dt), k[rows, cols].astype(dt), v[rows, cols].astype(dt), 1, 1, P,
                                                noise.astype(dt))
            ref[dt] = dict(O.attention_core_backward(cache, g[rows, cols].astype(dt)), out=o, dropped=cache["dropped"])
        r64, r32 = ref[np.float64], ref[np.float32]
        ds_max, pd_max = np.abs(r64["d_scores"]).max(), np.abs(r64["dropped"]).max()
        tag = f"C5_causal_full_size:%s (sample {b}, head {h})"
        assert_contraction(tag % "O", got["out"][rows, cols], r64["out"], S, pd_max, np.abs(v).max(), cpu32=r32["out"])
        assert_contraction(tag % "dQ", got["dq"][rows, cols], r64["dq"], S, ds_max, np.abs(k).max(), cpu32=r32["dq"])
        assert_contraction(tag % "dK", got["dk"][rows, cols], r64["dk"], S, ds_max, np.abs(q).max(), cpu32=r32["dk"])
        assert_contraction(tag % "dV", got["dv"][rows, cols], r64["dv"], S, pd_max, np.abs(g).max(), cpu32=r32["dv"])


def test_causal_module_at_c5_geometry():
    import neuronika_amd
    from tolerance import assert_contraction
    nk = neuronika_amd.tape
    tdev = nk.Device(0)
    seed = 20241
    nk.manual_seed(seed)
    mha = nk.nn.MultiheadAttention(tdev, D, H, P, 1)
    mha.causal = True
    x, g = rnd(0, (B * S, D), -1, 1), rnd(5, (B * S, D), -1, 1)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = mha.forward(X, B)
    assert y.history_len() == 2                      # the packed projections + causal core, the out-projection
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    out, dx = y.data(), X.grad()
    assert np.isfinite(out).all() and np.isfinite(dx).all()
    b = 13                                           # one sample: its output and input gradient depend on no other sample
    rows = slice(b * S, (b + 1) * S)
    per_sample = O.dropout_draws_calls(H * S * S)
    noise = O.dropout_noise(H * S * S, P, seed, b * per_sample).reshape(H, S, S)
    ref = {}
    for dt in (np.float64, np.float32):
        W = [getattr(mha, n).weight.data().astype(dt) for n in "qkvo"]
        Bs = [getattr(mha, n).bias.data().astype(dt) for n in "qkvo"]
        ref[dt] = CO.mha_forward_backward(x[rows].astype(dt), W[0], Bs[0], W[1], Bs[1], W[2], Bs[2], W[3], Bs[3], H, 1, P, noise.astype(dt),
                                         g[rows].astype(dt))
    (o64, g64), (o32, g32) = ref[np.float64], ref[np.float32]
    wmax = max(np.abs(getattr(mha, n).weight.data()).max() for n in "qkvo")
    ctx_max = np.abs(x).max() * wmax * D / (1 - P)   # |context| <= max|V| / (1 - p), |V| <= D max|x| max|w| + |b|
    assert_contraction(f"C5_causal_full_size:module output (sample {b})", out[rows], o64, D, ctx_max, wmax, cpu32=o32, epilogue=True)
    do_max = np.abs(g[rows].astype(np.float64) @ getattr(mha, "o").weight.data().astype(np.float64)).max()   # the gradient entering the core
    assert_contraction(f"C5_causal_full_size:module dx (sample {b})", dx[rows], g64["x"], 3 * D, do_max, wmax, cpu32=g32["x"])
