"""The sliding-window fused core through the tape (`_tape`): `nn::MultiheadAttention::forward()` with S > window takes ONE attention
node on the band kernels (nk_attention_qkv_band_* in the packed module, nk_attention_band_* on the strided path, grouped layers behind
`repeat_kv`) where the core takes the head size; `fused_core = false` keeps the composed path with the banded constant.

The oracle is tests/window_oracle.py's module in f64 and f32, fed the same Philox mask where dropout is active; the rule is the one
tests/test_gpu_tape_window.py holds the same quantities to (err_gpu <= max(2 * err_cpu32, 1e-6 * scale) against the f64 oracle, the
bias gradients with the weight gradient's magnitude as floor; margins under `attention_band:tape *`)."""
import numpy as np
import pytest

from oracle import neuronika_oracle as O
import rope_oracle as RO
import window_oracle as WO

pytestmark = pytest.mark.gpu

B = 2
# (d_model, heads, S, W): dh = 32 with whole tiles, dh = 64 ragged with a window that crosses a block seam
GEOMETRIES = [(128, 4, 160, 40), (256, 4, 300, 129)]
LAYERS = {"packed": (1, False), "grouped": (2, False), "packed, rope": (1, True), "grouped, rope": (2, True)}   # (heads / kv_heads, rope)


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


def rnd(seed, shape, lo=0.0, hi=1.0):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(hi - lo) + np.float32(lo), dtype=np.float32).reshape(shape)


def _check(got, want, want32, what, floor=0.0):
    scale = max(np.abs(want).max(), floor)
    err_gpu, err_cpu = np.abs(got - want).max(), np.abs(want32 - want).max()
    from conftest import record_margin
    record_margin("attention_band:tape " + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


def _params(mha, dt):
    return ([getattr(mha, n).weight.data().astype(dt) for n in "qkvo"], [getattr(mha, n).bias.data().astype(dt) for n in "qkvo"])


def _leaves(mha, X):
    return [X] + [getattr(getattr(mha, n), w) for n in "qkvo" for w in ("weight", "bias")]


def _module(nk, tdev, d, H, Hkv, window, use_rope, p=0.0, seed=3):
    mha = nk.nn.MultiheadAttention(tdev, d, H, p, seed, kv_heads=Hkv)
    mha.causal = True
    mha.window = window
    ro = None
    if use_rope:
        mha.rope = nk.nn.RotaryEmbedding(tdev, d // H, 320)
        ro = RO.make(320, d // H)
    return mha, ro


def _oracles(mha, ro, x, g, H, Hkv, W, p, noise):
    refs = []
    for dt in (np.float64, np.float32):
        Wt, Bs = _params(mha, dt)
        refs.append(WO.mha_forward_backward(x.astype(dt), Wt[0], Bs[0], Wt[1], Bs[1], Wt[2], Bs[2], Wt[3], Bs[3], H, Hkv, B, p,
                                            noise.astype(dt), g.astype(dt), W, rope=ro))
    return refs


def _hold(mha, X, y, refs, what):
    (ref, grads), (ref32, grads32) = refs
    assert np.isfinite(y.data()).all() and np.isfinite(X.grad()).all(), what
    _check(y.data(), ref, ref32, "out" + what)
    _check(X.grad(), grads["x"], grads32["x"], "dx" + what)
    for nme in "qkvo":
        _check(getattr(mha, nme).weight.grad(), grads["w" + nme], grads32["w" + nme], "dw" + nme + what)
        _check(getattr(mha, nme).bias.grad(), grads["b" + nme], grads32["b" + nme], "db" + nme + what, np.abs(grads["w" + nme]).max())


@pytest.mark.parametrize("layer", list(LAYERS))
@pytest.mark.parametrize("d,H,S,W", GEOMETRIES)
def test_forward_beyond_the_window_takes_the_band_core(nk, tdev, d, H, S, W, layer):
    """S > window: the graph has the node count of the same module without a window - the fused core was taken, not the composition -
    and output and every parameter / input gradient hold against the banded oracle."""
    G, use_rope = LAYERS[layer]
    Hkv = H // G
    assert nk.Var.attention_core_supported(S, d // H, 0.0)
    mha, ro = _module(nk, tdev, d, H, Hkv, W, use_rope)
    x, g = rnd(0, (B * S, d), -1, 1), rnd(5, (B * S, d), -1, 1)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = mha.forward(X, B)
    plain, _ = _module(nk, tdev, d, H, Hkv, 0, use_rope)
    n_core = plain.forward(nk.from_ndarray(tdev, x).requires_grad(), B).history_len()
    assert y.history_len() == n_core, (y.history_len(), n_core)
    mha.fused_core = False
    n_composed = mha.forward(nk.from_ndarray(tdev, x).requires_grad(), B).history_len()
    mha.fused_core = True
    assert n_composed > n_core
    for leaf in _leaves(mha, X):
        leaf.zero_grad()
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    refs = _oracles(mha, ro, x, g, H, Hkv, W, 0.0, np.ones((B * H, S, S)))
    what = " [d %d H %d Hkv %d S %d W %d, %s]" % (d, H, Hkv, S, W, layer)
    _hold(mha, X, y, refs, what)
    # the band is not the triangle
    y0 = plain.forward(nk.from_ndarray(tdev, x).requires_grad(), B); y0.forward()
    assert np.abs(y0.data()[:W] - y.data()[:W]).max() <= 1e-5             # rows r < W see every key <= r: f32 rounding of O(1) values
    assert not np.allclose(y0.data(), y.data(), atol=1e-3)


@pytest.mark.parametrize("Hkv_div", [1, 2], ids=["packed", "grouped"])
@pytest.mark.parametrize("d,H,S,W", GEOMETRIES)
def test_the_composed_path_stays_behind_the_switch(nk, tdev, d, H, S, W, Hkv_div):
    """fused_core = false: the node-by-node path with the banded constant still runs, holds against the oracle, and agrees with the
    band core within the rule's bound."""
    Hkv = H // Hkv_div
    mha, ro = _module(nk, tdev, d, H, Hkv, W, False)
    x, g = rnd(1, (B * S, d), -1, 1), rnd(6, (B * S, d), -1, 1)
    refs = _oracles(mha, ro, x, g, H, Hkv, W, 0.0, np.ones((B * H, S, S)))
    outs = []
    for core in (False, True):
        mha.fused_core = core
        X = nk.from_ndarray(tdev, x).requires_grad()
        y = mha.forward(X, B)
        for leaf in _leaves(mha, X):
            leaf.zero_grad()
        y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
        _hold(mha, X, y, refs, " [d %d Hkv %d S %d W %d, %s]" % (d, Hkv, S, W, "core" if core else "composed"))
        outs.append((y.history_len(), y.data().copy()))
    assert outs[0][0] > outs[1][0]
    (ref, _), (ref32, _) = refs
    bound = max(2 * np.abs(ref32 - ref).max(), 1e-6 * np.abs(ref).max())
    assert np.abs(outs[0][1] - outs[1][1]).max() <= 2 * bound             # each within `bound` of the f64 oracle


@pytest.mark.parametrize("Hkv_div", [1, 2], ids=["packed", "grouped"])
@pytest.mark.parametrize("d,H,S,W", GEOMETRIES)
def test_dropout_in_training_draws_the_padded_positions(nk, tdev, d, H, S, W, Hkv_div):
    """p = 0.2 in training: two forward / backward passes against the oracle fed the same Philox mask - score (bh, r, k) takes draw
    (bh * SP + r) * SP + k, and every forward advances the offset by one padded tensor's calls."""
    p, seed, Hkv = 0.2, 7654321, H // Hkv_div
    nk.manual_seed(seed)
    mha, ro = _module(nk, tdev, d, H, Hkv, W, False, p=p)
    x, g = rnd(2, (B * S, d), -1, 1), rnd(7, (B * S, d), -1, 1)
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = mha.forward(X, B)
    SP = (S + 31) // 32 * 32
    n = B * H * SP * SP
    for call in range(2):
        noise = np.ascontiguousarray(O.dropout_noise(n, p, seed, call * O.dropout_draws_calls(n)).reshape(B * H, SP, SP)[:, :S, :S])
        for leaf in _leaves(mha, X):
            leaf.zero_grad()
        y.forward(); y.no_grad(); y.with_grad()
        y.backward_from(nk.from_ndarray(tdev, g))
        refs = _oracles(mha, ro, x, g, H, Hkv, W, p, noise)
        _hold(mha, X, y, refs, " [d %d Hkv %d S %d W %d, p 0.2, pass %d]" % (d, Hkv, S, W, call))


def test_a_graph_without_gradients_runs_the_band_core_too(nk, tdev):
    """`Var::heads_attention(window)` without gradients: the values of the differentiable node, bit for bit; window >= S is the causal
    node; a window without the causal rule, or a negative one, panics."""
    S, H, dh, W = 300, 2, 64, 70
    d = H * dh
    scale = float(np.float32(1 / np.sqrt(dh)))
    q, k, v = (rnd(s, (B * S, d), -1, 1) for s in (1, 2, 3))
    status = nk.Status(False)
    Q, K, V = (nk.from_ndarray(tdev, t) for t in (q, k, v))
    out = Q.heads_attention(K, V, B, S, H, dh, scale, 0.0, status, causal=True, window=W)
    out.forward()
    Qd, Kd, Vd = (nk.from_ndarray(tdev, t).requires_grad() for t in (q, k, v))
    kept = Qd.heads_attention(Kd, Vd, B, S, H, dh, scale, 0.0, status, causal=True, window=W)
    kept.forward()
    assert np.array_equal(out.data(), kept.data())
    o, _ = WO.attention_core_forward(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), H, B, 0.0, np.ones((B * H, S, S)), W)
    np.testing.assert_allclose(out.data(), o, rtol=0, atol=2e-6)          # (|v| <= 1: the causal tape test's bound)
    causal = Q.heads_attention(K, V, B, S, H, dh, scale, 0.0, status, causal=True); causal.forward()
    wide = Q.heads_attention(K, V, B, S, H, dh, scale, 0.0, status, causal=True, window=S); wide.forward()
    assert np.array_equal(causal.data(), wide.data())
    with pytest.raises(RuntimeError, match="causal"):
        Q.heads_attention(K, V, B, S, H, dh, scale, 0.0, status, causal=False, window=W)
    with pytest.raises(RuntimeError, match="window"):
        Q.heads_attention(K, V, B, S, H, dh, scale, 0.0, status, causal=True, window=-2)


def test_the_evaluation_forward_captures_and_the_training_forward_refuses(nk, tdev):
    """As the causal core: a training-mode forward with dropout active bakes its Philox offset into the kernel arguments and refuses
    stream capture; the evaluation forward captures and replays to the same bits."""
    S, H, dh, W = 160, 2, 64, 40
    x = nk.from_ndarray(tdev, rnd(4, (B * S, H * dh), -1, 1))
    st = nk.Status(True)
    y, other = x.heads_attention(x, x, B, S, H, dh, 0.125, 0.5, st, causal=True, window=W), x.relu()
    y.forward(); other.forward()
    tdev.graph_begin()
    other.forward()                        # (something to capture)
    with pytest.raises(RuntimeError, match="same mask"):
        y.forward()
    g = tdev.graph_end()
    del g
    st.set(False)
    y.forward(); want = y.data().copy()
    tdev.graph_begin(); y.forward(); g = tdev.graph_end()
    g.launch(); g.launch()
    assert np.array_equal(y.data(), want)
