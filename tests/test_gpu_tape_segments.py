"""Packed sequences through the tape (`_tape`): `nn::MultiheadAttention::forward(x, batch, segments)` takes ONE attention node on the
seg kernels (nk_attention_qkv_seg_* in the packed module, nk_attention_seg_* on the strided path, grouped layers behind `repeat_kv`)
where the core takes the head size, with rope restarted at every document start; `fused_core = false` and other head sizes keep the
composed path with the per-sample constant.

The oracle is tests/segment_oracle.py's module in f64 and f32; the rule is tests/test_gpu_tape_band.py's (err_gpu <= max(2 *
err_cpu32, 1e-6 * scale) against the f64 oracle, the bias gradients with the weight gradient's magnitude as floor; margins under
`attention_seg:tape *`)."""
import numpy as np
import pytest

import rope_oracle as RO
import segment_oracle as SO
import window_oracle as WO

pytestmark = pytest.mark.gpu

B = 2
# name: (d_model, heads, kv_heads, S, documents per sample, window, packed_qkv, rope)
LAYERS = {
    "dh 64 packed": (256, 4, 4, 200, [[70, 33, 97], [120, 80]], 0, True, False),
    "dh 64 packed, rope": (256, 4, 4, 200, [[70, 33, 97], [120, 80]], 0, True, True),
    "dh 32 strided": (128, 4, 4, 160, [[7, 25, 32, 96], [100, 60]], 0, False, False),
    "dh 32 strided, rope": (128, 4, 4, 160, [[7, 25, 32, 96], [100, 60]], 0, False, True),
    "one kv head": (128, 4, 1, 160, [[7, 25, 32, 96], [100, 60]], 0, True, True),
    "half the kv heads": (256, 4, 2, 200, [[70, 33, 97], [120, 80]], 0, True, False),
    "with a window": (256, 4, 4, 300, [[150, 150], [40, 260]], 70, True, True),
    "with a window, grouped": (256, 4, 2, 300, [[150, 150], [40, 260]], 70, True, False),
}


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
    record_margin("attention_seg:tape " + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


def _params(mha, dt):
    return ([getattr(mha, n).weight.data().astype(dt) for n in "qkvo"], [getattr(mha, n).bias.data().astype(dt) for n in "qkvo"])


def _leaves(mha, X):
    return [X] + [getattr(getattr(mha, n), w) for n in "qkvo" for w in ("weight", "bias")]


def _module(nk, tdev, d, H, Hkv, window, use_rope, packed=True, p=0.0, seed=3, max_pos=320):
    mha = nk.nn.MultiheadAttention(tdev, d, H, p, seed, kv_heads=Hkv)
    mha.causal = True
    mha.window = window
    mha.packed_qkv = packed
    ro = None
    if use_rope:
        mha.rope = nk.nn.RotaryEmbedding(tdev, d // H, max_pos)
        ro = RO.make(max_pos, d // H)
    return mha, ro


def _span(seg, window):
    return min(seg.max_len, window) if window > 0 else seg.max_len


def _oracles(mha, ro, x, g, H, Hkv, batch, lo, pos, span):
    S = x.shape[0] // batch
    refs = []
    for dt in (np.float64, np.float32):
        Wt, Bs = _params(mha, dt)
        refs.append(SO.mha_forward_backward(x.astype(dt), Wt[0], Bs[0], Wt[1], Bs[1], Wt[2], Bs[2], Wt[3], Bs[3], H, Hkv, batch, 0.0,
                                            np.ones((batch * H, S, S), dt), g.astype(dt), lo, span, pos=pos, rope=ro))
    return refs


def _hold(mha, X, y, refs, what):
    (ref, grads), (ref32, grads32) = refs
    assert np.isfinite(y.data()).all() and np.isfinite(X.grad()).all(), what
    _check(y.data(), ref, ref32, "out" + what)
    _check(X.grad(), grads["x"], grads32["x"], "dx" + what)
    for nme in "qkvo":
        _check(getattr(mha, nme).weight.grad(), grads["w" + nme], grads32["w" + nme], "dw" + nme + what)
        _check(getattr(mha, nme).bias.grad(), grads["b" + nme], grads32["b" + nme], "db" + nme + what, np.abs(grads["w" + nme]).max())


def _step(nk, tdev, mha, x, g, batch, seg=None):
    X = nk.from_ndarray(tdev, x).requires_grad()
    y = mha.forward(X, batch) if seg is None else mha.forward(X, batch, seg)
    for leaf in _leaves(mha, X):
        leaf.zero_grad()
    y.forward(); y.backward_from(nk.from_ndarray(tdev, g))
    return X, y


@pytest.mark.parametrize("layer", list(LAYERS))
def test_the_fused_node_against_the_composed_path(nk, tdev, layer):
    """The same call with fused_core = true and false: the fused graph has the node count of the module without segments (ONE core
    node, not the composition), both hold against the oracle in output and every parameter / input gradient, and they agree with
    each other within the rule's bound."""
    d, H, Hkv, S, docs, window, packed, use_rope = LAYERS[layer]
    assert nk.Var.attention_core_supported(S, d // H, 0.0)
    mha, ro = _module(nk, tdev, d, H, Hkv, window, use_rope, packed)
    seg = nk.nn.Segments(tdev, B, S, docs)
    lo, pos, longest = SO.layout(S, docs)
    assert np.array_equal(seg.lo(), lo) and np.array_equal(seg.pos(), pos) and seg.max_len == longest and longest < S
    x, g = rnd(0, (B * S, d), -1, 1), rnd(5, (B * S, d), -1, 1)
    refs = _oracles(mha, ro, x, g, H, Hkv, B, lo, pos, _span(seg, window))
    plain = mha.forward(nk.from_ndarray(tdev, x).requires_grad(), B).history_len()   # (causal or band core: ONE node either way)
    outs = []
    for core in (True, False):
        mha.fused_core = core
        X, y = _step(nk, tdev, mha, x, g, B, seg)
        _hold(mha, X, y, refs, " [%s, %s]" % (layer, "core" if core else "composed"))
        outs.append((y.history_len(), y.data().copy()))
    mha.fused_core = True
    assert outs[1][0] > outs[0][0]
    assert outs[0][0] == plain, (outs[0][0], plain)
    (ref, _), (ref32, _) = refs
    bound = max(2 * np.abs(ref32 - ref).max(), 1e-6 * np.abs(ref).max())
    assert np.abs(outs[0][1] - outs[1][1]).max() <= 2 * bound             # each within `bound` of the f64 oracle
    # the documents are not the triangle
    y0 = mha.forward(nk.from_ndarray(tdev, x).requires_grad(), B); y0.forward()
    assert not np.allclose(y0.data(), outs[0][1], atol=1e-3)


@pytest.mark.parametrize("layer", ["dh 64 packed, rope", "dh 32 strided, rope", "one kv head"])
def test_a_packed_run_is_the_documents_run_one_by_one(nk, tdev, layer):
    """rope set, p = 0: every document alone through the same module (batch = 1, S = its length: positions 0 .. len - 1) - the packed
    run's rows hold against the per-document oracle within the rule, and the parameter gradients against the SUM of the per-document
    gradients.  This is the test that the positions restart: with `pos` ignored the rows of every document but the first differ in
    the first decimals.  The per-document runs on the device agree with the packed rows within twice the bound."""
    d, H, Hkv, S, docs, window, packed, use_rope = LAYERS[layer]
    assert use_rope and window == 0
    mha, ro = _module(nk, tdev, d, H, Hkv, 0, True, packed)
    seg = nk.nn.Segments(tdev, B, S, docs)
    lo, pos, longest = SO.layout(S, docs)
    x, g = rnd(10, (B * S, d), -1, 1), rnd(15, (B * S, d), -1, 1)
    ref, ref32 = np.zeros((B * S, d)), np.zeros((B * S, d), np.float32)
    dx, dx32 = np.zeros((B * S, d)), np.zeros((B * S, d), np.float32)
    sums, sums32, dev_rows = {}, {}, np.zeros((B * S, d), np.float32)
    for b in range(B):
        for start in np.unique(lo[b]):
            rows = np.flatnonzero(lo[b] == start) + b * S
            n = rows.size
            for dt, out, dxs, acc in ((np.float64, ref, dx, sums), (np.float32, ref32, dx32, sums32)):
                Wt, Bs = _params(mha, dt)
                o, grads = WO.mha_forward_backward(x[rows].astype(dt), Wt[0], Bs[0], Wt[1], Bs[1], Wt[2], Bs[2], Wt[3], Bs[3], H, Hkv, 1, 0.0,
                                                   np.ones((H, n, n), dt), g[rows].astype(dt), n, rope=ro)
                out[rows], dxs[rows] = o, grads["x"]
                for key, val in grads.items():
                    if key != "x":
                        acc[key] = acc.get(key, 0) + val
            _, y1 = _step(nk, tdev, mha, x[rows], g[rows], 1)
            dev_rows[rows] = y1.data()
    X, y = _step(nk, tdev, mha, x, g, B, seg)
    what = " [%s, per document]" % layer
    _check(y.data(), ref, ref32, "out" + what)
    _check(X.grad(), dx, dx32, "dx" + what)
    for nme in "qkvo":
        _check(getattr(mha, nme).weight.grad(), sums["w" + nme], sums32["w" + nme], "dw" + nme + what)
        _check(getattr(mha, nme).bias.grad(), sums["b" + nme], sums32["b" + nme], "db" + nme + what, np.abs(sums["w" + nme]).max())
    bound = max(2 * np.abs(ref32 - ref).max(), 1e-6 * np.abs(ref).max())
    assert np.abs(dev_rows - y.data()).max() <= 2 * bound
    # ... and the positions matter: the same run with one document per sample is far from it beyond the first document
    y0 = mha.forward(nk.from_ndarray(tdev, x).requires_grad(), B); y0.forward()
    later = lo.reshape(-1) > 0
    assert np.abs(y0.data()[later] - y.data()[later]).max() > 1e-2


@pytest.mark.parametrize("layer", ["dh 64 packed, rope", "dh 32 strided", "half the kv heads", "with a window"])
def test_one_document_per_sample_is_the_call_without_segments(nk, tdev, layer):
    """max_len >= S: forward(x, batch, seg) builds the nodes of forward(x, batch) - the same history length, the same bits in the
    output and in every gradient."""
    d, H, Hkv, S, _, window, packed, use_rope = LAYERS[layer]
    mha, _ = _module(nk, tdev, d, H, Hkv, window, use_rope, packed)
    seg = nk.nn.Segments(tdev, B, S, [[S], []])                            # (an empty list: the remainder is the one document)
    assert seg.max_len == S and not seg.lo().any() and np.array_equal(seg.pos()[1], np.arange(S))
    x, g = rnd(20, (B * S, d), -1, 1), rnd(25, (B * S, d), -1, 1)
    X0, y0 = _step(nk, tdev, mha, x, g, B)
    want = [y0.data().copy(), X0.grad().copy()] + [leaf.grad().copy() for leaf in _leaves(mha, X0)[1:]]
    X1, y1 = _step(nk, tdev, mha, x, g, B, seg)
    got = [y1.data().copy(), X1.grad().copy()] + [leaf.grad().copy() for leaf in _leaves(mha, X1)[1:]]
    assert y1.history_len() == y0.history_len()
    for a, b_ in zip(got, want):
        assert np.array_equal(a, b_)


@pytest.mark.parametrize("use_rope", [False, True], ids=["plain", "rope"])
def test_an_unsupported_head_size_takes_the_composed_path(nk, tdev, use_rope):
    """dh = 48: the fused core does not apply; the node-by-node path with the per-sample constant holds against the oracle."""
    d, H, S, docs = 192, 4, 100, [[30, 1, 44, 25], [64, 36]]
    assert not nk.Var.attention_core_supported(S, d // H, 0.0)
    mha, ro = _module(nk, tdev, d, H, H, 0, use_rope)
    seg = nk.nn.Segments(tdev, B, S, docs)
    lo, pos, longest = SO.layout(S, docs)
    x, g = rnd(30, (B * S, d), -1, 1), rnd(35, (B * S, d), -1, 1)
    refs = _oracles(mha, ro, x, g, H, H, B, lo, pos, longest)
    X, y = _step(nk, tdev, mha, x, g, B, seg)
    _hold(mha, X, y, refs, " [dh 48%s]" % (", rope" if use_rope else ""))
    fused = nk.nn.MultiheadAttention(tdev, 256, 4, 0.0, 3); fused.causal = True
    n_core = fused.forward(nk.from_ndarray(tdev, rnd(1, (B * S, 256))).requires_grad(), B).history_len()
    assert y.history_len() > n_core


def test_heads_attention_takes_the_segments_with_and_without_gradients(nk, tdev):
    """`Var::heads_attention(..., segments)` without gradients gives the differentiable node's values bit for bit and holds against
    the oracle; one document per sample is the causal node; the evaluation forward can be captured and replays to the same bits."""
    S, H, dh = 200, 2, 64
    d = H * dh
    docs = [[70, 33, 97], [120, 80]]
    scale = float(np.float32(1 / np.sqrt(dh)))
    q, k, v = (rnd(s, (B * S, d), -1, 1) for s in (1, 2, 3))
    status = nk.Status(False)
    seg = nk.nn.Segments(tdev, B, S, docs)
    Q, K, V = (nk.from_ndarray(tdev, t) for t in (q, k, v))
    out = Q.heads_attention(K, V, B, S, H, dh, scale, 0.0, status, True, 0, seg)
    out.forward()
    Qd, Kd, Vd = (nk.from_ndarray(tdev, t).requires_grad() for t in (q, k, v))
    kept = Qd.heads_attention(Kd, Vd, B, S, H, dh, scale, 0.0, status, True, 0, seg)
    kept.forward()
    assert np.array_equal(out.data(), kept.data())
    lo, _, longest = SO.layout(S, docs)
    o, _ = SO.attention_core_forward(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), H, B, 0.0, np.ones((B * H, S, S)), lo, longest)
    np.testing.assert_allclose(out.data(), o, rtol=0, atol=2e-6)          # (|v| <= 1: the causal tape test's bound)
    causal = Q.heads_attention(K, V, B, S, H, dh, scale, 0.0, status, causal=True); causal.forward()
    whole = Q.heads_attention(K, V, B, S, H, dh, scale, 0.0, status, True, 0, nk.nn.Segments(tdev, B, S, [[], []])); whole.forward()
    assert np.array_equal(causal.data(), whole.data())
    want = out.data().copy()
    tdev.graph_begin(); out.forward(); graph = tdev.graph_end()
    graph.launch(); graph.launch()
    assert np.array_equal(out.data(), want)


def test_construction_refuses_stream_capture_and_leaves_the_capture_valid(nk, tdev):
    """`nn.Segments` uploads its arrays with a synchronising copy: between graph_begin and graph_end it raises BEFORE anything touches
    the stream, as nk_rope_table does - the capture still ends, and replays what was captured around the refusal."""
    S = 64
    x = nk.from_ndarray(tdev, rnd(2, (B * S, 32), -1, 1))
    y = x.relu()
    y.forward(); want = y.data().copy()
    tdev.graph_begin()
    y.forward()                            # (something to capture)
    with pytest.raises(RuntimeError, match="nn::Segments"):
        nk.nn.Segments(tdev, B, S, [[10, 20], [64]])
    y.forward()
    graph = tdev.graph_end()
    graph.launch(); graph.launch()
    tdev.sync()
    assert np.array_equal(y.data(), want)
    seg = nk.nn.Segments(tdev, B, S, [[10, 20], [64]])                      # ... and outside a capture it builds as before
    assert seg.max_len == 64 and seg.lo()[0].tolist() == [0] * 10 + [10] * 20 + [30] * 34


def test_what_the_layer_refuses(nk, tdev):
    d, H, S = 128, 4, 64
    x = nk.from_ndarray(tdev, rnd(1, (B * S, d))).requires_grad()
    seg = nk.nn.Segments(tdev, B, S, [[10, 20], [64]])
    mha = nk.nn.MultiheadAttention(tdev, d, H, 0.0, 3)
    with pytest.raises(RuntimeError, match="causal"):
        mha.forward(x, B, seg)
    mha.causal = True
    with pytest.raises(RuntimeError, match="segments were built for"):
        mha.forward(x, B, nk.nn.Segments(tdev, B + 1, S, [[10], [20], [30]]))
    with pytest.raises(RuntimeError, match="segments were built for"):
        mha.forward(x, B, nk.nn.Segments(tdev, B, S + 1, [[10], [20]]))
    mha.rope = nk.nn.RotaryEmbedding(tdev, d // H, 33)
    with pytest.raises(RuntimeError, match="exceeds rope's table"):
        mha.forward(x, B, seg)                                             # sample 1 is one document of 64
    mha.forward(x, B, nk.nn.Segments(tdev, B, S, [[31, 33], [32, 32]]))   # S = 64 > max_pos, every document inside the table
    st = nk.Status(False)
    with pytest.raises(RuntimeError, match="causal"):
        x.heads_attention(x, x, B, S, H, d // H, 0.125, 0.0, st, False, 0, seg)
    for bad, why in (([[10]], "lists of document lengths"), ([[0, 5], [3]], "must be positive"), ([[-2], [3]], "must be positive"),
                     ([[60, 5], [3]], "more than S")):
        with pytest.raises(RuntimeError, match=why):
            nk.nn.Segments(tdev, B, S, bad)
