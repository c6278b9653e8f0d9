"""GPU parity of the CAUSAL fused attention core (nk_attention_causal_fwd / _bwd and the packed nk_attention_qkv_causal_*: query r
attends to keys <= r; the kernels walk the key tiles on and below the diagonal only) against the oracle's node-by-node
composition with the mask added in front of the Softmax (tests/causal_oracle.py), through the C ABI.

Tolerance: tests/test_gpu_attention.py's rule - kernels and f32 oracle both measured against the f64 oracle fed the SAME Philox
mask; pass iff err_gpu <= max(2 * err_cpu32, 1e-6 * scale) per tensor (SURVEY.md 8c ii), margins recorded under
`attention_causal:*`.

Scratch contract checked here (include/neuronika_hip.h): scores / dS / dropped tiles strictly above the diagonal are neither
written nor read; inside a visited tile a masked score is -inf; dS and Pd are defined - and exactly 0 at masked positions - on
every 128 x 128 block that touches or lies below the diagonal."""
import numpy as np
import pytest

from oracle import neuronika_oracle as O
import causal_oracle as CO

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def capi():
    from neuronika_amd import capi as c
    return c


def rnd(seed, shape, lo, hi):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(hi - lo) + np.float32(lo), dtype=np.float32)


def _check(got, want64, want32, what, floor=0.0):
    scale = max(np.abs(want64).max(), floor)
    err_gpu, err_cpu = np.abs(got - want64).max(), np.abs(want32 - want64).max()
    from conftest import record_margin
    record_margin("attention_causal:" + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


def _regions(S, SP):
    """Boolean (SP, SP) maps: `low` key <= query; `tile` the 32 x 32 tiles the forward visits (on or below the diagonal);
    `block` the 128 x 128 blocks that touch or lie below the diagonal (where the backward defines dS / Pd)."""
    r, k = np.arange(SP)[:, None], np.arange(SP)[None, :]
    return k <= r, (k // 32) <= (r // 32), (k // 128) <= (r // 128)


def _run(dev, B, S, H, p, train, seed, offset, assign, q, k, v, g, dq0, dh=64, fill=SENTINEL):
    """Causal forward + backward; returns the whole padded (B*H, SP, SP) scratch tensors."""
    c = capi()
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    SP = c.attention_padded(S)
    Q, K, V, G = (dev.array(t) for t in (q, k, v, g))
    scores, stats, out = dev.full((B * H, SP, SP), fill), dev.zeros((B * H, SP, 2)), dev.zeros((B * S, H * dh))
    bits = dev.zeros((B * H, SP, SP // 32))
    c.attention_fwd(dev, Q, K, V, scores, stats, bits, out, B, S, H, dh, scale, p, train, seed, offset, causal=True)
    dS, dropped, dQ = dev.full((B * H, SP, SP), fill), dev.full((B * H, SP, SP), fill), dev.array(dq0)
    dK, dV = dev.full((B * S, H * dh), np.nan), dev.full((B * S, H * dh), np.nan)
    c.attention_bwd(dev, dQ, dK, dV, dS, dropped, G, out, scores, stats, bits, Q, K, V, B, S, H, dh, scale, p, train,
                    assign=(assign, True, True), causal=True)
    return dict(scores=scores.numpy(), stats=stats.numpy(), out=out.numpy(), bits=bits.numpy().view(np.uint32), d_scores=dS.numpy(),
                dropped=dropped.numpy(), dq=dQ.numpy(), dk=dK.numpy(), dv=dV.numpy()), (Q, K)


def _oracle(B, S, H, p, train, seed, offset, q, k, v, g):
    SP = capi().attention_padded(S)
    masked = train and p != 0.0
    noise = (np.ascontiguousarray(O.dropout_noise(B * H * SP * SP, p, seed, offset).reshape(B * H, SP, SP)[:, :S, :S]) if masked
             else np.ones((B * H, S, S), np.float32))
    pe = p if masked else 0.0
    ref, ref32 = {}, {}
    for dt, dst in ((np.float64, ref), (np.float32, ref32)):
        o, cache = CO.attention_core_forward(q.astype(dt), k.astype(dt), v.astype(dt), H, B, pe, noise.astype(dt))
        dst.update(O.attention_core_backward(cache, g.astype(dt)), out=o, scores=cache["scores"], dropped=cache["dropped"])
    return ref, ref32, noise, pe


# whole blocks (128, 256, 384), whole tiles but not whole blocks (32, 96, 160), ragged (7, 33, 100, 129, 197, 1000), every head size
# (S = 1 and S = 2, where a one-key row's score gradient is an exact zero in the oracle and a rounding of dP here, and that rounding
# is most of what dQ / dK consist of: test_causal_core_degenerate_lengths, measured against dP's size as in test_gpu_attention.py)
GEOMETRIES = [(2, 128, 2, 64), (1, 256, 2, 64), (1, 384, 1, 64), (3, 32, 1, 64), (2, 96, 2, 64), (1, 160, 3, 64),
              (2, 128, 2, 32), (1, 160, 3, 32), (1, 256, 1, 32), (2, 128, 2, 128), (1, 160, 3, 128), (1, 256, 1, 128),
              (2, 7, 2, 64), (3, 33, 1, 128), (3, 100, 3, 64), (2, 129, 1, 64), (1, 197, 2, 64),
              (2, 100, 2, 32), (2, 129, 1, 32), (2, 197, 2, 128), (1, 1000, 2, 64)]


@pytest.mark.parametrize("B,S,H,dh", GEOMETRIES)
@pytest.mark.parametrize("p,train", [(0.1, True), (0.0, True), (0.35, False), (0.5, True)])
def test_causal_core_equals_oracle(dev, B, S, H, dh, p, train):
    c = capi()
    seed, offset = 0x1234567890ABCDEF, 4242
    q, k, v, g = (rnd(s, (B * S, H * dh), -1, 1) for s in (1, 2, 3, 4))
    dq0 = rnd(9, (B * S, H * dh), -1, 1)
    got, (Q, K) = _run(dev, B, S, H, p, train, seed, offset, False, q, k, v, g, dq0, dh)
    SP = c.attention_padded(S)
    masked = train and p != 0.0
    ref, ref32, noise, pe = _oracle(B, S, H, p, train, seed, offset, q, k, v, g)
    low, tile, block = _regions(S, SP)
    lowS, tileS, blockS = low[:S, :S], tile[:S, :S], block[:S, :S]
    cut = lambda t: t[:, :S, :S]
    # raw scores on and below the diagonal: same MFMA reduction order as the batched GEMM -> identical bits; masked positions of
    # the visited tiles hold -inf; the tiles above were never touched
    ref_scores = dev.zeros((B * H, S, S))
    c.sgemm_batched(dev, 0, 1, S, S, dh, 1.0, Q, H * dh, S * H * dh, dh, K, H * dh, S * H * dh, dh, 0.0, ref_scores, S, H * S * S, S * S, B, H)
    assert np.array_equal(cut(got["scores"])[:, lowS], ref_scores.numpy()[:, lowS])
    _check(cut(got["scores"])[:, lowS], ref["scores"][:, lowS], ref32["scores"][:, lowS], "scores")
    assert np.all(np.isneginf(got["scores"][:, tile & ~low]))
    assert np.all(got["scores"][:, ~tile] == SENTINEL)
    # padded keys (ragged S) of the real queries, where the tile is visited: -inf as in the non-causal kernels
    padk = np.zeros_like(low); padk[:S, S:] = True
    assert np.all(np.isneginf(got["scores"][:, padk & tile]))
    # dS / Pd: oracle values on and below the diagonal, exactly 0 at every masked position of a defined block, untouched above
    for name in ("d_scores", "dropped"):
        _check(cut(got[name])[:, lowS], ref[name][:, lowS], ref32[name][:, lowS], name)
        assert not got[name][:, block & ~low].any(), name
        assert not got[name][:, padk & block].any(), name
        assert np.all(got[name][:, ~block] == SENTINEL), name
    assert np.array_equal(cut(got["dropped"])[:, lowS] == 0, noise[:, lowS] == 0)   # dropped exactly where the mask says
    if masked:   # mask words of the visited tiles are the shared draw layout; the words of skipped tiles were never written
        w = got["bits"].reshape(B * H, SP // 32, SP // 32, 32).transpose(0, 1, 3, 2).reshape(B * H, SP, SP // 32)
        unpacked = ((w[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B * H, SP, SP)
        draws = O.dropout_noise(B * H * SP * SP, p, seed, offset).reshape(B * H, SP, SP) != 0
        rows = np.arange(SP) < S   # (the words of padded query rows are scratch)
        assert np.array_equal(unpacked[:, tile & rows[:, None]], draws[:, tile & rows[:, None]])
        assert not unpacked[:, ~tile].any()
    terms = {"out": np.abs(v).max() / (1 - pe),
             "dq": np.abs(ref["d_scores"]).sum(2).max() * np.abs(k).max(),
             "dk": np.abs(ref["d_scores"]).sum(1).max() * np.abs(q).max(),
             "dv": np.abs(ref["dropped"]).sum(1).max() * np.abs(g).max()}
    for name in ("out", "dk", "dv"):
        assert np.isfinite(got[name]).all(), name
        _check(got[name], ref[name], ref32[name], name, floor=float(terms[name]))
    _check(got["dq"] - dq0, ref["dq"], ref32["dq"], "dq (accumulated)", floor=max(np.abs(dq0).max(), float(terms["dq"])))
    # row statistics over the unmasked keys: with the scores they reproduce the causal softmax
    c1 = np.float64(np.float32(1.0 / np.sqrt(dh))) * np.log2(np.e)
    sc2 = np.where(lowS, ref["scores"] * c1, -np.inf)
    m2, inv = got["stats"][:, :S, 0].astype(np.float64), got["stats"][:, :S, 1].astype(np.float64)
    assert (m2 >= sc2.max(2) - 6.0 - 1e-4).all() and (m2 <= sc2.max(2) + 1e-4).all()
    z = np.where(lowS, ref["scores"] * np.float64(np.float32(1.0 / np.sqrt(dh))), -np.inf)
    soft = np.exp(z - z.max(2, keepdims=True)); soft /= soft.sum(2, keepdims=True)
    np.testing.assert_allclose(np.exp2(sc2 - m2[..., None]) * inv[..., None], soft, rtol=2e-5, atol=1e-9)
    # first-write form: dQ assigned, whatever the buffer held
    got2, _ = _run(dev, B, S, H, p, train, seed, offset, True, q, k, v, g, dq0, dh)
    assert np.array_equal(got2["dq"] + dq0, got["dq"]) or np.abs(got2["dq"] + dq0 - got["dq"]).max() <= 1e-6 * np.abs(dq0).max()
    _check(got2["dq"], ref["dq"], ref32["dq"], "dq (assigned)", floor=float(terms["dq"]))


@pytest.mark.parametrize("B,S,H,dh", [(2, 256, 2, 64), (1, 384, 2, 32), (1, 300, 2, 128), (2, 160, 1, 64), (1, 1000, 1, 64)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_causal_core_never_reads_an_undefined_block(dev, B, S, H, dh, p):
    """Scratch poisoned with NaN before the forward (scores) and the backward (dS, Pd): O, dQ, dK, dV come out finite and within
    tolerance - the dK / dV products reduce over the queries from a key strip's first row on and never touch the blocks above the
    diagonal (NaN times zero would be NaN)."""
    seed, offset = 5, 3
    q, k, v, g = (rnd(s_, (B * S, H * dh), -1, 1) for s_ in (51, 52, 53, 54))
    got, _ = _run(dev, B, S, H, p, True, seed, offset, True, q, k, v, g, np.full((B * S, H * dh), np.nan, np.float32), dh, fill=np.nan)
    ref, ref32, _, pe = _oracle(B, S, H, p, True, seed, offset, q, k, v, g)
    SP = capi().attention_padded(S)
    _, tile, block = _regions(S, SP)
    assert np.all(np.isnan(got["scores"][:, ~tile])) and np.all(np.isnan(got["d_scores"][:, ~block])) and np.all(np.isnan(got["dropped"][:, ~block]))
    assert np.isfinite(got["d_scores"][:, block]).all() and np.isfinite(got["dropped"][:, block]).all()
    terms = {"out": np.abs(v).max() / (1 - pe),
             "dq": np.abs(ref["d_scores"]).sum(2).max() * np.abs(k).max(),
             "dk": np.abs(ref["d_scores"]).sum(1).max() * np.abs(q).max(),
             "dv": np.abs(ref["dropped"]).sum(1).max() * np.abs(g).max()}
    for name in ("out", "dq", "dk", "dv"):
        assert np.isfinite(got[name]).all(), name
        _check(got[name], ref[name], ref32[name], name + " (poisoned scratch)", floor=float(terms[name]))


@pytest.mark.parametrize("B,S,H,dh", [(2, 128, 2, 64), (1, 160, 3, 32), (2, 100, 2, 64), (1, 96, 2, 128), (3, 33, 1, 64), (1, 1024, 4, 64)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_causal_core_reads_packed_qkv_bit_for_bit(dev, B, S, H, dh, p):
    """nk_attention_qkv_causal_fwd / _bwd on one (B*S, 3*H*dh) array give the bits of nk_attention_causal_fwd / _bwd on three."""
    c = capi()
    seed, offset = 77, 5
    d = H * dh
    q, k, v, g = (rnd(s_, (B * S, d), -1, 1) for s_ in (11, 12, 13, 14))
    ref, _ = _run(dev, B, S, H, p, True, seed, offset, True, q, k, v, g, np.zeros((B * S, d), np.float32), dh)
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    SP = c.attention_padded(S)
    QKV, G = dev.array(np.concatenate([q, k, v], axis=1)), dev.array(g)
    scores, stats, out = dev.full((B * H, SP, SP), SENTINEL), dev.zeros((B * H, SP, 2)), dev.zeros((B * S, d))
    bits = dev.zeros((B * H, SP, SP // 32))
    c.attention_qkv_fwd(dev, QKV, scores, stats, bits, out, B, S, H, dh, scale, p, True, seed, offset, causal=True)
    dS, dropped = dev.full((B * H, SP, SP), SENTINEL), dev.full((B * H, SP, SP), SENTINEL)
    dQKV = dev.full((B * S, 3 * d), np.nan)
    c.attention_qkv_bwd(dev, dQKV, dS, dropped, G, out, scores, stats, bits, QKV, B, S, H, dh, scale, p, True, assign=True, causal=True)
    assert np.array_equal(out.numpy(), ref["out"]) and np.array_equal(scores.numpy(), ref["scores"])
    assert np.array_equal(stats.numpy()[:, :S], ref["stats"][:, :S]) and np.array_equal(bits.numpy().view(np.uint32), ref["bits"])
    assert np.array_equal(dS.numpy(), ref["d_scores"]) and np.array_equal(dropped.numpy(), ref["dropped"])
    dqkv = dQKV.numpy()
    for i, name in enumerate(("dq", "dk", "dv")):
        assert np.array_equal(dqkv[:, i * d:(i + 1) * d], ref[name]), name
    start = rnd(15, (B * S, 3 * d), -1, 1)   # accumulating form: onto a non-zero start
    D2 = dev.array(start)
    c.attention_qkv_bwd(dev, D2, dS, dropped, G, out, scores, stats, bits, QKV, B, S, H, dh, scale, p, True, assign=False, causal=True)
    np.testing.assert_allclose(D2.numpy() - start, dqkv, rtol=0, atol=2e-6 * max(1.0, float(np.abs(dqkv).max())))


@pytest.mark.parametrize("dh", [64, 32, 128])
@pytest.mark.parametrize("S", [1, 2])
def test_causal_core_degenerate_lengths(dev, dh, S):
    """S = 1: causal and full attention are the same function (bit for bit).  S = 2: the first query of a sample sees one key (its
    context is that key's value row, kept or dropped whole), the second sees both."""
    c = capi()
    B, H, p, seed, offset = 3, 2, 0.25, 5, 0
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    q, k, v, g = (rnd(s_, (B * S, H * dh), -1, 1) for s_ in (41, 42, 43, 44))
    got, (Q, K) = _run(dev, B, S, H, p, True, seed, offset, True, q, k, v, g, np.zeros((B * S, H * dh), np.float32), dh)
    noise = O.dropout_noise(B * H * 32 * 32, p, seed, offset).reshape(B * H, 32, 32)
    keep0 = np.repeat(noise[:, 0, 0].reshape(B, H), dh, axis=1) / (np.float32(1) - np.float32(p))   # draw of (query 0, key 0)
    np.testing.assert_allclose(got["out"][::S], v[::S] * keep0, rtol=2e-7, atol=0)
    if S == 1:
        V = dev.array(v)
        scores, stats, bits, full = dev.zeros((B * H, 32, 32)), dev.zeros((B * H, 32, 2)), dev.zeros((B * H, 32, 1)), dev.zeros((B, H * dh))
        c.attention_fwd(dev, Q, K, V, scores, stats, bits, full, B, 1, H, dh, scale, p, True, seed, offset)
        assert np.array_equal(full.numpy(), got["out"])
        np.testing.assert_allclose(got["dv"], g * keep0, rtol=2e-7, atol=0)
        dp_max = np.abs((g.astype(np.float64) * v).reshape(B, H, dh).sum(2)).max() / (1 - p)   # dS = P (dP - sum dP P) cancels: measured against dP
        for name in ("dq", "dk"):
            assert np.abs(got[name]).max() <= 1e-6 * max(dp_max, 1.0), (name, np.abs(got[name]).max(), dp_max)
        assert np.abs(got["d_scores"][:, 0, 0]).max() <= 1e-6 * max(dp_max, 1.0)
    else:
        ref, ref32, _, pe = _oracle(B, S, H, p, True, seed, offset, q, k, v, g)
        for name in ("out", "dv", "dq", "dk"):
            _check(got[name], ref[name], ref32[name], name + " (S = 2)", floor=1.0)


@pytest.mark.parametrize("S,p,train,dh", [(128, 0.0, True, 64), (96, 0.3, False, 64), (256, 0.0, True, 32), (100, 0.0, True, 64), (45, 0.2, False, 32),
                                          (70, 0.0, True, 128), (384, 0.2, True, 64), (197, 0.4, True, 128)])
def test_causal_forward_without_kept_state_is_the_same_forward(dev, S, p, train, dh):
    """Inference form (scores = stats = mask_bits = NULL): the output is bit-identical to the training-graph form's, with dropout
    inactive and (same Philox stream) active."""
    c = capi()
    B, H, seed, offset = 2, 2, 31337, 9
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    q, k, v = (rnd(s_, (B * S, H * dh), -1, 1) for s_ in (21, 22, 23))
    Q, K, V = dev.array(q), dev.array(k), dev.array(v)
    SP = c.attention_padded(S)
    scores, stats, bits = dev.zeros((B * H, SP, SP)), dev.zeros((B * H, SP, 2)), dev.zeros((B * H, SP, SP // 32))
    kept, lean = dev.zeros((B * S, H * dh)), dev.zeros((B * S, H * dh))
    c.attention_fwd(dev, Q, K, V, scores, stats, bits, kept, B, S, H, dh, scale, p, train, seed, offset, causal=True)
    c.attention_fwd(dev, Q, K, V, None, None, None, lean, B, S, H, dh, scale, p, train, seed, offset, causal=True)
    assert np.array_equal(kept.numpy(), lean.numpy())
    with pytest.raises(RuntimeError, match="kept together"):
        c.attention_fwd(dev, Q, K, V, scores, None, None, lean, B, S, H, dh, scale, p, train, seed, offset, causal=True)


def test_causal_core_is_deterministic_at_benchmark_width(dev):
    """B = 32, S = 1024 (the C5 width: blocks of one head walk 4 .. 32 key tiles): two runs agree BIT for bit in every output the
    kernels define - no atomics anywhere, the dK / dV strips are batched products in a fixed order."""
    B, S, H, p, seed = 32, 1024, 1, 0.1, 4711
    q, k, v, g = (rnd(s_, (B * S, H * 64), -1, 1) for s_ in (31, 32, 33, 34))
    dq0 = np.zeros((B * S, H * 64), np.float32)
    a, _ = _run(dev, B, S, H, p, True, seed, 0, True, q, k, v, g, dq0)
    b, _ = _run(dev, B, S, H, p, True, seed, 0, True, q, k, v, g, dq0)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    c2, _ = _run(dev, B, S, H, p, True, seed, 1 << 24, True, q, k, v, g, dq0)
    assert not np.array_equal(a["bits"], c2["bits"])


def test_causal_core_rejects_what_it_cannot_do(dev):
    c = capi()
    z = dev.zeros((64, 96))
    sc, st = dev.zeros((1, 64, 64)), dev.zeros((1, 64, 2))
    with pytest.raises(RuntimeError, match="fused attention needs"):
        c.attention_fwd(dev, z, z, z, sc, st, None, z, 1, 64, 1, 96, 0.1, 0.0, causal=True)
    z64 = dev.zeros((64, 64))
    with pytest.raises(RuntimeError, match="fused attention needs"):
        c.attention_fwd(dev, z64, z64, z64, sc, st, None, z64, 1, 64, 1, 64, 0.1, 1.0, True, causal=True)
    with pytest.raises(RuntimeError, match="Wrong probability"):
        c.attention_fwd(dev, z64, z64, z64, sc, st, None, z64, 1, 64, 1, 64, 0.1, 1.5, causal=True)
    with pytest.raises(RuntimeError, match="mask_bits buffer is needed"):
        c.attention_fwd(dev, z64, z64, z64, sc, st, None, z64, 1, 64, 1, 64, 0.1, 0.5, causal=True)
    with pytest.raises(RuntimeError, match="positive finite scale"):
        c.attention_fwd(dev, z64, z64, z64, sc, st, None, z64, 1, 64, 1, 64, -0.1, 0.0, causal=True)
    with pytest.raises(RuntimeError, match="null pointer"):
        c.check(c.lib.nk_attention_qkv_causal_fwd(dev.h, None, sc.p, st.p, None, z64.p, 1, 64, 1, 64, 0.125, 0.0, 0, 0, 0))
