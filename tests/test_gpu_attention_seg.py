"""GPU parity of packed sequences in the fused core (nk_attention_seg_fwd / _bwd and the packed nk_attention_qkv_seg_*: query r of sample
b attends to keys lo_eff[b][r] .. r, lo_eff = min(r, max(lo, r - span + 1, 0)); the kernels are the band kernels with the left edge
read from a device array) against tests/segment_oracle.py's composition with the per-sample constant, through the C ABI.

Tolerance: tests/test_gpu_attention_band.py's rule, unchanged - kernels and f32 oracle both measured against the f64 oracle fed the
SAME Philox mask; pass iff err_gpu <= max(2 * err_cpu32, 1e-6 * scale) per tensor, margins recorded under `attention_seg:*`.

Scratch contract checked here (include/neuronika_hip.h): the band's geometry at window = span - element (r, k) of scores / dS /
dropped at r * nk_attention_band_ld(S, span) + k of its head's nk_attention_band_scratch(S, span) floats; scores written on the tiles
a wave computes (lo_eff[r0] / 32 .. r0 / 32, -inf at masked positions), dS and Pd defined - exactly 0 at masked positions - on the
128 x 128 blocks a block of queries staged, everything else keeps the sentinel.

Instantiations of attention_band_kernel<BWD, MASKED, OCC, DH, RAGGED, SEG = true> and the case of test_seg_core_equals_oracle that reaches them
(forward and backward alike; MASKED = the (0.1, True) case, unmasked = (0.0, True) and (0.35, False)), ids `p-train-case`:
  DH 64  whole  mixed-160 two-128-256 ones-384 window-320        DH 64  ragged three-197 long-1000
  DH 32  whole  split-384                                       DH 32  ragged small-129
  DH 128 whole  three-512                                       DH 128 ragged three-300
Loop regions (block qb, wave w, tiles of 32 keys):
  zero-only tiles [kt0, lo_w)   two-128-256 (block 1 starts at a document start on a block edge: tiles 0 .. 3 are zero-filled and
                                nothing left of tile 4 is computed), ones-384, three-512, long-1000
  left-edge tiles (EDGE body)   a boundary INSIDE a 32-tile: mixed-160 (7), ones-384 (33, 34, 35, 225), split-384 (130), three-197 (40,
                                80, 5, 105), long-1000 (130, 430); ON a 32-multiple: mixed-160 (32, 64), two-128-256 (128), three-512
                                (256), three-300 (96, 192), small-129 (64)
  whole tiles [left_end, 4 qb)  split-384 (block 2: tiles 5 .. 7 behind the edge at 130), long-1000 (blocks 5 .. 7 of the last document),
                                three-512 (block 3: tiles 8 .. 11)
  the diagonal square           every case
  span < longest document       window-320: lo from documents of 200 and 120 with span = 48 (the clamp adds the sliding window)
Non-uniform rows - the ones that move the softmax shift after a row's first finite tile: tests/test_gpu_attention_band_rows.py."""
import numpy as np
import pytest

from oracle import neuronika_oracle as O
import segment_oracle as SO

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
    record_margin("attention_seg:" + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


class Geometry:
    """The walk of include/neuronika_hip.h for (S, span, lo): per (sample, head) dense (BH, SP, SP) maps `allowed` (lo_eff[r] <= k <= r,
    k < S; a padded query uses the clamped row S - 1), `tile` (the 32 x 32 tiles a wave computes) and `block` (what a block of queries
    stages: where the backward defines dS / Pd - the band's, from span alone), and the gather that turns a head's banded floats into
    the dense (SP, SP) matrix."""

    def __init__(self, S, span, lo, H):
        c = capi()
        B = lo.shape[0]
        self.S, self.span, self.SP, self.BH = S, span, c.attention_padded(S), B * H
        SP = self.SP
        self.ld, self.ext, self.words = c.attention_band_ld(S, span), c.attention_band_scratch(S, span), c.attention_band_mask_words(S, span)
        le = SO.lo_eff(lo, span)                                            # (B, S)
        le = np.concatenate([le, np.repeat(le[:, -1:], SP - S, axis=1)], axis=1)   # padded queries: the clamped row's edge
        r, k = np.arange(SP)[:, None], np.arange(SP)[None, :]
        allowed = (k[None] <= r[None]) & (k[None] >= le[:, :, None]) & (k[None] < S)
        tile, block = np.zeros((B, SP, SP), bool), np.zeros((SP, SP), bool)
        self.tiles = [[] for _ in range(B)]                                 # per sample: (query tile, key tile, first staged tile of the block)
        ntile = SP // 32
        for qb in range((S + 127) // 128):
            js = max(0, 128 * qb - span + 1) // 128
            for w in range(4):
                r0 = 128 * qb + 32 * w
                if r0 >= S:
                    continue
                block[r0:r0 + 32, 128 * js:32 * min(ntile, 4 * qb + 4)] = True
                for b in range(B):
                    first = int(le[b, r0]) // 32
                    assert first >= 4 * js
                    for kt in range(first, 4 * qb + w + 1):
                        tile[b, r0:r0 + 32, 32 * kt:32 * kt + 32] = True
                        self.tiles[b].append((r0 // 32, kt, 4 * js))
        self.allowed, self.tile = np.repeat(allowed, H, axis=0), np.repeat(tile, H, axis=0)
        self.block = np.broadcast_to(block, (self.BH, SP, SP))
        self.H = H
        self.addr = (r * self.ld + k).astype(np.int64)                      # element (r, k) inside a head's extent
        assert self.addr[block].max() < self.ext and np.unique(self.addr[block]).size == block.sum()
        assert not (self.tile & ~self.block).any() and not (self.allowed & ~self.tile).any()
        self.real = np.zeros((self.BH, SP, SP), bool); self.real[:, :S] = True

    def dense(self, flat, where, fill=np.nan):
        """(BH, ext) banded floats -> (BH, SP, SP) with `fill` outside `where` ((BH, SP, SP) bool)"""
        out = np.full((self.BH, self.SP, self.SP), fill, flat.dtype)
        for bh in range(self.BH):
            out[bh][where[bh]] = flat[bh][self.addr[where[bh]]]
        return out

    def untouched(self, flat, where):
        """the floats of every head that no element of `where` lives at"""
        out = []
        for bh in range(self.BH):
            m = np.ones(self.ext, bool)
            m[self.addr[where[bh]]] = False
            out.append(flat[bh][m])
        return np.concatenate(out)

    def unpack(self, words):
        """mask words -> (BH, SP, SP) 0 / 1 on the computed tiles (0 elsewhere), and the words no computed tile owns"""
        w = words.reshape(self.BH, self.SP // 32, self.ld // 32, 32)
        bits = np.zeros((self.BH, self.SP, self.SP), np.uint32)
        others = []
        for bh in range(self.BH):
            owned = np.zeros(w.shape[1:3], bool)
            for qt, kt, kt0 in self.tiles[bh // self.H]:
                owned[qt, kt - kt0] = True
                bits[bh, 32 * qt:32 * qt + 32, 32 * kt:32 * kt + 32] = (w[bh, qt, kt - kt0, :, None] >> np.arange(32, dtype=np.uint32)) & 1
            others.append(w[bh][~owned].reshape(-1))
        return bits, np.concatenate(others)


def _run(dev, B, S, H, dh, lo, span, p, train, seed, offset, assign, q, k, v, g, dq0, fill=SENTINEL):
    """Seg forward + backward; returns the raw banded buffers."""
    c = capi()
    geo = Geometry(S, span, lo, H)
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    SP, BH = geo.SP, B * H
    Q, K, V, G = (dev.array(t) for t in (q, k, v, g))
    LO = dev.int_array(lo)
    scores, stats, out = dev.full((BH, geo.ext), fill), dev.zeros((BH, SP, 2)), dev.zeros((B * S, H * dh))
    bits = dev.zeros((BH, geo.words))
    c.attention_seg_fwd(dev, Q, K, V, LO, scores, stats, bits, out, B, S, H, dh, scale, p, train, seed, offset, span=span)
    dS, dropped, dQ = dev.full((BH, geo.ext), fill), dev.full((BH, geo.ext), fill), dev.array(dq0)
    dK, dV = dev.full((B * S, H * dh), np.nan), dev.full((B * S, H * dh), np.nan)
    c.attention_seg_bwd(dev, dQ, dK, dV, dS, dropped, G, out, scores, stats, bits, Q, K, V, LO, B, S, H, dh, scale, p, train,
                        assign=(assign, True, True), span=span)
    return dict(scores=scores.numpy(), stats=stats.numpy(), out=out.numpy(), bits=bits.numpy().view(np.uint32), d_scores=dS.numpy(),
                dropped=dropped.numpy(), dq=dQ.numpy(), dk=dK.numpy(), dv=dV.numpy()), (Q, K), geo


def _run_band(dev, B, S, H, dh, W, p, seed, offset, q, k, v, g, dq0):
    c = capi()
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    SP, BH = c.attention_padded(S), B * H
    ext, words = c.attention_band_scratch(S, W), c.attention_band_mask_words(S, W)
    Q, K, V, G = (dev.array(t) for t in (q, k, v, g))
    scores, stats, out = dev.full((BH, ext), SENTINEL), dev.zeros((BH, SP, 2)), dev.zeros((B * S, H * dh))
    bits = dev.zeros((BH, words))
    c.attention_band_fwd(dev, Q, K, V, scores, stats, bits, out, B, S, H, dh, scale, p, True, seed, offset, window=W)
    dS, dropped, dQ = dev.full((BH, ext), SENTINEL), dev.full((BH, ext), SENTINEL), dev.array(dq0)
    dK, dV = dev.full((B * S, H * dh), np.nan), dev.full((B * S, H * dh), np.nan)
    c.attention_band_bwd(dev, dQ, dK, dV, dS, dropped, G, out, scores, stats, bits, Q, K, V, B, S, H, dh, scale, p, True,
                         assign=(False, True, True), window=W)
    return dict(scores=scores.numpy(), stats=stats.numpy(), out=out.numpy(), bits=bits.numpy().view(np.uint32), d_scores=dS.numpy(),
                dropped=dropped.numpy(), dq=dQ.numpy(), dk=dK.numpy(), dv=dV.numpy())


def _oracle(B, S, H, lo, span, p, train, seed, offset, q, k, v, g):
    SP = capi().attention_padded(S)
    masked = train and p != 0.0
    noise = (np.ascontiguousarray(O.dropout_noise(B * H * SP * SP, p, seed, offset).reshape(B * H, SP, SP)[:, :S, :S]) if masked
             else np.ones((B * H, S, S), np.float32))
    pe = p if masked else 0.0
    ref, ref32 = {}, {}
    for dt, dst in ((np.float64, ref), (np.float32, ref32)):
        o, cache = SO.attention_core_forward(q.astype(dt), k.astype(dt), v.astype(dt), H, B, pe, noise.astype(dt), lo, span)
        dst.update(O.attention_core_backward(cache, g.astype(dt)), out=o, scores=cache["scores"], dropped=cache["dropped"])
    return ref, ref32, noise, pe


def _terms(ref, pe, q, k, v, g):
    return {"out": np.abs(v).max() / (1 - pe),
            "dq": np.abs(ref["d_scores"]).sum(2).max() * np.abs(k).max(),
            "dk": np.abs(ref["d_scores"]).sum(1).max() * np.abs(q).max(),
            "dv": np.abs(ref["dropped"]).sum(1).max() * np.abs(g).max()}


# name: (B, S, H, dh, document lengths per sample, span or None = the longest document)
CASES = {
    "mixed-160": (2, 160, 2, 64, [[7, 25, 32, 96], [100, 60]], None),
    "two-128-256": (1, 256, 2, 64, [[128, 128]], None),
    "ones-384": (1, 384, 1, 64, [[33, 1, 1, 190, 159]], None),
    "split-384": (1, 384, 2, 32, [[130, 254]], None),
    "three-512": (1, 512, 1, 128, [[200, 56, 256]], None),
    "three-197": (2, 197, 2, 64, [[40, 40, 117], [5, 100, 92]], None),
    "three-300": (1, 300, 2, 128, [[96, 96, 108]], None),
    "small-129": (2, 129, 1, 32, [[5, 124], [64, 65]], None),
    "long-1000": (1, 1000, 1, 64, [[130, 300, 570]], None),
    "window-320": (1, 320, 1, 64, [[200, 120]], 48),
}


def _case(name):
    B, S, H, dh, docs, span = CASES[name]
    lo, _, longest = SO.layout(S, docs)
    return B, S, H, dh, lo, longest if span is None else span


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("p,train", [(0.1, True), (0.0, True), (0.35, False)])
def test_seg_core_equals_oracle(dev, case, p, train):
    c = capi()
    B, S, H, dh, lo, span = _case(case)
    seed, offset = 0x1234567890ABCDEF, 4242
    q, k, v, g = (rnd(s, (B * S, H * dh), -1, 1) for s in (1, 2, 3, 4))
    dq0 = rnd(9, (B * S, H * dh), -1, 1)
    got, (Q, K), geo = _run(dev, B, S, H, dh, lo, span, p, train, seed, offset, False, q, k, v, g, dq0)
    SP, BH = geo.SP, B * H
    masked = train and p != 0.0
    ref, ref32, noise, pe = _oracle(B, S, H, lo, span, p, train, seed, offset, q, k, v, g)
    real = geo.real
    allowS = geo.allowed[:, :S, :S]
    cut = lambda t: t[:, :S, :S]
    # raw scores on the allowed set: the batched GEMM's reduction order -> identical bits; masked positions of the computed tiles hold
    # -inf (keys right of the diagonal, left of the row's edge, padded keys); nothing else was touched
    ref_scores = dev.zeros((BH, S, S))
    c.sgemm_batched(dev, 0, 1, S, S, dh, 1.0, Q, H * dh, S * H * dh, dh, K, H * dh, S * H * dh, dh, 0.0, ref_scores, S, H * S * S, S * S, B, H)
    scores = geo.dense(got["scores"], geo.tile)
    assert np.array_equal(cut(scores)[allowS], ref_scores.numpy()[allowS])
    _check(cut(scores)[allowS], ref["scores"][allowS], ref32["scores"][allowS], "scores")
    assert np.all(np.isneginf(scores[geo.tile & ~geo.allowed & real]))
    assert np.all(geo.untouched(got["scores"], geo.tile) == SENTINEL)
    # dS / Pd: oracle values on the allowed set, exactly 0 at every masked position of a defined block, untouched elsewhere
    for name in ("d_scores", "dropped"):
        t = geo.dense(got[name], geo.block)
        _check(cut(t)[allowS], ref[name][allowS], ref32[name][allowS], name)
        assert not t[geo.block & ~geo.allowed & real].any(), name
        assert np.isfinite(t[geo.block]).all(), name                     # (padded query rows are copies of row S - 1)
        assert np.all(geo.untouched(got[name], geo.block) == SENTINEL), name
    assert np.array_equal(cut(geo.dense(got["dropped"], geo.block))[allowS] == 0, noise[allowS] == 0)   # dropped exactly where the mask says
    if masked:   # mask words of the computed tiles are the shared draw layout at the PADDED S x S position; no other word was written
        unpacked, others = geo.unpack(got["bits"])
        draws = O.dropout_noise(BH * SP * SP, p, seed, offset).reshape(BH, SP, SP) != 0
        assert np.array_equal(unpacked[geo.tile & real] != 0, draws[geo.tile & real])
        assert not others.any()
    else:
        assert not got["bits"].any()
    terms = _terms(ref, pe, q, k, v, g)
    for name in ("out", "dk", "dv"):
        assert np.isfinite(got[name]).all(), name
        _check(got[name], ref[name], ref32[name], name, floor=float(terms[name]))
    _check(got["dq"] - dq0, ref["dq"], ref32["dq"], "dq (accumulated)", floor=max(np.abs(dq0).max(), float(terms["dq"])))
    # row statistics over the unmasked keys: with the scores they reproduce the masked softmax
    s32 = np.float64(np.float32(1.0 / np.sqrt(dh)))
    sc2 = np.where(allowS, ref["scores"] * s32 * np.log2(np.e), -np.inf)
    m2, inv = got["stats"][:, :S, 0].astype(np.float64), got["stats"][:, :S, 1].astype(np.float64)
    assert (m2 >= sc2.max(2) - 6.0 - 1e-4).all() and (m2 <= sc2.max(2) + 1e-4).all()
    z = np.where(allowS, ref["scores"] * s32, -np.inf)
    soft = np.exp(z - z.max(2, keepdims=True)); soft /= soft.sum(2, keepdims=True)
    np.testing.assert_allclose(np.exp2(sc2 - m2[..., None]) * inv[..., None], soft, rtol=2e-5, atol=1e-9)
    # first-write form: dQ assigned, whatever the buffer held
    got2, _, _ = _run(dev, B, S, H, dh, lo, span, p, train, seed, offset, True, q, k, v, g, dq0)
    assert np.array_equal(got2["dq"] + dq0, got["dq"]) or np.abs(got2["dq"] + dq0 - got["dq"]).max() <= 1e-6 * np.abs(dq0).max()
    _check(got2["dq"], ref["dq"], ref32["dq"], "dq (assigned)", floor=float(terms["dq"]))


@pytest.mark.parametrize("B,S,H,dh,W", [(2, 160, 2, 64, 40), (1, 197, 2, 32, 33), (1, 384, 1, 128, 130)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_band_edges_give_the_band_core_to_the_bit(dev, B, S, H, dh, W, p):
    """Bit contract 1: lo = max(0, r - W + 1), and every entry -7 (the clamp makes it that), with span = W: every buffer - scores,
    statistics, mask words, out, dS, Pd, dq, dk, dv - is byte-identical to nk_attention_band_*'s, the untouched sentinel included."""
    seed, offset = 77, 5
    q, k, v, g = (rnd(s_, (B * S, H * dh), -1, 1) for s_ in (11, 12, 13, 14))
    dq0 = rnd(15, (B * S, H * dh), -1, 1)
    want = _run_band(dev, B, S, H, dh, W, p, seed, offset, q, k, v, g, dq0)
    for lo in (SO.band_lo(B, S, W), np.full((B, S), -7, np.int32)):
        got, _, _ = _run(dev, B, S, H, dh, lo, W, p, True, seed, offset, False, q, k, v, g, dq0)
        for name in ("scores", "stats", "bits", "out", "d_scores", "dropped", "dq", "dk", "dv"):   # (in the order they are made)
            assert got[name].tobytes() == want[name].tobytes(), (name, int(lo[0, 0]))


@pytest.mark.parametrize("B,S,H,dh", [(2, 128, 2, 64), (1, 160, 3, 32), (1, 300, 2, 128)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_one_document_with_a_span_that_holds_every_key_is_the_causal_core_to_the_bit(dev, B, S, H, dh, p):
    """span in {S, S + 50} and lo = 0: ld = SP, the causal layouts - and the causal entry points' bits in every buffer."""
    c = capi()
    seed, offset = 77, 5
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    SP, BH = c.attention_padded(S), B * H
    q, k, v, g = (rnd(s_, (B * S, H * dh), -1, 1) for s_ in (11, 12, 13, 14))
    dq0 = rnd(15, (B * S, H * dh), -1, 1)
    Q, K, V, G = (dev.array(t) for t in (q, k, v, g))
    scores, stats, out = dev.full((BH, SP, SP), SENTINEL), dev.zeros((BH, SP, 2)), dev.zeros((B * S, H * dh))
    bits = dev.zeros((BH, SP, SP // 32))
    c.attention_fwd(dev, Q, K, V, scores, stats, bits, out, B, S, H, dh, scale, p, True, seed, offset, causal=True)
    dS, dropped, dQ = dev.full((BH, SP, SP), SENTINEL), dev.full((BH, SP, SP), SENTINEL), dev.array(dq0)
    dK, dV = dev.full((B * S, H * dh), np.nan), dev.full((B * S, H * dh), np.nan)
    c.attention_bwd(dev, dQ, dK, dV, dS, dropped, G, out, scores, stats, bits, Q, K, V, B, S, H, dh, scale, p, True,
                    assign=(False, True, True), causal=True)
    want = dict(scores=scores.numpy(), stats=stats.numpy(), out=out.numpy(), bits=bits.numpy().view(np.uint32), d_scores=dS.numpy(),
                dropped=dropped.numpy(), dq=dQ.numpy(), dk=dK.numpy(), dv=dV.numpy())
    for span in (S, S + 50):
        got, _, geo = _run(dev, B, S, H, dh, np.zeros((B, S), np.int32), span, p, True, seed, offset, False, q, k, v, g, dq0)
        assert geo.ld == SP and geo.ext == SP * SP
        for name in ("out", "dq", "dk", "dv"):
            assert np.array_equal(got[name], want[name]), (name, span)
        assert np.array_equal(got["stats"][:, :S], want["stats"][:, :S]), span
        for name in ("scores", "d_scores", "dropped"):
            assert np.array_equal(got[name].reshape(BH, SP, SP), want[name], equal_nan=True), (name, span)
        assert np.array_equal(got["bits"].reshape(want["bits"].shape), want["bits"]), span


@pytest.mark.parametrize("B,S,H,dh", [(2, 70, 2, 64), (1, 129, 1, 32), (1, 160, 1, 128)])
@pytest.mark.parametrize("edges", ["own row", "2**30"])
@pytest.mark.parametrize("span", [1, 33])
def test_documents_of_one_token(dev, B, S, H, dh, edges, span):
    """lo[r] = r, and every entry 2**30 (the clamp makes it the diagonal): every row has one key, its probability is 1 and its context
    that key's value row, kept or dropped whole.  The expectations of test_a_window_of_one_key: the oracle's dS is an exact zero; here
    it is a rounding of dP, and that rounding is all dQ and dK consist of - both are held to dP's size as the floor."""
    p, seed, offset = 0.25, 5, 0
    lo = np.tile(np.arange(S, dtype=np.int32), (B, 1)) if edges == "own row" else np.full((B, S), 2 ** 30, np.int32)
    q, k, v, g = (rnd(s_, (B * S, H * dh), -1, 1) for s_ in (41, 42, 43, 44))
    got, _, geo = _run(dev, B, S, H, dh, lo, span, p, True, seed, offset, True, q, k, v, g, np.zeros((B * S, H * dh), np.float32))
    ref, ref32, noise, pe = _oracle(B, S, H, lo, span, p, True, seed, offset, q, k, v, g)
    assert not ref["d_scores"].any()
    _check(got["out"], ref["out"], ref32["out"], "out (one token)", floor=float(np.abs(v).max() / (1 - p)))
    _check(got["dv"], ref["dv"], ref32["dv"], "dv (one token)", floor=float(np.abs(g).max() / (1 - p)))
    gh, vh = (O._heads_split(t.astype(np.float64), B, H) for t in (g, v))
    dp_max = np.abs((gh * vh).sum(2)).max() / (1 - p)                     # dPd of (r, r) = dO_r . V_r, dP = dPd * noise
    for name in ("dq", "dk"):
        print(name, "one token: max %.3g against dP %.3g" % (np.abs(got[name]).max(), dp_max))
        assert np.abs(got[name]).max() <= 1e-6 * max(dp_max, 1.0), (name, np.abs(got[name]).max(), dp_max)
    ds = geo.dense(got["d_scores"], geo.block)
    assert np.abs(ds[geo.block & geo.real]).max() <= 1e-6 * max(dp_max, 1.0)
    assert np.isfinite(ds[geo.block]).all()
    # only the diagonal tile of every wave was computed
    assert all(kt == qt for tiles in geo.tiles for qt, kt, _ in tiles)


@pytest.mark.parametrize("case,keep", [("three-197", (0, 1)), ("three-197", (1, 2)), ("three-300", (0, 1)), ("mixed-160", (0, 1)), ("small-129", (0, 1))])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_a_document_does_not_see_its_neighbours(dev, case, keep, p):
    """Bit contract 2: q, k, v and g of every OTHER document (of every sample) replaced by different finite values of magnitude up to
    1e3 - the rows of the kept document (sample, index) are bit-identical in out, dq, dk and dv.  The kept documents start and end
    inside 32-row tiles they share with their neighbours (rows 40 .. 79, 105 .. 196, 96 .. 191, 7 .. 31, 5 .. 128): the masked products are
    exact zeros, and a later document's rows ask for the wave's softmax shift only where they ask whatever they hold.  Finite values only: a NaN in a masked key
    of a shared tile legitimately reaches 0 * NaN, as in the causal core."""
    B, S, H, dh, lo, span = _case(case)
    seed, offset = 31, 7
    b, idx = keep
    starts = np.unique(lo[b])
    mine = np.flatnonzero(lo[b] == starts[idx]) + b * S
    q, k, v, g = (rnd(s_, (B * S, H * dh), -1, 1) for s_ in (61, 62, 63, 64))
    zero = np.zeros((B * S, H * dh), np.float32)
    a, _, _ = _run(dev, B, S, H, dh, lo, span, p, True, seed, offset, True, q, k, v, g, zero)
    others = np.setdiff1d(np.arange(B * S), mine)
    q2, k2, v2, g2 = (t.copy() for t in (q, k, v, g))
    for t, s_ in ((q2, 71), (k2, 72), (v2, 73), (g2, 74)):
        t[others] = rnd(s_, (others.size, H * dh), -1e3, 1e3)
    assert np.abs(q2).max() > 900 and np.isfinite(q2).all()
    b2, _, _ = _run(dev, B, S, H, dh, lo, span, p, True, seed, offset, True, q2, k2, v2, g2, zero)
    for name in ("out", "dq", "dk", "dv"):
        assert np.isfinite(b2[name]).all(), name
        assert np.array_equal(a[name][mine], b2[name][mine]), name
        assert not np.array_equal(a[name][others], b2[name][others]), name


@pytest.mark.parametrize("case", ["three-512", "split-384", "three-300"])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_seg_core_never_reads_an_undefined_element(dev, case, p):
    """Scratch poisoned with NaN before the forward (scores) and the backward (dS, Pd): O, dQ, dK, dV come out finite and within
    tolerance, and NaN is still present exactly outside what the contract defines."""
    B, S, H, dh, lo, span = _case(case)
    seed, offset = 5, 3
    q, k, v, g = (rnd(s_, (B * S, H * dh), -1, 1) for s_ in (51, 52, 53, 54))
    got, _, geo = _run(dev, B, S, H, dh, lo, span, p, True, seed, offset, True, q, k, v, g, np.full((B * S, H * dh), np.nan, np.float32), fill=np.nan)
    ref, ref32, _, pe = _oracle(B, S, H, lo, span, p, True, seed, offset, q, k, v, g)
    assert np.all(np.isnan(geo.untouched(got["scores"], geo.tile)))
    assert not np.isnan(geo.dense(got["scores"], geo.tile)[geo.tile]).any()
    for name in ("d_scores", "dropped"):
        assert np.all(np.isnan(geo.untouched(got[name], geo.block))), name
        assert np.isfinite(geo.dense(got[name], geo.block)[geo.block]).all(), name
    terms = _terms(ref, pe, q, k, v, g)
    for name in ("out", "dq", "dk", "dv"):
        assert np.isfinite(got[name]).all(), name
        _check(got[name], ref[name], ref32[name], name + " (poisoned scratch)", floor=float(terms[name]))


@pytest.mark.parametrize("case", ["mixed-160", "three-197", "three-300", "small-129"])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_seg_core_reads_packed_qkv_bit_for_bit_and_is_deterministic(dev, case, p):
    """nk_attention_qkv_seg_fwd / _bwd on one (B*S, 3*H*dh) array give the bits of nk_attention_seg_fwd / _bwd on three; a second run
    of the unpacked entry points gives the first one's bits in every buffer (no atomics, the dK / dV strips in a fixed order)."""
    c = capi()
    B, S, H, dh, lo, span = _case(case)
    seed, offset = 77, 5
    d = H * dh
    q, k, v, g = (rnd(s_, (B * S, d), -1, 1) for s_ in (11, 12, 13, 14))
    zero = np.zeros((B * S, d), np.float32)
    ref, _, geo = _run(dev, B, S, H, dh, lo, span, p, True, seed, offset, True, q, k, v, g, zero)
    again, _, _ = _run(dev, B, S, H, dh, lo, span, p, True, seed, offset, True, q, k, v, g, zero)
    for name in ref:
        assert ref[name].tobytes() == again[name].tobytes(), name
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    SP, BH = geo.SP, B * H
    QKV, G, LO = dev.array(np.concatenate([q, k, v], axis=1)), dev.array(g), dev.int_array(lo)
    scores, stats, out = dev.full((BH, geo.ext), SENTINEL), dev.zeros((BH, SP, 2)), dev.zeros((B * S, d))
    bits = dev.zeros((BH, geo.words))
    c.attention_qkv_seg_fwd(dev, QKV, LO, scores, stats, bits, out, B, S, H, dh, scale, p, True, seed, offset, span=span)
    dS, dropped = dev.full((BH, geo.ext), SENTINEL), dev.full((BH, geo.ext), SENTINEL)
    dQKV = dev.full((B * S, 3 * d), np.nan)
    c.attention_qkv_seg_bwd(dev, dQKV, dS, dropped, G, out, scores, stats, bits, QKV, LO, B, S, H, dh, scale, p, True, assign=True, span=span)
    assert np.array_equal(out.numpy(), ref["out"]) and np.array_equal(scores.numpy(), ref["scores"])
    assert np.array_equal(stats.numpy()[:, :S], ref["stats"][:, :S]) and np.array_equal(bits.numpy().view(np.uint32), ref["bits"])
    assert np.array_equal(dS.numpy(), ref["d_scores"]) and np.array_equal(dropped.numpy(), ref["dropped"])
    dqkv = dQKV.numpy()
    for i, name in enumerate(("dq", "dk", "dv")):
        assert np.array_equal(dqkv[:, i * d:(i + 1) * d], ref[name]), name
    start = rnd(15, (B * S, 3 * d), -1, 1)   # accumulating form: onto a non-zero start
    D2 = dev.array(start)
    c.attention_qkv_seg_bwd(dev, D2, dS, dropped, G, out, scores, stats, bits, QKV, LO, B, S, H, dh, scale, p, True, assign=False, span=span)
    np.testing.assert_allclose(D2.numpy() - start, dqkv, rtol=0, atol=2e-6 * max(1.0, float(np.abs(dqkv).max())))


def test_seg_core_rejects_what_it_cannot_do(dev):
    """NK_ERR_INVALID, nothing launched, buffers untouched: lo = NULL, span <= 0, an unsupported head size, no kept state, p = 1 in
    training."""
    c = capi()
    S, dh, span = 64, 64, 8
    ext, words = c.attention_band_scratch(S, span), c.attention_band_mask_words(S, span)
    z, o = dev.full((S, dh), 3.0), dev.full((S, dh), SENTINEL)
    lo = dev.int_array(np.zeros((1, S), np.int32))
    sc, st, bits = dev.full((1, ext + 4), SENTINEL), dev.full((1, S, 2), SENTINEL), dev.zeros((1, words))
    ds, pd = dev.full((1, ext + 4), SENTINEL), dev.full((1, ext + 4), SENTINEL)
    fwd = lambda **kw: c.attention_seg_fwd(dev, z, z, z, kw.get("lo", lo), kw.get("scores", sc), kw.get("stats", st), None, o, 1, S, 1,
                                           kw.get("dh", dh), 0.125, kw.get("p", 0.0), True, 0, 0, span=kw.get("span", span))
    bwd = lambda **kw: c.attention_seg_bwd(dev, o, o, o, ds, pd, z, z, sc, st, None, z, z, z, kw.get("lo", lo), 1, S, 1, kw.get("dh", dh), 0.125,
                                           kw.get("p", 0.0), True, assign=(True, True, True), span=kw.get("span", span))
    for call in (fwd, bwd):
        with pytest.raises(RuntimeError, match="left edges"):
            call(lo=None)
        for bad in (0, -3):
            with pytest.raises(RuntimeError, match="must be positive"):
                call(span=bad)
        with pytest.raises(RuntimeError, match="fused attention needs"):
            call(p=1.0)
    z48 = dev.zeros((S, 48))
    with pytest.raises(RuntimeError, match="fused attention needs"):
        c.attention_seg_fwd(dev, z48, z48, z48, lo, sc, st, None, z48, 1, S, 1, 48, 0.1, 0.0, span=span)
    with pytest.raises(RuntimeError, match="fused attention needs"):
        c.attention_seg_bwd(dev, z48, z48, z48, ds, pd, z48, z48, sc, st, None, z48, z48, z48, lo, 1, S, 1, 48, 0.1, 0.0, span=span)
    with pytest.raises(RuntimeError, match="no inference form"):
        fwd(scores=None, stats=None)
    with pytest.raises(RuntimeError, match="mask_bits buffer is needed"):
        fwd(p=0.5)
    with pytest.raises(RuntimeError, match="left edges"):
        c.check(c.lib.nk_attention_qkv_seg_fwd(dev.h, z.p, None, sc.p, st.p, None, o.p, 1, S, 1, dh, span, 0.125, 0.0, 0, 0, 0))
    with pytest.raises(RuntimeError, match="null pointer"):
        c.check(c.lib.nk_attention_qkv_seg_bwd(dev.h, None, ds.p, pd.p, z.p, z.p, sc.p, st.p, None, None, lo.p, 1, S, 1, dh, span, 0.125, 0.0, 0, 1))
    for buf in (o, sc, st, ds, pd):
        assert np.all(buf.numpy() == SENTINEL)
    assert not bits.numpy().any()
