"""GPU parity of the sliding-window fused core (nk_attention_band_fwd / _bwd and the packed nk_attention_qkv_band_*: query r attends
to keys r - W < k <= r; the kernels walk the key tiles between the band's left edge and the diagonal only and keep scores / dS / Pd
in banded scratch) against tests/window_oracle.py's composition with the banded constant in front of the Softmax, through the C ABI.

Tolerance: tests/test_gpu_attention.py's rule - kernels and f32 oracle both measured against the f64 oracle fed the SAME Philox
mask; pass iff err_gpu <= max(2 * err_cpu32, 1e-6 * scale) per tensor (SURVEY.md 8c ii), margins recorded under `attention_band:*`.

Scratch contract checked here (include/neuronika_hip.h): element (r, k) of scores / dS / dropped is at r * ld + k of its head's
nk_attention_band_scratch floats; scores are written on the tiles a wave computes (-inf at masked positions), dS and Pd are defined
- exactly 0 at masked positions - on the 128 x 128 blocks a block of queries staged, everything else keeps the sentinel.

Instantiations of attention_band_kernel<BWD, MASKED, OCC, DH, RAGGED, SEG = false> and the case of test_band_core_equals_oracle that reaches
them (forward and backward alike; MASKED = the (0.1, True) case, unmasked = (0.0, True) and (0.35, False)):
  DH 64  whole  (2,160,2,64,7) (1,160,2,64,32) (1,256,2,64,33) (1,384,1,64,100) (1,512,1,64,129) (1,640,1,64,256)
  DH 64  ragged (2,197,2,64,40) (1,1000,1,64,130)          DH 32  whole (1,384,2,32,128)    DH 32  ragged (2,129,1,32,5)
  DH 128 whole  (1,512,1,128,200)                          DH 128 ragged (1,300,2,128,96)
Non-uniform rows - the ones that move the softmax shift after a row's first finite tile: tests/test_gpu_attention_band_rows.py."""
import numpy as np
import pytest

from oracle import neuronika_oracle as O
import window_oracle as WO

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
    record_margin("attention_band:" + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


class Geometry:
    """The walk of include/neuronika_hip.h for (S, W): dense (SP, SP) maps `band` (r - W < k <= r, k < S), `tile` (the 32 x 32 tiles a
    wave computes) and `block` (what a block of queries stages: where the backward defines dS / Pd), and the gather that turns a head's
    banded floats into the dense (SP, SP) matrix."""

    def __init__(self, S, W):
        c = capi()
        self.S, self.W, self.SP = S, W, c.attention_padded(S)
        SP = self.SP
        self.ld, self.ext, self.words = c.attention_band_ld(S, W), c.attention_band_scratch(S, W), c.attention_band_mask_words(S, W)
        r, k = np.arange(SP)[:, None], np.arange(SP)[None, :]
        self.band = (k <= r) & (k > r - W) & (k < S)
        self.tile, self.block = np.zeros((SP, SP), bool), np.zeros((SP, SP), bool)
        self.tiles = []                                                    # (query tile, key tile, first staged tile of the block)
        ntile = SP // 32
        for qb in range((S + 127) // 128):
            js = max(0, 128 * qb - W + 1) // 128
            for w in range(4):
                r0 = 128 * qb + 32 * w
                if r0 >= S:
                    continue
                self.block[r0:r0 + 32, 128 * js:32 * min(ntile, 4 * qb + 4)] = True
                for kt in range(max(0, r0 - W + 1) // 32, 4 * qb + w + 1):
                    self.tile[r0:r0 + 32, 32 * kt:32 * kt + 32] = True
                    self.tiles.append((r0 // 32, kt, 4 * js))
        self.addr = (r * self.ld + k).astype(np.int64)                     # element (r, k) inside a head's extent
        assert self.addr[self.block].max() < self.ext and np.unique(self.addr[self.block]).size == self.block.sum()

    def dense(self, flat, where, fill=np.nan):
        """(BH, ext) banded floats -> (BH, SP, SP) with `fill` outside `where`"""
        out = np.full((flat.shape[0], self.SP, self.SP), fill, flat.dtype)
        out[:, where] = flat[:, self.addr[where]]
        return out

    def untouched(self, flat, where):
        """the floats of every head that no element of `where` lives at"""
        m = np.ones(self.ext, bool)
        m[self.addr[where]] = False
        return flat[:, m]

    def unpack(self, words, BH):
        """mask words -> (BH, SP, SP) 0 / 1 on the computed tiles (0 elsewhere), and the words no computed tile owns"""
        w = words.reshape(BH, self.SP // 32, self.ld // 32, 32)
        bits = np.zeros((BH, self.SP, self.SP), np.uint32)
        owned = np.zeros(w.shape[1:3], bool)
        for qt, kt, kt0 in self.tiles:
            owned[qt, kt - kt0] = True
            bits[:, 32 * qt:32 * qt + 32, 32 * kt:32 * kt + 32] = (w[:, qt, kt - kt0, :, None] >> np.arange(32, dtype=np.uint32)) & 1
        return bits, w[:, ~owned]


def _run(dev, B, S, H, dh, W, p, train, seed, offset, assign, q, k, v, g, dq0, fill=SENTINEL):
    """Band forward + backward; returns the raw banded buffers."""
    c = capi()
    geo = Geometry(S, W)
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    SP, BH = geo.SP, B * H
    Q, K, V, G = (dev.array(t) for t in (q, k, v, g))
    scores, stats, out = dev.full((BH, geo.ext), fill), dev.zeros((BH, SP, 2)), dev.zeros((B * S, H * dh))
    bits = dev.zeros((BH, geo.words))
    c.attention_band_fwd(dev, Q, K, V, scores, stats, bits, out, B, S, H, dh, scale, p, train, seed, offset, window=W)
    dS, dropped, dQ = dev.full((BH, geo.ext), fill), dev.full((BH, geo.ext), fill), dev.array(dq0)
    dK, dV = dev.full((B * S, H * dh), np.nan), dev.full((B * S, H * dh), np.nan)
    c.attention_band_bwd(dev, dQ, dK, dV, dS, dropped, G, out, scores, stats, bits, Q, K, V, B, S, H, dh, scale, p, train,
                         assign=(assign, True, True), window=W)
    return dict(scores=scores.numpy(), stats=stats.numpy(), out=out.numpy(), bits=bits.numpy().view(np.uint32), d_scores=dS.numpy(),
                dropped=dropped.numpy(), dq=dQ.numpy(), dk=dK.numpy(), dv=dV.numpy()), (Q, K), geo


def _oracle(B, S, H, W, p, train, seed, offset, q, k, v, g):
    SP = capi().attention_padded(S)
    masked = train and p != 0.0
    noise = (np.ascontiguousarray(O.dropout_noise(B * H * SP * SP, p, seed, offset).reshape(B * H, SP, SP)[:, :S, :S]) if masked
             else np.ones((B * H, S, S), np.float32))
    pe = p if masked else 0.0
    ref, ref32 = {}, {}
    for dt, dst in ((np.float64, ref), (np.float32, ref32)):
        o, cache = WO.attention_core_forward(q.astype(dt), k.astype(dt), v.astype(dt), H, B, pe, noise.astype(dt), W)
        dst.update(O.attention_core_backward(cache, g.astype(dt)), out=o, scores=cache["scores"], dropped=cache["dropped"])
    return ref, ref32, noise, pe


def _terms(ref, pe, q, k, v, g):
    return {"out": np.abs(v).max() / (1 - pe),
            "dq": np.abs(ref["d_scores"]).sum(2).max() * np.abs(k).max(),
            "dk": np.abs(ref["d_scores"]).sum(1).max() * np.abs(q).max(),
            "dv": np.abs(ref["dropped"]).sum(1).max() * np.abs(g).max()}


# (B, S, H, dh, W): the smallest shapes that reach each edge of the walk
GEOMETRIES = [(2, 160, 2, 64, 7), (1, 160, 2, 64, 32), (1, 256, 2, 64, 33), (1, 384, 1, 64, 100), (1, 384, 2, 32, 128),
              (1, 512, 1, 64, 129), (1, 512, 1, 128, 200), (2, 197, 2, 64, 40), (1, 300, 2, 128, 96), (2, 129, 1, 32, 5),
              (1, 1000, 1, 64, 130), (1, 640, 1, 64, 256)]


@pytest.mark.parametrize("B,S,H,dh,W", GEOMETRIES)
@pytest.mark.parametrize("p,train", [(0.1, True), (0.0, True), (0.35, False)])
def test_band_core_equals_oracle(dev, B, S, H, dh, W, p, train):
    c = capi()
    seed, offset = 0x1234567890ABCDEF, 4242
    q, k, v, g = (rnd(s, (B * S, H * dh), -1, 1) for s in (1, 2, 3, 4))
    dq0 = rnd(9, (B * S, H * dh), -1, 1)
    got, (Q, K), geo = _run(dev, B, S, H, dh, W, p, train, seed, offset, False, q, k, v, g, dq0)
    SP, BH = geo.SP, B * H
    masked = train and p != 0.0
    ref, ref32, noise, pe = _oracle(B, S, H, W, p, train, seed, offset, q, k, v, g)
    real = np.zeros((SP, SP), bool); real[:S] = True                      # rows of real queries
    bandS = geo.band[:S, :S]
    cut = lambda t: t[:, :S, :S]
    # raw scores on the band: the batched GEMM's reduction order -> identical bits; masked positions of the computed tiles hold -inf
    # (keys right of the diagonal, left of the window, padded keys); nothing else was touched
    ref_scores = dev.zeros((BH, S, S))
    c.sgemm_batched(dev, 0, 1, S, S, dh, 1.0, Q, H * dh, S * H * dh, dh, K, H * dh, S * H * dh, dh, 0.0, ref_scores, S, H * S * S, S * S, B, H)
    scores = geo.dense(got["scores"], geo.tile)
    assert np.array_equal(cut(scores)[:, bandS], ref_scores.numpy()[:, bandS])
    _check(cut(scores)[:, bandS], ref["scores"][:, bandS], ref32["scores"][:, bandS], "scores")
    assert np.all(np.isneginf(scores[:, geo.tile & ~geo.band & real]))
    assert np.all(geo.untouched(got["scores"], geo.tile) == SENTINEL)
    # dS / Pd: oracle values on the band, exactly 0 at every masked position of a defined block, untouched elsewhere
    for name in ("d_scores", "dropped"):
        t = geo.dense(got[name], geo.block)
        _check(cut(t)[:, bandS], ref[name][:, bandS], ref32[name][:, bandS], name)
        assert not t[:, geo.block & ~geo.band & real].any(), name
        assert np.isfinite(t[:, geo.block]).all(), name                  # (padded query rows are copies of row S - 1)
        assert np.all(geo.untouched(got[name], geo.block) == SENTINEL), name
    assert np.array_equal(cut(geo.dense(got["dropped"], geo.block))[:, bandS] == 0, noise[:, bandS] == 0)   # dropped exactly where the mask says
    if masked:   # mask words of the computed tiles are the shared draw layout at the PADDED S x S position; no other word was written
        unpacked, others = geo.unpack(got["bits"], BH)
        draws = O.dropout_noise(BH * SP * SP, p, seed, offset).reshape(BH, SP, SP) != 0
        assert np.array_equal(unpacked[:, geo.tile & real] != 0, draws[:, geo.tile & real])
        assert not others.any()
    else:
        assert not got["bits"].any()
    terms = _terms(ref, pe, q, k, v, g)
    for name in ("out", "dk", "dv"):
        assert np.isfinite(got[name]).all(), name
        _check(got[name], ref[name], ref32[name], name, floor=float(terms[name]))
    _check(got["dq"] - dq0, ref["dq"], ref32["dq"], "dq (accumulated)", floor=max(np.abs(dq0).max(), float(terms["dq"])))
    # row statistics over the unmasked keys: with the scores they reproduce the banded softmax
    s32 = np.float64(np.float32(1.0 / np.sqrt(dh)))
    sc2 = np.where(bandS, ref["scores"] * s32 * np.log2(np.e), -np.inf)
    m2, inv = got["stats"][:, :S, 0].astype(np.float64), got["stats"][:, :S, 1].astype(np.float64)
    assert (m2 >= sc2.max(2) - 6.0 - 1e-4).all() and (m2 <= sc2.max(2) + 1e-4).all()
    z = np.where(bandS, ref["scores"] * s32, -np.inf)
    soft = np.exp(z - z.max(2, keepdims=True)); soft /= soft.sum(2, keepdims=True)
    np.testing.assert_allclose(np.exp2(sc2 - m2[..., None]) * inv[..., None], soft, rtol=2e-5, atol=1e-9)
    # first-write form: dQ assigned, whatever the buffer held
    got2, _, _ = _run(dev, B, S, H, dh, W, p, train, seed, offset, True, q, k, v, g, dq0)
    assert np.array_equal(got2["dq"] + dq0, got["dq"]) or np.abs(got2["dq"] + dq0 - got["dq"]).max() <= 1e-6 * np.abs(dq0).max()
    _check(got2["dq"], ref["dq"], ref32["dq"], "dq (assigned)", floor=float(terms["dq"]))


@pytest.mark.parametrize("B,S,H,dh", [(2, 70, 2, 64), (1, 129, 1, 32), (1, 160, 1, 128)])
def test_a_window_of_one_key(dev, B, S, H, dh):
    """W = 1: every row has one key, its probability is 1 and its context that key's value row, kept or dropped whole.  The oracle's
    dS is an exact zero (P (dP - dP P) with P = 1); here it is a rounding of dP, and that rounding is all dQ and dK consist of: both
    are held to dP's size as the floor, as test_causal_core_degenerate_lengths does."""
    p, seed, offset = 0.25, 5, 0
    q, k, v, g = (rnd(s_, (B * S, H * dh), -1, 1) for s_ in (41, 42, 43, 44))
    got, _, geo = _run(dev, B, S, H, dh, 1, p, True, seed, offset, True, q, k, v, g, np.zeros((B * S, H * dh), np.float32))
    ref, ref32, noise, pe = _oracle(B, S, H, 1, p, True, seed, offset, q, k, v, g)
    assert not ref["d_scores"].any()
    _check(got["out"], ref["out"], ref32["out"], "out (W = 1)", floor=float(np.abs(v).max() / (1 - p)))
    _check(got["dv"], ref["dv"], ref32["dv"], "dv (W = 1)", floor=float(np.abs(g).max() / (1 - p)))
    gh, vh = (O._heads_split(t.astype(np.float64), B, H) for t in (g, v))
    dp_max = np.abs((gh * vh).sum(2)).max() / (1 - p)                     # dPd of (r, r) = dO_r . V_r, dP = dPd * noise
    for name in ("dq", "dk"):
        print(name, "W = 1: max %.3g against dP %.3g" % (np.abs(got[name]).max(), dp_max))
        assert np.abs(got[name]).max() <= 1e-6 * max(dp_max, 1.0), (name, np.abs(got[name]).max(), dp_max)
    # (rows of real queries: a padded query row is scratch - it recomputes row S - 1 under its OWN dropout draws, which is not what
    # the stored context of row S - 1 was made with - and is never read: the dK / dV products stop at row S - 1)
    real = np.zeros_like(geo.block); real[:S] = True
    ds = geo.dense(got["d_scores"], geo.block)
    assert np.abs(ds[:, geo.block & real]).max() <= 1e-6 * max(dp_max, 1.0)
    assert np.isfinite(ds[:, geo.block]).all()


@pytest.mark.parametrize("B,S,H,dh", [(2, 128, 2, 64), (1, 160, 3, 32), (1, 300, 2, 128), (1, 384, 1, 64)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_a_window_that_holds_every_key_is_the_causal_core_to_the_bit(dev, B, S, H, dh, p):
    """W in {S, S + 50}: ld = SP, the causal layouts - and the causal entry points' bits for O, the statistics, dQ, dK, dV, and for
    scores, dS and Pd on the triangle.  This pins the per-tile arithmetic of the band kernels to the causal kernels'."""
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
    r, kk = np.arange(SP)[:, None], np.arange(SP)[None, :]
    low = (kk <= r)[:S, :S]
    for W in (S, S + 50):
        got, _, geo = _run(dev, B, S, H, dh, W, p, True, seed, offset, False, q, k, v, g, dq0)
        assert geo.ld == SP and geo.ext == SP * SP
        for name in ("out", "dq", "dk", "dv"):                            # (first differing tensor first, in the order they are made)
            assert np.array_equal(got[name], want[name]), (name, W)
        assert np.array_equal(got["stats"][:, :S], want["stats"][:, :S]), W
        for name in ("scores", "d_scores", "dropped"):
            assert np.array_equal(got[name].reshape(BH, SP, SP)[:, :S, :S][:, low], want[name][:, :S, :S][:, low]), (name, W)
        # ... and in fact everywhere: the same tiles are visited, the same zero tiles written, the sentinel kept
        for name in ("scores", "d_scores", "dropped"):
            assert np.array_equal(got[name].reshape(BH, SP, SP), want[name], equal_nan=True), (name, W)
        assert np.array_equal(got["bits"].reshape(want["bits"].shape), want["bits"]), W


@pytest.mark.parametrize("B,S,H,dh,W", [(1, 512, 2, 64, 129), (1, 384, 2, 32, 100), (1, 300, 1, 128, 96)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_band_core_never_reads_an_undefined_element(dev, B, S, H, dh, W, p):
    """Scratch poisoned with NaN before the forward (scores) and the backward (dS, Pd): O, dQ, dK, dV come out finite and within
    tolerance, and NaN is still present exactly outside what the contract defines."""
    seed, offset = 5, 3
    q, k, v, g = (rnd(s_, (B * S, H * dh), -1, 1) for s_ in (51, 52, 53, 54))
    got, _, geo = _run(dev, B, S, H, dh, W, p, True, seed, offset, True, q, k, v, g, np.full((B * S, H * dh), np.nan, np.float32), fill=np.nan)
    ref, ref32, _, pe = _oracle(B, S, H, W, p, True, seed, offset, q, k, v, g)
    assert np.all(np.isnan(geo.untouched(got["scores"], geo.tile)))
    assert not np.isnan(geo.dense(got["scores"], geo.tile)[:, geo.tile]).any()
    for name in ("d_scores", "dropped"):
        assert np.all(np.isnan(geo.untouched(got[name], geo.block))), name
        assert np.isfinite(geo.dense(got[name], geo.block)[:, geo.block]).all(), name
    terms = _terms(ref, pe, q, k, v, g)
    for name in ("out", "dq", "dk", "dv"):
        assert np.isfinite(got[name]).all(), name
        _check(got[name], ref[name], ref32[name], name + " (poisoned scratch)", floor=float(terms[name]))


@pytest.mark.parametrize("B,S,H,dh,W", [(2, 160, 2, 64, 40), (1, 197, 2, 32, 33), (1, 384, 1, 128, 130)])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_band_core_reads_packed_qkv_bit_for_bit(dev, B, S, H, dh, W, p):
    """nk_attention_qkv_band_fwd / _bwd on one (B*S, 3*H*dh) array give the bits of nk_attention_band_fwd / _bwd on three."""
    c = capi()
    seed, offset = 77, 5
    d = H * dh
    q, k, v, g = (rnd(s_, (B * S, d), -1, 1) for s_ in (11, 12, 13, 14))
    ref, _, geo = _run(dev, B, S, H, dh, W, p, True, seed, offset, True, q, k, v, g, np.zeros((B * S, d), np.float32))
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    SP, BH = geo.SP, B * H
    QKV, G = dev.array(np.concatenate([q, k, v], axis=1)), dev.array(g)
    scores, stats, out = dev.full((BH, geo.ext), SENTINEL), dev.zeros((BH, SP, 2)), dev.zeros((B * S, d))
    bits = dev.zeros((BH, geo.words))
    c.attention_qkv_band_fwd(dev, QKV, scores, stats, bits, out, B, S, H, dh, scale, p, True, seed, offset, window=W)
    dS, dropped = dev.full((BH, geo.ext), SENTINEL), dev.full((BH, geo.ext), SENTINEL)
    dQKV = dev.full((B * S, 3 * d), np.nan)
    c.attention_qkv_band_bwd(dev, dQKV, dS, dropped, G, out, scores, stats, bits, QKV, B, S, H, dh, scale, p, True, assign=True, window=W)
    assert np.array_equal(out.numpy(), ref["out"]) and np.array_equal(scores.numpy(), ref["scores"])
    assert np.array_equal(stats.numpy()[:, :S], ref["stats"][:, :S]) and np.array_equal(bits.numpy().view(np.uint32), ref["bits"])
    assert np.array_equal(dS.numpy(), ref["d_scores"]) and np.array_equal(dropped.numpy(), ref["dropped"])
    dqkv = dQKV.numpy()
    for i, name in enumerate(("dq", "dk", "dv")):
        assert np.array_equal(dqkv[:, i * d:(i + 1) * d], ref[name]), name
    start = rnd(15, (B * S, 3 * d), -1, 1)   # accumulating form: onto a non-zero start
    D2 = dev.array(start)
    c.attention_qkv_band_bwd(dev, D2, dS, dropped, G, out, scores, stats, bits, QKV, B, S, H, dh, scale, p, True, assign=False, window=W)
    np.testing.assert_allclose(D2.numpy() - start, dqkv, rtol=0, atol=2e-6 * max(1.0, float(np.abs(dqkv).max())))


def test_band_core_is_deterministic(dev):
    """(2, 1024, 4, 64), W = 256, p = 0.1: two runs agree BIT for bit in every buffer - no atomics anywhere, the dK / dV strips are
    batched products in a fixed order."""
    B, S, H, dh, W, p, seed = 2, 1024, 4, 64, 256, 0.1, 4711
    q, k, v, g = (rnd(s_, (B * S, H * dh), -1, 1) for s_ in (31, 32, 33, 34))
    dq0 = np.zeros((B * S, H * dh), np.float32)
    a, _, _ = _run(dev, B, S, H, dh, W, p, True, seed, 0, True, q, k, v, g, dq0)
    b, _, _ = _run(dev, B, S, H, dh, W, p, True, seed, 0, True, q, k, v, g, dq0)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    c2, _, _ = _run(dev, B, S, H, dh, W, p, True, seed, 1 << 24, True, q, k, v, g, dq0)
    assert not np.array_equal(a["bits"], c2["bits"])


def test_band_core_rejects_what_it_cannot_do(dev):
    """NK_ERR_INVALID, buffers untouched: window <= 0, an unsupported head size, misaligned pointers, no kept state."""
    c = capi()
    S, dh, W = 64, 64, 8
    ext, words = c.attention_band_scratch(S, W), c.attention_band_mask_words(S, W)
    z, o = dev.full((S, dh), 3.0), dev.full((S, dh), SENTINEL)
    sc, st, bits = dev.full((1, ext + 4), SENTINEL), dev.full((1, S, 2), SENTINEL), dev.zeros((1, words))
    ds, pd = dev.full((1, ext + 4), SENTINEL), dev.full((1, ext + 4), SENTINEL)
    fwd = lambda **kw: c.attention_band_fwd(dev, kw.get("Q", z), z, z, kw.get("scores", sc), kw.get("stats", st), kw.get("bits", None), o, 1, S, 1,
                                            kw.get("dh", dh), kw.get("scale", 0.125), kw.get("p", 0.0), kw.get("train", True), 0, 0,
                                            window=kw.get("W", W))
    bwd = lambda **kw: c.attention_band_bwd(dev, o, o, o, kw.get("dS", ds), pd, z, z, sc, st, None, z, z, z, 1, S, 1, kw.get("dh", dh), 0.125, 0.0, True,
                                            assign=(True, True, True), window=kw.get("W", W))
    for bad in (0, -3):
        with pytest.raises(RuntimeError, match="window must be positive"):
            fwd(W=bad)
        with pytest.raises(RuntimeError, match="window must be positive"):
            bwd(W=bad)
    z96 = dev.zeros((S, 96))
    with pytest.raises(RuntimeError, match="fused attention needs"):
        c.attention_band_fwd(dev, z96, z96, z96, sc, st, None, z96, 1, S, 1, 96, 0.1, 0.0, window=W)
    with pytest.raises(RuntimeError, match="fused attention needs"):
        fwd(p=1.0)
    with pytest.raises(RuntimeError, match="Wrong probability"):
        fwd(p=1.5)
    with pytest.raises(RuntimeError, match="mask_bits buffer is needed"):
        fwd(p=0.5)
    with pytest.raises(RuntimeError, match="positive finite scale"):
        fwd(scale=-0.1)
    with pytest.raises(RuntimeError, match="no inference form"):
        fwd(scores=None, stats=None)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        fwd(scores=sc.view_offset(1))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        fwd(Q=dev.full((S * dh + 4,), 3.0).view_offset(1))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        bwd(dS=ds.view_offset(2))
    with pytest.raises(RuntimeError, match="null pointer"):
        c.check(c.lib.nk_attention_qkv_band_fwd(dev.h, None, sc.p, st.p, None, o.p, 1, S, 1, dh, 0.125, 0.0, 0, 0, 0, W))
    for buf in (o, sc, st, ds, pd):
        assert np.all(buf.numpy() == SENTINEL)
    assert not bits.numpy().any()
