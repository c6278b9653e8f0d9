"""Parity of the MFMA kernels by dispatch branch: the GEMM tile / loader / epilogue grid, every attention instantiation (forward and
backward), and the convolution instantiations the rest of the suite never enters (tests/dispatch_paths_mfma.py is the inventory;
profiles/r11_suite_kernels_entered.md is the measurement it was written from).

nk_gemm / nk_conv / nk_attention pick a template instantiation from layouts, extents, alignment, channel counts, strides, the
sequence length and the per-handle nk_dev_tune knobs.  Each grid below is read off those conditions and steers by a natural geometry
where a small one takes the branch, by the knob (reset in a `finally`) where only a large problem would.  Every case

  * is compared with a float64 restatement of the same operation: GEMM through tolerance.assert_contraction with the real K and the
    operands' real maxima (and bit for bit with oracle/device_order_sgemm.c where the summation-order contract applies), attention
    against the oracle's node-by-node composition fed the same Philox mask, convolution inside the contraction bound AND - on
    small-integer data, where every f32 sum is exact - equal to the oracle and to a different kernel family;
  * writes into a window inside a larger allocation whose sentinel cells must survive (GEMM, convolution);
  * runs `+=` from a random destination and the first-write twin from NaN;
  * uses inputs that depend on the flat index, so a swapped row or lane changes the result.

All calls go through neuronika_amd.capi.  Only host-side rejections are provoked.  Nothing here is larger than 20 MiB."""
import numpy as np
import pytest

import causal_oracle as CO
import tolerance
from oracle import neuronika_oracle as O
from test_gpu_dispatch_paths import Window, bits, pattern, put, rejected

pytestmark = pytest.mark.gpu


def capi():
    from neuronika_amd import capi as c
    return c


def ints(seed, shape, lo=-3, hi=3):
    """small integers that depend on the flat index: every product and every f32 sum of them is exact"""
    n = int(np.prod(shape, dtype=np.int64))
    r = np.random.default_rng(seed).integers(lo, hi + 1, n)
    ramp = (np.arange(n, dtype=np.int64) * 2654435761 >> 9) % 3 - 1
    return np.clip(r + ramp, lo, hi).astype(np.float32).reshape(shape)


# ======================================================================================================================
# GEMM: sgemm_kernel<TA, TB, ALIGNED, TI, TJ, KG, EPX>
# ======================================================================================================================
LAYOUTS = {"nn": (0, 0), "nt": (0, 1), "tn": (1, 0), "tt": (1, 1)}
TILES = [(1, 1), (1, 2), (2, 1), (2, 2)]
# form -> (M, N, K, extra leading dimension, float offset of A): `aligned` needs M % 64 ti == 0, N % 64 tj == 0, K % 32 == 0, lda / ldb % 4 == 0
# and 16-byte aligned A / B; each of the other forms breaks one of those (ALIGNED = false)
FORMS = {"aligned": (128, 128, 96, 4, 0), "ragged": (130, 70, 45, 3, 0), "ragged_ld": (128, 128, 96, 3, 0), "offset": (128, 128, 96, 4, 1),
         "m_minus1": (127, 128, 96, 4, 0), "k_plus1": (128, 128, 97, 4, 0)}
GEMM_GRID = [(l, f, ti, tj) for l in LAYOUTS for f in FORMS for ti, tj in TILES]


def _operands(seed, ta, tb, M, N, K, pad):
    ar, ac = (K, M) if ta else (M, K)
    br, bc = (N, K) if tb else (K, N)
    a_full, b_full = pattern(seed, (ar, ac + pad), -1, 1), pattern(seed + 1, (br, bc + pad), -1, 1)
    a, b = a_full[:, :ac], b_full[:, :bc]
    return a_full, b_full, np.ascontiguousarray(a.T if ta else a), np.ascontiguousarray(b.T if tb else b)


@pytest.mark.parametrize("layout,form,ti,tj", GEMM_GRID, ids=[f"{l}-{f}-{ti}x{tj}" for l, f, ti, tj in GEMM_GRID])
def test_sgemm_forced_tiles(dev, layout, form, ti, tj):
    """nk_sgemm with the tile shape forced (NK_TUNE_GEMM_FORCE), unsplit: <TA, TB, form == aligned, TI, TJ, 1, EPX = NT>"""
    c = capi()
    ta, tb = LAYOUTS[layout]
    M, N, K, pad, off = FORMS[form]
    a_full, b_full, opa, opb = _operands(11, ta, tb, M, N, K, pad)
    c0 = pattern(13, (M, N + 5), -2, 2)
    prod = opa.astype(np.float64) @ opb.astype(np.float64)
    amax, bmax = float(np.abs(opa).max()), float(np.abs(opb).max())
    dev.gemm_force(f"{ti},{tj},1"); dev.gemm_kpair(0)
    try:
        A, B = put(dev, a_full, off), put(dev, b_full)
        outs = {}
        for name, alpha, beta, init in (("acc", -0.5, 1.0, c0), ("zero", 1.0, 1.0, 0.0), ("assign", 1.0, 0.0, np.nan)):
            w = Window(dev, (M, N + 5), init)
            c.sgemm(dev, ta, tb, M, N, K, alpha, A, a_full.shape[1], B, b_full.shape[1], beta, w.v, N + 5)
            outs[name] = w.read()
        tolerance.assert_contraction("mfma_paths:sgemm", outs["acc"][:, :N], -0.5 * prod + c0[:, :N].astype(np.float64), K, amax, bmax, scale=0.5, epilogue=True)
        tolerance.assert_contraction("mfma_paths:sgemm", outs["zero"][:, :N], prod, K, amax, bmax, epilogue=True)
        assert np.array_equal(outs["acc"][:, N:], c0[:, N:]), "the padding columns of C were written"
        assert np.array_equal(outs["assign"][:, :N], outs["zero"][:, :N]), "beta = 0 into NaN differs from beta = 1 into zeros"
        assert np.isnan(outs["assign"][:, N:]).all()
        if M % (64 * ti) == 0 and N % (64 * tj) == 0:   # whole tiles: one fma chain per output in the MFMA feeding order, whatever the loader
            from oracle.build_c import sgemm_device_order
            assert np.array_equal(outs["assign"][:, :N], sgemm_device_order(opa, opb, 0)), "not the device-order model's bits"
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None)


EPX_GRID = [(e, f, ti, tj, kg) for e in ("mask", "bias", "bias_relu") for f in ("aligned", "ragged", "k_plus1") for ti, tj in TILES
            for kg in (1, 2) if kg == 1 or (f == "aligned" and ti == tj)]


@pytest.mark.parametrize("epi,form,ti,tj,kg", EPX_GRID, ids=[f"{e}-{f}-{ti}x{tj}-kg{kg}" for e, f, ti, tj, kg in EPX_GRID])
def test_sgemm_epilogues_equal_the_separate_nodes(dev, epi, form, ti, tj, kg):
    """EPX = true: nk_linear_bwd_input_relu (NN, mask), nk_linear_fwd / nk_linear_relu_fwd (NT, bias / bias + ReLU) at every forced tile
    shape, aligned and guarded loaders, 256-thread and k-pair blocks - against float64 and, bit for bit, against the plain product
    followed by the separate node"""
    c = capi()
    n, m, o = FORMS[form][:3]                       # C is (n, .): M = n; the reduction is the third extent
    K = 512 if kg == 2 else o                       # k-pair blocks: an even number (>= 8) of whole k-tiles per block
    dev.gemm_force(f"{ti},{tj},1"); dev.gemm_kpair(2 if kg == 2 else 0)
    try:
        if epi == "mask":                           # dZ (n, m) (+)= (X > 0) * (G (n, K) . W (K, m))
            g, wt, x = pattern(21, (n, K), -1, 1), pattern(22, (K, m), -1, 1), pattern(23, (n, m), -1, 1)
            prod = g.astype(np.float64) @ wt.astype(np.float64)
            ref = np.where(x > 0, prod, 0.0)
            G, W, X = dev.array(g), dev.array(wt), dev.array(x)
            d0 = pattern(24, (n, m), -2, 2)
            acc, zero, first = Window(dev, (n, m), d0), Window(dev, (n, m), 0.0), Window(dev, (n, m), np.nan)
            c.linear_bwd_input_relu(dev, acc.v, G, W, X); c.linear_bwd_input_relu(dev, zero.v, G, W, X)
            c.linear_bwd_input_relu(dev, first.v, G, W, X, assign=True)
            got = first.read()
            assert np.array_equal(got, zero.read())
            tolerance.assert_contraction("mfma_paths:sgemm_mask", got, ref, K, float(np.abs(g).max()), float(np.abs(wt).max()), epilogue=True)
            tolerance.assert_contraction("mfma_paths:sgemm_mask", acc.read(), ref + d0, K, float(np.abs(g).max()), float(np.abs(wt).max()), epilogue=True)
            plain = Window(dev, (n, m), np.nan)     # the two nodes: MatMul, then ReLU's backward
            c.sgemm(dev, 0, 0, n, m, K, 1.0, G, K, W, m, 0.0, plain.v, m)
            assert np.array_equal(got, np.where(x > 0, plain.read(), np.float32(0)))
        else:                                       # Y (n, m) = X (n, K) . W (m, K)^T + b (, ReLU)
            x, wt, b = pattern(31, (n, K), -1, 1), pattern(32, (m, K), -1, 1), pattern(33, (m,), -1, 1)
            ref = x.astype(np.float64) @ wt.astype(np.float64).T + b
            X, W, Bv = dev.array(x), dev.array(wt), dev.array(b)
            y = Window(dev, (n, m), np.nan)
            (c.linear_relu_fwd if epi == "bias_relu" else c.linear_fwd)(dev, X, W, Bv, y.v)
            got = y.read()
            tolerance.assert_contraction("mfma_paths:sgemm_bias", got, np.maximum(ref, 0) if epi == "bias_relu" else ref, K,
                                         float(np.abs(x).max()), float(np.abs(wt).max()), epilogue=True)
            plain = Window(dev, (n, m), np.nan)
            c.sgemm(dev, 0, 1, n, m, K, 1.0, X, K, W, K, 0.0, plain.v, m)
            two = plain.read() + b
            assert np.array_equal(got, np.maximum(two, np.float32(0)) if epi == "bias_relu" else two)
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None)


PAIR_GRID = [(l, ti, tj) for l in ("nn", "nt", "tn") for ti, tj in ((1, 1), (2, 1), (2, 2))]


@pytest.mark.parametrize("first,ti,tj", PAIR_GRID, ids=[f"{l}-{ti}x{tj}" for l, ti, tj in PAIR_GRID])
def test_sgemm_pair_kernel(dev, first, ti, tj):
    """sgemm_pair_kernel<TA0, TB0, true, false, TI, TJ>: two aligned unsplit products with one forced tile shape in ONE launch
    (NK_TUNE_GEMM_PAIR = 1) equal two launches bit for bit, and float64 inside the bound; `+=` and first write"""
    c = capi()
    M, N, K = 128 * 2, 64 * tj * 2, 256
    probs = []
    for i, (ta, tb) in enumerate((LAYOUTS[first], (1, 0))):
        a_full, b_full, opa, opb = _operands(41 + 7 * i, ta, tb, M, N, K, 4)
        probs.append((ta, tb, a_full, b_full, opa, opb, pattern(45 + i, (M, N), -2, 2)))

    def run(pair, beta):
        dev.gemm_force(f"{ti},{tj},1"); dev.gemm_kpair(0); dev.gemm_pair(pair)
        try:
            ops = [(put(dev, p[2]), put(dev, p[3]), Window(dev, (M, N), p[6] if beta else np.nan)) for p in probs]
            (p0, (A0, B0, C0)), (p1, (A1, B1, C1)) = zip(probs, ops)
            c.sgemm_pair(dev, p0[0], p0[1], M, N, K, A0, p0[2].shape[1], B0, p0[3].shape[1], beta, C0.v, N,
                         p1[0], p1[1], M, N, K, A1, p1[2].shape[1], B1, p1[3].shape[1], beta, C1.v, N)
            return [C0.read(), C1.read()]
        finally:
            dev.gemm_force(None); dev.gemm_kpair(None); dev.gemm_pair(None)

    for beta in (0.0, 1.0):
        one, two = run(1, beta), run(0, beta)
        for p, x, y in zip(probs, one, two):
            assert np.array_equal(x, y), "one launch and two launches differ"
            ref = p[4].astype(np.float64) @ p[5].astype(np.float64) + beta * p[6]
            tolerance.assert_contraction("mfma_paths:sgemm_pair", x, ref, K, float(np.abs(p[4]).max()), float(np.abs(p[5]).max()), epilogue=True)


@pytest.mark.parametrize("layout", ["nn", "nt", "tn"])
def test_sgemm_tail_kernel(dev, layout):
    """sgemm_tail_kernel<TA, TB, EPX>: 17 x 17 tiles of 128 x 128 with 240 of the 512 resident-block slots declared busy - 272 whole
    tiles, the last 17 cut along K into 16 pieces each and summed by splitk_reduce_kernel; the tiles outside that rectangle keep
    the plain launch's bits, the rectangle stays inside the bound"""
    c = capi()
    ta, tb = LAYOUTS[layout]
    M = N = 17 * 128
    K = 48 * 32
    a_full, b_full, opa, opb = _operands(51, ta, tb, M, N, K, 0)
    A, B = dev.array(a_full), dev.array(b_full)
    c0 = pattern(53, (M, N), -2, 2)
    ref = opa.astype(np.float64) @ opb.astype(np.float64) + c0
    plain, shared = Window(dev, (M, N), c0), Window(dev, (M, N), c0)
    c.sgemm(dev, ta, tb, M, N, K, 1.0, A, a_full.shape[1], B, b_full.shape[1], 1.0, plain.v, N)
    dev.busy_slots(240)
    try:
        c.sgemm(dev, ta, tb, M, N, K, 1.0, A, a_full.shape[1], B, b_full.shape[1], 1.0, shared.v, N)
    finally:
        dev.busy_slots(0)
    p, s = plain.read(), shared.read()
    tolerance.assert_contraction("mfma_paths:sgemm_tail", s, ref, K, float(np.abs(opa).max()), float(np.abs(opb).max()), epilogue=True)
    same = p == s
    assert same[:16 * 128].all(), "a tile outside the last tile row changed"
    assert not same[16 * 128:].all(), "the shared-chip schedule was not taken: the last tile row has the plain launch's bits"


def test_sgemm_rejects_a_short_leading_dimension(dev):
    """a leading dimension below the row length is refused on the host, before any launch"""
    c = capi()
    z = dev.zeros((64, 64))
    rejected(c.sgemm, dev, 1, 0, 64, 64, 64, 1.0, z, 32, z, 64, 0.0, z, 64)


# ======================================================================================================================
# attention forward: attention_kernel<false, MASKED, FULL, OCC, KEEP, DH, RAGGED, CAUSAL>
# ======================================================================================================================
# S: below one 32-key tile, the tile and +- 1, whole tiles short of a 128-query block, the block and +- 1, two blocks
ATT_S = [1, 31, 32, 33, 96, 127, 128, 129, 256]
ATT_GRID = [(dh, S, p, causal) for dh in (32, 64, 128) for S in ATT_S for p in (0.0, 0.25) for causal in (False, True)]


@pytest.mark.parametrize("dh,S,p,causal", ATT_GRID, ids=[f"dh{dh}-S{S}-p{p}-{'causal' if cz else 'full'}" for dh, S, p, cz in ATT_GRID])
def test_attention_forward_forms(dev, dh, S, p, causal):
    """One geometry through every forward instantiation the dispatcher has for it: with kept state (KEEP, the register budget of
    OCC_F blocks per CU), without (inference: out only), and - full attention, DH < 128 - the two-block variant of
    NK_TUNE_ATTENTION_OCC = 2.  The kept form against the float64 oracle (out, scores, statistics, mask words against the row
    kernels' Philox draws); the other forms must give its output bit for bit."""
    c = capi()
    B, H, seed, offset = 2, 2, 0x5EED5EED, 77
    assert c.attention_supported(S, dh, p, True)
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    q, k, v = (pattern(s_, (B * S, H * dh), -1, 1) for s_ in (61, 62, 63))
    SP = c.attention_padded(S)
    masked = p != 0.0
    noise = (np.ascontiguousarray(O.dropout_noise(B * H * SP * SP, p, seed, offset).reshape(B * H, SP, SP)[:, :S, :S]) if masked
             else np.ones((B * H, S, S), np.float32))
    fwd = CO.attention_core_forward if causal else O.attention_core_forward
    ref, cache = fwd(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), H, B, p, noise.astype(np.float64))
    ref32, _ = fwd(q, k, v, H, B, p, noise)
    Q, K, V = dev.array(q), dev.array(k), dev.array(v)

    def run(keep, occ=None, packed=False):
        scores = dev.full((B * H, SP, SP), 7.0) if keep else None
        stats = dev.zeros((B * H, SP, 2)) if keep else None
        wbits = dev.zeros((B * H, SP, SP // 32)) if keep else None
        out = Window(dev, (B * S, H * dh), np.nan)
        dev.tune(c.TUNE_ATTENTION_OCC, occ)
        try:
            if packed:
                QKV = dev.array(np.concatenate([q, k, v], axis=1))
                c.attention_qkv_fwd(dev, QKV, scores, stats, wbits, out.v, B, S, H, dh, scale, p, True, seed, offset, causal=causal)
            else:
                c.attention_fwd(dev, Q, K, V, scores, stats, wbits, out.v, B, S, H, dh, scale, p, True, seed, offset, causal=causal)
        finally:
            dev.tune(c.TUNE_ATTENTION_OCC, None)
        return out.read(), scores, stats, wbits

    kept, scores, stats, wbits = run(True)
    floor = float(np.abs(v).max()) / (1 - p)
    err_gpu, err_cpu = np.abs(kept - ref).max(), np.abs(ref32 - ref).max()
    from conftest import record_margin
    record_margin("mfma_paths:attention_out", err_gpu, err_cpu, 1e-6 * floor)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * max(np.abs(ref).max(), floor)), (err_gpu, err_cpu)
    low = (np.arange(S)[None, :] <= np.arange(S)[:, None]) if causal else np.ones((S, S), bool)
    sc = scores.numpy()[:, :S, :S]
    err_s = np.abs(sc[:, low] - cache["scores"][:, low]).max()
    assert err_s <= tolerance.abs_term(dh, np.abs(q).max(), np.abs(k).max()), err_s
    inv = stats.numpy()[:, :S, 1].astype(np.float64)
    c1 = np.float64(np.float32(scale)) * np.log2(np.e)
    m2 = stats.numpy()[:, :S, 0].astype(np.float64)
    z = np.where(low, cache["scores"] * np.float64(np.float32(scale)), -np.inf)
    soft = np.exp(z - z.max(2, keepdims=True)); soft /= soft.sum(2, keepdims=True)
    np.testing.assert_allclose(np.where(low, np.exp2(cache["scores"] * c1 - m2[..., None]) * inv[..., None], 0.0), soft, rtol=2e-5, atol=1e-9)
    if masked:   # the mask words against the row kernels' draws (oracle/neuronika_oracle.py: the shared Philox layout)
        w = wbits.numpy().view(np.uint32).reshape(B * H, SP // 32, SP // 32, 32).transpose(0, 1, 3, 2).reshape(B * H, SP, SP // 32)
        unpacked = ((w[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B * H, SP, SP)[:, :S, :S]
        tile = ((np.arange(S)[None, :] // 32) <= (np.arange(S)[:, None] // 32)) if causal else low
        assert np.array_equal(unpacked[:, tile] != 0, noise[:, tile] != 0)
    lean = run(False)[0]
    assert np.array_equal(bits(lean), bits(kept)), "the forward without kept state computes another output"
    assert np.array_equal(bits(run(True, packed=True)[0]), bits(kept)), "the packed projection layout computes another output"
    if not causal and dh != 128:
        assert np.array_equal(bits(run(True, occ=2)[0]), bits(kept)), "the two-blocks-per-CU variant computes another output"
    assert np.array_equal(bits(run(False, occ=2)[0]), bits(kept))     # (the knob does not reach the inference form)


# backward: S below a block with a ragged tail, whole tiles short of a block, one block, a second block (causal: a main part and a tail)
ATT_BWD_GRID = [(dh, S, p, causal) for dh in (32, 64, 128) for S in (33, 96, 128, 160) for p in (0.0, 0.25) for causal in (False, True)]


@pytest.mark.parametrize("dh,S,p,causal", ATT_BWD_GRID, ids=[f"dh{dh}-S{S}-p{p}-{'causal' if cz else 'full'}" for dh, S, p, cz in ATT_BWD_GRID])
def test_attention_backward_forms(dev, dh, S, p, causal):
    """attention_kernel<true, ...> and the dK / dV products behind it: dQ, dK, dV, dS and the dropped probabilities against the float64
    oracle fed the same Philox mask; `+=` from a random start against the first write into NaN; causal: dS and Pd exactly 0 at every
    masked position of the blocks the kernel defines; the packed projection layout bit for bit"""
    c = capi()
    B, H, seed, offset = 2, 2, 0xABCDEF12345, 99
    d = H * dh
    scale = float(np.float32(1.0 / np.sqrt(dh)))
    q, k, v, g = (pattern(s_, (B * S, d), -1, 1) for s_ in (65, 66, 67, 68))
    SP = c.attention_padded(S)
    masked = p != 0.0
    noise = (np.ascontiguousarray(O.dropout_noise(B * H * SP * SP, p, seed, offset).reshape(B * H, SP, SP)[:, :S, :S]) if masked
             else np.ones((B * H, S, S), np.float32))
    fwd = CO.attention_core_forward if causal else O.attention_core_forward
    ref, ref32 = {}, {}
    for dt, dst in ((np.float64, ref), (np.float32, ref32)):
        _, cache = fwd(q.astype(dt), k.astype(dt), v.astype(dt), H, B, p, noise.astype(dt))
        dst.update(O.attention_core_backward(cache, g.astype(dt)), dropped=cache["dropped"])
    Q, K, V, G = (dev.array(t) for t in (q, k, v, g))
    scores, stats, out = dev.full((B * H, SP, SP), 7.0), dev.zeros((B * H, SP, 2)), dev.zeros((B * S, d))
    wbits = dev.zeros((B * H, SP, SP // 32))
    c.attention_fwd(dev, Q, K, V, scores, stats, wbits, out, B, S, H, dh, scale, p, True, seed, offset, causal=causal)
    starts = [pattern(s_, (B * S, d), -1, 1) for s_ in (75, 76, 77)]

    def backward(assign):
        dS, Pd = dev.full((B * H, SP, SP), 7.0), dev.full((B * H, SP, SP), 7.0)
        wins = [Window(dev, (B * S, d), np.nan if assign else s0) for s0 in starts]
        c.attention_bwd(dev, wins[0].v, wins[1].v, wins[2].v, dS, Pd, G, out, scores, stats, wbits, Q, K, V, B, S, H, dh, scale, p, True,
                        assign=(assign,) * 3, causal=causal)
        return [w.read() for w in wins], dS.numpy(), Pd.numpy()

    first, dS, Pd = backward(True)
    acc, _, _ = backward(False)
    low = (np.arange(S)[None, :] <= np.arange(S)[:, None]) if causal else np.ones((S, S), bool)
    from conftest import record_margin

    def check(what, got, want, want32, floor=0.0):
        sc = max(float(np.abs(want).max()), floor)
        err_gpu, err_cpu = float(np.abs(got - want).max()), float(np.abs(want32 - want).max())
        record_margin("mfma_paths:attention_" + what, err_gpu, err_cpu, 1e-6 * sc)
        assert err_gpu <= max(2 * err_cpu, 1e-6 * sc), (what, err_gpu, err_cpu, sc)

    # dS = P (dP - sum_k P dP): its rounding is that of dP = dO . V^T / (1 - p), a contraction over dh whose f32 chain the NumPy oracle
    # sums pairwise - the yardstick is dP's size, as for the one-key rows of tests/test_gpu_attention_causal.py
    dp = np.abs(np.einsum("bqhd,bkhd->bhqk", g.reshape(B, S, H, dh).astype(np.float64), v.reshape(B, S, H, dh).astype(np.float64))).max() / (1 - p)
    check("d_scores", dS[:, :S, :S][:, low], ref["d_scores"][:, low], ref32["d_scores"][:, low], float(dp))
    check("dropped", Pd[:, :S, :S][:, low], ref["dropped"][:, low], ref32["dropped"][:, low])
    assert np.array_equal(Pd[:, :S, :S][:, low] == 0, noise[:, low] == 0), "dropped probabilities and the mask disagree"
    if causal:   # defined - and exactly 0 at masked positions - on every 128 x 128 block that touches or lies below the diagonal
        r, kk = np.arange(SP)[:, None], np.arange(SP)[None, :]
        block = (kk // 128) <= (r // 128)
        for name, t in (("dS", dS), ("Pd", Pd)):
            assert not t[:, block & ~(kk <= r)].any(), name + " is not zero above the diagonal"
            assert np.all(t[:, ~block] == 7.0), name + " was written in a block the kernel does not define"
    elif S % 32:
        assert not dS[:, :S, S:].any() and not Pd[:, :S, S:].any(), "padded keys carry a gradient"
    floors = (np.abs(ref["d_scores"]).sum(2).max() * np.abs(k).max(), np.abs(ref["d_scores"]).sum(1).max() * np.abs(q).max(),
              np.abs(ref["dropped"]).sum(1).max() * np.abs(g).max())
    for name, got, a, s0, floor in zip(("dq", "dk", "dv"), first, acc, starts, floors):
        assert np.isfinite(got).all(), name
        check(name, got, ref[name], ref32[name], float(floor))
        assert np.array_equal(a, (s0 + got).astype(np.float32)) or np.abs(a - (s0 + got)).max() <= 1e-6 * max(1.0, float(floor)), name + ": `+=` is not old + first write"
    QKV = dev.array(np.concatenate([q, k, v], axis=1))
    sc2, st2, out2, wb2 = dev.full((B * H, SP, SP), 7.0), dev.zeros((B * H, SP, 2)), dev.zeros((B * S, d)), dev.zeros((B * H, SP, SP // 32))
    c.attention_qkv_fwd(dev, QKV, sc2, st2, wb2, out2, B, S, H, dh, scale, p, True, seed, offset, causal=causal)
    dQKV, dS2, Pd2 = Window(dev, (B * S, 3 * d), np.nan), dev.full((B * H, SP, SP), 7.0), dev.full((B * H, SP, SP), 7.0)
    c.attention_qkv_bwd(dev, dQKV.v, dS2, Pd2, G, out2, sc2, st2, wb2, QKV, B, S, H, dh, scale, p, True, assign=True, causal=causal)
    packed = dQKV.read()
    for i, (name, got) in enumerate(zip(("dq", "dk", "dv"), first)):
        assert np.array_equal(bits(packed[:, i * d:(i + 1) * d]), bits(got)), name + ": the packed layout computes other bits"
    assert np.array_equal(bits(dS2.numpy()), bits(dS)) and np.array_equal(bits(Pd2.numpy()), bits(Pd))


def test_attention_eval_ignores_p(dev):
    """evaluation with p > 0 is the unmasked instantiation: bit for bit the p = 0 output, no mask words needed"""
    c = capi()
    B, S, H, dh = 1, 100, 2, 64
    scale = float(np.float32(0.125))
    q, k, v = (dev.array(pattern(s_, (B * S, H * dh), -1, 1)) for s_ in (71, 72, 73))
    a, b = Window(dev, (B * S, H * dh), np.nan), Window(dev, (B * S, H * dh), np.nan)
    c.attention_fwd(dev, q, k, v, None, None, None, a.v, B, S, H, dh, scale, 0.4, False, 1, 2)
    c.attention_fwd(dev, q, k, v, None, None, None, b.v, B, S, H, dh, scale, 0.0, True, 1, 2)
    assert np.array_equal(bits(a.read()), bits(b.read()))
    assert not c.attention_supported(S, 48, 0.0) and not c.attention_supported(S, 64, 1.0, True)


# ======================================================================================================================
# convolution
# ======================================================================================================================
def _conv_ref(x, w, stride, dil, groups, go=None):
    """float64 oracle: y, and with `go` the two gradients"""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    y = np.zeros(O.conv_out_shape(x.shape, w.shape, stride, dil)); O.convolution_forward(x64, w64, y, stride, dil, groups)
    if go is None:
        return y
    dx, dw = np.zeros(x.shape), np.zeros(w.shape)
    O.convolution_backward_input(dx, go.astype(np.float64), w64, stride, dil, groups)
    O.convolution_backward_kernel(dw, go.astype(np.float64), x64, stride, dil, groups)
    return y, dx, dw


# id -> (x shape, w shape, stride, dilation, groups): the forward instantiation is read off Cg = w[1], Mg = w[0] / groups, the last
# stride and the last output extent; 2 x 2 taps keep Winograd and the stride-2 tap-plane kernels out of the way
CONV_FWD = {
    "fast_m96_s2_w4": ((2, 32, 8, 8), (96, 32, 2, 2), (2, 2), (1, 1), 1),      # conv_fwd_fast_kernel<false, 2, false, 2>
    "fast_m96_s1_w5": ((2, 32, 6, 6), (96, 32, 2, 2), (1, 1), (1, 1), 1),      # <false, 2, true, 1>: out width % 4 != 0 (RP)
    "fast_m96_s2_w5": ((2, 32, 10, 10), (96, 32, 2, 2), (2, 2), (1, 1), 1),    # <false, 2, true, 2>
    "fast_m64_s2_w4": ((2, 32, 8, 8), (64, 32, 2, 2), (2, 2), (1, 1), 1),      # <true, 1, false, 2>
    "fast_m64_s2_w4_g2": ((2, 64, 8, 8), (128, 32, 2, 2), (2, 2), (1, 1), 2),  # ... two groups in grid.z
    "generic_m64_k32_w4": ((2, 8, 5, 5), (64, 8, 2, 2), (1, 1), (1, 1), 1),    # conv_fwd_kernel<true, 1, true>: Cg * taps == 32, quads in a row
    "generic_m128_k32_w4": ((2, 8, 5, 5), (128, 8, 2, 2), (1, 1), (1, 1), 1),  # conv_fwd_kernel<true, 2, true>
    "generic_m128_k32_w4_3d": ((1, 8, 3, 5, 5), (128, 8, 1, 2, 2), (1, 1, 1), (1, 1, 1), 1),   # ... in three dimensions
    "direct_5x5_w5": ((2, 6, 9, 9), (6, 3, 5, 5), (1, 1), (1, 1), 2),          # conv_direct_fwd_kernel<1, 5, 5>: L < 512, width % 4 != 0
    "direct_5x5_dil2": ((2, 4, 12, 12), (4, 4, 5, 5), (1, 1), (2, 2), 1),      # ... dilated (the rows kernel needs dilation 1)
}


@pytest.mark.parametrize("case", list(CONV_FWD), ids=list(CONV_FWD))
def test_conv_forward_paths(dev, case):
    c = capi()
    xs, ws, stride, dil, groups = CONV_FWD[case]
    K = ws[1] * int(np.prod(ws[2:]))
    bshape = (ws[0],) + (1,) * (len(xs) - 2)
    for kind in ("float", "int"):
        gen = pattern if kind == "float" else ints
        x, w, b = gen(81, xs), gen(82, ws), gen(83, bshape)
        ref = _conv_ref(x, w, stride, dil, groups)
        X, W = dev.array(x), dev.array(w)
        y, yb = Window(dev, ref.shape, np.nan), Window(dev, ref.shape, np.nan)
        c.conv_fwd(dev, X, W, y.v, stride, dil, groups)
        c.conv_fwd(dev, X, W, yb.v, stride, dil, groups, bias=dev.array(b))
        got, gotb = y.read(), yb.read()
        if kind == "int":
            assert np.array_equal(got, ref) and np.array_equal(gotb, ref + b), "integer data: every sum is exact"
        else:
            tolerance.assert_contraction("mfma_paths:conv_fwd", got, ref, K, float(np.abs(x).max()), float(np.abs(w).max()))
            assert np.array_equal(gotb, (got + b).astype(np.float32))


# the kernel gradient: conv_bwd_kernel_kernel<VEC_G, 2, 1, QUADR, SW> - Mg = 128 (TI 2), Cg * taps = 32 <= 64 (TJ 1)
CONV_BWDK = {
    "quad_s1": ((2, 8, 6, 6), (128, 8, 2, 2), (1, 1)),        # <true, 2, 1, true, 1>: last stride 1, out width 5 >= 4
    "quad_s2": ((2, 8, 10, 10), (128, 8, 2, 2), (2, 2)),      # <true, 2, 1, true, 2>
    "vec_s3_L12": ((2, 8, 5, 8), (128, 8, 2, 2), (1, 3)),     # <true, 2, 1, false, 1>: last stride 3 (no quads), L = 12
    "scalar_s3_L9": ((2, 8, 4, 8), (128, 8, 2, 2), (1, 3)),   # <false, 2, 1, false, 1>: L = 9
}


@pytest.mark.parametrize("case", list(CONV_BWDK), ids=list(CONV_BWDK))
def test_conv_kernel_gradient_paths(dev, case):
    c = capi()
    xs, ws, stride = CONV_BWDK[case]
    dil = (1, 1)
    for kind in ("float", "int"):
        gen = pattern if kind == "float" else ints
        x, w = gen(91, xs), gen(92, ws)
        oshape = O.conv_out_shape(xs, ws, stride, dil)
        go = gen(93, oshape)
        _, _, dw_ref = _conv_ref(x, w, stride, dil, 1, go)
        db_ref = go.astype(np.float64).sum(axis=(0, 2, 3)).reshape(ws[0], 1, 1)
        R = xs[0] * int(np.prod(oshape[2:]))
        X, G = dev.array(x), dev.array(go)
        d0 = gen(94, ws)
        acc, first = Window(dev, ws, d0), Window(dev, ws, np.nan)
        c.conv_bwd_kernel(dev, acc.v, G, X, stride, dil)
        c.conv_bwd_kernel(dev, first.v, G, X, stride, dil, assign=True)
        fb, db = Window(dev, ws, np.nan), Window(dev, (ws[0], 1, 1), np.nan)
        c.conv_bwd_kernel_bias(dev, fb.v, db.v, G, X, stride, dil, assign=(True, True))
        got = first.read()
        assert np.array_equal(acc.read(), (d0 + got).astype(np.float32)), "`+=` is not old + first write"
        assert np.array_equal(bits(fb.read()), bits(got)), "the fused bias gradient changed dW"
        if kind == "int":
            assert np.array_equal(got, dw_ref) and np.array_equal(db.read(), db_ref), "integer data: every sum is exact"
        else:
            tolerance.assert_contraction("mfma_paths:conv_bwd_kernel", got, dw_ref, R, float(np.abs(go).max()), float(np.abs(x).max()))
            tolerance.assert_contraction("mfma_paths:conv_bwd_bias", db.read(), db_ref, R, float(np.abs(go).max()), 1.0)


def test_conv_input_gradient_fast_ragged_128(dev):
    """conv_bwd_input_fast_kernel<false, 2>: 96 input channels per group (one 128-row tile, 32 rows of padding), 32 output channels;
    on integer data equal to the oracle and to the generic kernel, which a 33rd output channel with zero weights selects"""
    c = capi()
    xs, ws, stride, dil = (2, 96, 9, 9), (32, 96, 2, 2), (1, 1), (1, 1)
    for kind in ("float", "int"):
        gen = pattern if kind == "float" else ints
        x, w = gen(101, xs), gen(102, ws)
        go = gen(103, O.conv_out_shape(xs, ws, stride, dil))
        _, dx_ref, _ = _conv_ref(x, w, stride, dil, 1, go)
        G, W = dev.array(go), dev.array(w)
        d0 = gen(104, xs)
        acc, first = Window(dev, xs, d0), Window(dev, xs, np.nan)
        c.conv_bwd_input(dev, acc.v, G, W, stride, dil)
        c.conv_bwd_input(dev, first.v, G, W, stride, dil, assign=True)
        got = first.read()
        assert np.array_equal(acc.read(), (d0 + got).astype(np.float32))
        if kind == "int":
            assert np.array_equal(got, dx_ref)
            w33 = np.concatenate([w, np.zeros((1,) + ws[1:], np.float32)])
            go33 = np.concatenate([go, ints(105, (xs[0], 1) + go.shape[2:])], axis=1)
            other = Window(dev, xs, np.nan)
            c.conv_bwd_input(dev, other.v, dev.array(go33), dev.array(w33), stride, dil, assign=True)
            assert np.array_equal(other.read(), got), "fast and generic input gradients differ on integer data"
        else:
            tolerance.assert_contraction("mfma_paths:conv_bwd_input", got, dx_ref, ws[0] * 4, float(np.abs(go).max()), float(np.abs(w).max()))


@pytest.mark.parametrize("pad", [0, 1])
def test_conv_s2dx_wide_blocks(dev, pad):
    """s2dx_kernel<4, 32, PAD>: the fused-phase 3 x 3 stride-2 input gradient with wide blocks (NK_TUNE_CONV_S2DX = 3: 128 input
    channels per block) against the oracle, and exactly - integer data - against the per-phase kernels (knob 0) and the narrow blocks"""
    c = capi()
    xs, ws, stride, dil = (2, 128, 8, 8), (32, 128, 3, 3), (2, 2), (1, 1)
    ps = tuple(xs[:2]) + tuple(e + 2 * pad for e in xs[2:])
    oshape = O.conv_out_shape(ps, ws, stride, dil)
    sl = (slice(None), slice(None)) + (slice(pad, pad + 8),) * 2
    padding = (pad, pad) if pad else None
    for kind in ("float", "int"):
        gen = pattern if kind == "float" else ints
        w, go = gen(111, ws), gen(112, oshape)
        dxp = np.zeros(ps)
        O.convolution_backward_input(dxp, go.astype(np.float64), w.astype(np.float64), stride, dil, 1)
        ref = dxp[sl]
        G, W = dev.array(go), dev.array(w)
        outs = {}
        for knob in (3, 2, 0):
            dev.conv_s2dx(knob)
            try:
                d0 = gen(113, xs)
                acc, first = Window(dev, xs, d0), Window(dev, xs, np.nan)
                c.conv_bwd_input(dev, acc.v, G, W, stride, dil, padding=padding)
                c.conv_bwd_input(dev, first.v, G, W, stride, dil, assign=True, padding=padding)
            finally:
                dev.conv_s2dx(None)
            outs[knob] = first.read()
            assert np.array_equal(acc.read(), (d0 + outs[knob]).astype(np.float32)), knob
        if kind == "int":
            assert np.array_equal(outs[3], ref) and np.array_equal(outs[2], ref) and np.array_equal(outs[0], ref)
        else:
            tolerance.assert_contraction("mfma_paths:conv_s2dx", outs[3], ref, ws[0] * 9, float(np.abs(go).max()), float(np.abs(w).max()))
