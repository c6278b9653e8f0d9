"""Reductions over 32768 rows - the weight and bias gradients of the benchmark's attention workload (C5: B * S = 32 * 1024 rows) -
checked without a GPU: which plan `gemm_plan` (nk_gemm.hip) takes BY RULE at K = 32768, that the stated plan satisfies the parity
policy of tests/tolerance.py, and that the asserts tests/test_gpu_long_reductions.py applies to the device have teeth.

The plan at this length is "split K, no split longer than 128 k-tiles": a slab is ONE f32 chain of up to 4096 products (chained
launches, the other route past one chain, stop at GEMM_CHAIN_K = 2048).  The device's value of one output is restated by
`slab_model`: `oracle.build_c.sgemm_device_order` per slab, the slabs added in split order from 0 in f32 (the second pass).

Measured with that model (worst err / (1e-6 K |a| |b|) against f64 over 16 rows x 64 columns, K = 32768; NumPy's f32 product of
the same operands: one_signed 0.100, signed 0.0024):
  8 chains of 4096     one_signed 0.241   signed 0.0093
  16 chains of 2048    one_signed 0.132   signed 0.0049
  32 chains of 1024    one_signed 0.110   signed 0.0039
  128 chains of 256    one_signed 0.121   signed 0.0025
  the flaws below, x the bound, (one_signed, signed): a slab dropped or added twice (32312, 2428), a split boundary one k-tile
  early / late (361 / 346, 188 / 191), one product missing at a seam (28.7, 27.9); none leaves the integers exact
This file also holds what the GPU file shares with it: the cases, their operands, the sampled rows and the model."""
import functools

import numpy as np
import pytest

BK = 32            # a k-tile (nk_gemm.hip)
K_LONG = 32768     # B * S of the benchmark's attention workload
KINDS = ("signed", "one_signed", "int")

# id -> (layouts, M, N, K, the plan the rule takes: (ti, tj, splits, k-tiles per split))
CASES = {
    "c5_dw":         (("tn",), 1024, 1024, 32768, (2, 2, 8, 128)),        # 64 tiles of 128 x 128, s = 8, the cap of 8 not engaged
    "c5_dw_packed":  (("tn",), 3072, 1024, 32768, (2, 2, 8, 128)),        # 192 tiles, s = 3 raised to 8 by the cap
    "c5_dw_ragged":  (("tn",), 1000, 1000, 32700, (2, 2, 8, 128)),        # guarded loader, last split 126 k-tiles, the last one of 28
    "small_64tiles": (("tn", "nn", "nt"), 256, 256, 32768, (1, 1, 32, 32)),  # 128 x 128 cannot reach 384 blocks: 64 x 64 tiles
    "one_tile":      (("tn",), 64, 64, 32768, (1, 1, 128, 8)),
}


def rule_plan(M, N, K):
    """What `gemm_plan` (nk_gemm.hip) decides for an unforced, unbatched launch, restated:
    (ti, tj, splits, k-tiles per split); tiles are 64 ti x 64 tj."""
    kt = -(-K // BK)
    blocks = lambda ti, tj: -(-M // (64 * ti)) * -(-N // (64 * tj))                     # noqa: E731
    ti = 1 if M <= 64 or (M % 128 != 0 and M % 64 == 0) else 2
    tj = 1 if N <= 64 or (N % 128 != 0 and N % 64 == 0) else 2
    splits, nb = 1, blocks(ti, tj)
    if nb >= 512:                                # plenty of blocks: unsplit; the last wave of resident slots against MFMA density
        eff = lambda n, slots: n / (-(-n // slots) * slots)                             # noqa: E731
        t0 = ti * tj
        best = {4: 1.0, 2: 0.9, 1: 0.8}[t0] * eff(nb, 512 if t0 == 4 else 768)
        if t0 == 4:
            for cand in ((1, 2), (2, 1)):
                c = 0.9 * eff(blocks(*cand), 768)
                if c > best + 0.05:
                    best, (ti, tj) = c, cand
        if t0 >= 2:
            n1 = blocks(1, 1)
            q = eff(n1, 768)
            if 0.8 * (0.9 if n1 >= 1536 and q < 0.9 else q) > best + 0.05:
                ti = tj = 1
    else:
        s = min(-(-512 // nb), kt // 16)
        if ti * tj == 4 and nb >= 256 and kt >= 48:      # one 128 x 128 block per CU and a long reduction: unsplit
            splits = 1
        elif ti * tj > 1 and s >= 1 and nb * s >= 384:
            splits = s
        else:
            ti = tj = 1
            if blocks(1, 1) < 256:
                splits = max(1, min(512 // blocks(1, 1), kt // 8))
    if 1 < splits < (kt + 127) // 128:           # the cap: split anyway -> no split takes more than 128 k-tiles
        splits = (kt + 127) // 128
    kts = max(1, -(-kt // splits))
    return ti, tj, max(1, -(-kt // kts)), kts


def twin(case):
    """the forced configuration (`dev.gemm_force`, with `dev.gemm_kpair(0)`) that must give the rule's bits"""
    _, M, N, K, _ = CASES[case]
    ti, tj, splits, _ = rule_plan(M, N, K)
    return "%d,%d,%d" % (ti, tj, splits)


# ---- operands: generated once, shared, read-only ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def operand(kind, seed, shape):
    """signed U[-1, 1); one_signed U[0, 1) (the drift that cut the chains at 2048); int: integers in [-3, 3], every sum of
    32768 products is at most 9 * 32768 < 2^24 in magnitude and so exact in f32 in any order"""
    rng = np.random.default_rng(seed)
    if kind == "int":
        t = rng.integers(-3, 4, shape, dtype=np.int8).astype(np.float32)
    else:
        t = rng.random(shape, dtype=np.float32)
        if kind == "signed":
            t *= np.float32(2.0)
            t -= np.float32(1.0)
    assert kind in KINDS and t.dtype == np.float32
    t.setflags(write=False)
    return t


SEEDS = {"c5_dw": (11, 12), "c5_dw_packed": (13, 12), "c5_dw_ragged": (14, 15), "small_64tiles": (16, 17), "one_tile": (18, 19)}


def stored_tn(case, kind):
    """(a, b) as LinearBwd passes them to the TN product: a = the gradient (K, M), b = the layer input (K, N); lda = M, ldb = N.
    (c5_dw_packed shares c5_dw's input: the packed projection reads the same activations.)"""
    _, M, N, K, _ = CASES[case]
    sa, sb = SEEDS[case]
    return operand(kind, sa, (K, M)), operand(kind, sb, (K, N))


def sample_rows(M, seed=0, n_random=24):
    """first and last row, both sides of the 128-row seams nearest 0, M / 2 and M, and ~24 seeded random rows"""
    rows = {0, M - 1}
    for seam in (128, int(round(M / 2 / 128)) * 128, (M - 1) // 128 * 128):
        if 0 < seam < M:
            rows |= {seam - 1, seam}
    rows |= set(int(r) for r in np.random.default_rng(1000 + seed + M).integers(0, M, n_random))
    return np.array(sorted(rows))


# ---- the model of one launch -----------------------------------------------------------------------------------------------
FLAWS = ("slab_dropped", "slab_twice", "boundary_early", "boundary_late", "seam_product")


def slab_model(opa, opb, splits, kts, kc=0, flaw=None):
    """opa (rows, K) . opb (K, N) as a split-K launch computes it: slab s = one device-order chain over
    [s kts 32, min(K, (s + 1) kts 32)), then s = 0; s += slab in split order (f32) - the composition of
    test_gpu_parity.py::test_sgemm_is_the_device_order_model_bit_for_bit.  `flaw`: a bookkeeping bug, by name."""
    from oracle.build_c import sgemm_device_order
    assert flaw is None or (flaw in FLAWS and splits >= 4)
    K = opa.shape[1]
    hit = splits // 2                                        # the slab a flaw touches
    want = np.zeros((opa.shape[0], opb.shape[1]), np.float32)
    for s in range(splits):
        k0, k1 = s * kts * BK, min(K, (s + 1) * kts * BK)
        if s == hit:
            if flaw == "slab_dropped":
                continue
            if flaw == "boundary_early":                     # ends one k-tile early: 32 products missing
                k1 -= BK
            if flaw == "boundary_late":                      # ends one k-tile late: 32 products doubled
                k1 += BK
            if flaw == "seam_product":                       # starts one product late
                k0 += 1
        slab = sgemm_device_order(opa[:, k0:k1], opb[k0:k1], kc)
        want = want + slab
        if s == hit and flaw == "slab_twice":
            want = want + slab
    return want


@functools.lru_cache(maxsize=None)
def small(kind):
    """16 rows x 64 columns of a K = 32768 product: operands, f64 and NumPy-f32 products"""
    a, b = operand(kind, 31, (16, K_LONG)), operand(kind, 32, (K_LONG, 64))
    ref64 = a.astype(np.float64) @ b.astype(np.float64)
    cpu32 = a @ b
    for t in (ref64, cpu32):
        t.setflags(write=False)
    return a, b, ref64, cpu32, float(np.abs(a).max()), float(np.abs(b).max())


PLANS = [(8, 128), (32, 32), (128, 8)]           # (splits, k-tiles per split) of the table's three plans at K = 32768


def test_the_table_is_what_the_rule_decides():
    for case, (_, M, N, K, plan) in CASES.items():
        assert rule_plan(M, N, K) == plan, (case, rule_plan(M, N, K))
        ti, tj, splits, kts = plan
        # the twin runs with k-pair blocks off; so does the rule here: more blocks than CUs (256), or too few k-tiles per block
        nblk = -(-M // (64 * ti)) * -(-N // (64 * tj)) * splits
        assert nblk > 256 or kts < (32 if ti * tj == 4 else 16), case
        assert splits * kts * BK >= K > (splits - 1) * kts * BK, case     # every split has work, together they cover K
        assert kts * BK <= 4096, case                                     # a slab is one chain of at most 4096 products
    assert {twin(c) for c in ("c5_dw", "c5_dw_packed", "c5_dw_ragged")} == {"2,2,8"}
    assert twin("small_64tiles") == "1,1,32" and twin("one_tile") == "1,1,128"
    assert sorted({(p[2], p[3]) for *_, p in CASES.values()}) == sorted(PLANS)
    # the branches around the table: without the cap the packed gradient would run as 3 splits of 342 k-tiles (chains of 10944);
    # the benchmark's other weight gradients (K = 4096 at B = 4: 2 splits of 64 k-tiles; C4: unsplit, chained launches)
    assert -(-512 // (24 * 8)) == 3 and -(-1024 // 3) * BK == 10944
    assert rule_plan(1024, 1024, 4096) == (2, 2, 8, 16) and rule_plan(1024, 1024, 8192) == (2, 2, 8, 32)
    assert rule_plan(4096, 4096, 4096) == (2, 2, 1, 128) and rule_plan(2048, 2048, 32768) == (2, 2, 1, 1024)
    assert rule_plan(1024, 1024, 65536) == (2, 2, 16, 128)                # the cap engaged on the square shape too


@pytest.mark.parametrize("kind", ["one_signed", "signed"])
@pytest.mark.parametrize("splits,kts", PLANS)
def test_the_stated_plan_satisfies_the_policy(kind, splits, kts):
    """Half the absolute term of the policy: the device adds the roundings of the second pass and of the epilogue that this
    model of one output carries only in part.  Measured: 0.241 of the bound for 8 chains of 4096 on one_signed data, the worst
    of the six (module docstring)."""
    from tolerance import abs_term
    a, b, ref64, _, amax, bmax = small(kind)
    got = slab_model(a, b, splits, kts)
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    assert err <= 0.5 * abs_term(K_LONG, amax, bmax), (err, abs_term(K_LONG, amax, bmax))


def test_chains_of_2048_are_other_bits():
    a, b, *_ = small("one_signed")
    assert not np.array_equal(slab_model(a, b, 8, 128), slab_model(a, b, 8, 128, kc=2048))
    assert not np.array_equal(slab_model(a, b, 8, 128), slab_model(a, b, 16, 64))


def test_integers_are_exact_in_the_model():
    a, b, ref64, cpu32, _, _ = small("int")
    assert np.abs(ref64).max() < 2 ** 24 and np.array_equal(cpu32, ref64)
    for splits, kts in PLANS:
        assert np.array_equal(slab_model(a, b, splits, kts), ref64)


@pytest.mark.parametrize("flaw", FLAWS)
def test_a_bookkeeping_flaw_is_caught(flaw):
    """Each flaw breaks integer exactness and leaves the bound `assert_contraction` applies, on both float kinds."""
    from tolerance import assert_contraction
    a, b, ref64, _, _, _ = small("int")
    assert not np.array_equal(slab_model(a, b, 8, 128, flaw=flaw), ref64)
    for kind in ("one_signed", "signed"):
        a, b, ref64, cpu32, amax, bmax = small(kind)
        assert_contraction(None, slab_model(a, b, 8, 128), ref64, K_LONG, amax, bmax, cpu32=cpu32)
        with pytest.raises(AssertionError):
            assert_contraction(None, slab_model(a, b, 8, 128, flaw=flaw), ref64, K_LONG, amax, bmax, cpu32=cpu32)


def test_sampled_rows_cover_the_seams():
    assert {0, 127, 128, 511, 512, 895, 896, 1023} <= set(sample_rows(1024))
    assert {0, 127, 128, 1535, 1536, 2943, 2944, 3071} <= set(sample_rows(3072))
    assert {0, 127, 128, 511, 512, 895, 896, 999} <= set(sample_rows(1000))
    assert {0, 127, 128, 255} <= set(sample_rows(256)) and {0, 63} <= set(sample_rows(64))
    for M in (64, 256, 1000, 1024, 3072):
        r = sample_rows(M)
        assert r.min() >= 0 and r.max() < M and len(set(r)) == len(r) and len(r) <= 32
