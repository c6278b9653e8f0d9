"""GPU parity of the paged key / value cache through the C ABI: nk_kv_pages_append, nk_kv_pages_copy and
nk_attention_decode_paged_fwd against the NumPy model of tests/paged_oracle.py and against the CONTIGUOUS entry points.

Pass condition of the decode tests (include/neuronika_hip.h, "paged decoding", bit contract (1)): `np.array_equal` with
nk_attention_decode_gqa_fwd (window 0) or nk_attention_decode_window_fwd with ring = 0 run on the (B, Hkv, cap_v, dh) cache gathered
through the table - the paged kernels are the contiguous bodies with one more switch, so nothing but equality is accepted.  For one
page size per head size the result is also held against tests/decode_oracle.py on the gathered cache with the suite's own rule,
err_gpu <= max(2 * err_cpu32, 1e-6 * scale), margins recorded under `attention_decode_paged:*`.

Every decode setup is hostile: pages nobody owns, the unwritten slots of owned pages and (windowed) the positions below the window
hold NaN, table entries past a sequence's own pages alternate between -1 and num_pages + 5, and the table rows are a random
permutation of the pool."""
import numpy as np
import pytest

import decode_oracle as DO
import paged_oracle as PO

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
DHS = [32, 64, 128, 20, 5]
GEOMETRIES = [(1, 1), (3, 3), (4, 2), (4, 1), (12, 1)]                    # (H, Hkv); (12, 1): two blocks of one group
B = 3


def capi():
    from neuronika_amd import capi as c
    return c


def rnd(seed, shape, lo, hi):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(hi - lo) + np.float32(lo), dtype=np.float32)


def _scale(dh):
    return float(np.float32(1.0 / np.sqrt(dh)))


def _pages(dh):
    ch = capi().attention_decode_chunk(dh)
    return [16, 64, ch, 2 * ch]


def _lengths(dh, page):
    """what the FIRST new row of a sample reads up to"""
    ch = capi().attention_decode_chunk(dh)
    return sorted({n for n in (1, page - 1, page, page + 1, ch - 1, ch, ch + 1, 2 * ch + 1, 3 * ch + 7) if n >= 1})


def _windows(dh, page):
    ch = capi().attention_decode_chunk(dh)
    return [1, page, ch - 1, ch + 1, 2 * ch + 3]


def _setup(seed, start, T, Hkv, dh, page, garbage=np.nan, bad=(-1, None), lo=None):
    """-> (Kp, Vp, table, num_pages): pools holding random keys / values at positions [lo[b], start[b] + T) of sample b and `garbage`
    everywhere else, behind table rows that are a random permutation of the pool; entries past a sample's own pages alternate
    between the two values of `bad` (None: num_pages + 5)."""
    rng = np.random.default_rng(seed)
    ends = [int(s) + T for s in start]
    max_pages = max((e + page - 1) // page for e in ends) + 2
    num_pages = len(start) * max_pages + 3
    perm = rng.permutation(num_pages)
    table = np.empty((len(start), max_pages), np.int32)
    cap = max_pages * page
    kc, vc = rnd(seed + 1, (len(start), Hkv, cap, dh), -1, 1), rnd(seed + 2, (len(start), Hkv, cap, dh), -1, 1)
    Kp, Vp = (np.full((num_pages, Hkv, page, dh), garbage, np.float32) for _ in range(2))
    at = 0
    for b, e in enumerate(ends):
        own = (e + page - 1) // page
        table[b, :own] = perm[at:at + own]
        at += own
        for i in range(own, max_pages):
            v = bad[(i + b) % 2]
            table[b, i] = num_pages + 5 if v is None else v
        first = 0 if lo is None else int(lo[b])
        for pos in range(first, e):                                      # per position: unwritten slots of owned pages keep the garbage
            Kp[table[b, pos // page], :, pos % page] = kc[b, :, pos]
            Vp[table[b, pos // page], :, pos % page] = vc[b, :, pos]
    return Kp, Vp, table, num_pages


def _paged(dev, Q, ldq, KP, VP, S, TAB, max_pages, T, H, Hkv, dh, page, num_pages, W):
    c = capi()
    out = dev.full((B * T, H * dh), np.nan)
    ws = dev.full((c.attention_decode_paged_workspace(B, T, H, dh, max_pages, page, W),), np.nan)
    c.attention_decode_paged_fwd(dev, Q, ldq, KP, VP, S, TAB, max_pages, out, ws, B, T, H, Hkv, dh, page, num_pages, W, _scale(dh))
    return out.numpy()


def _twin(dev, Q, ldq, KC, VC, S, cap, T, H, Hkv, dh, W):
    c = capi()
    out = dev.full((B * T, H * dh), np.nan)
    if W == 0:
        ws = dev.full((c.attention_decode_workspace(B, T, H, dh, cap),), np.nan)
        c.attention_decode_gqa_fwd(dev, Q, ldq, KC, VC, S, out, ws, B, T, H, Hkv, dh, cap, _scale(dh))
    else:
        ws = dev.full((c.attention_decode_window_workspace(B, T, H, dh, W),), np.nan)
        c.attention_decode_window_fwd(dev, Q, ldq, KC, VC, S, out, ws, B, T, H, Hkv, dh, cap, W, 0, _scale(dh))
    return out.numpy()


def _check(got, want64, want32, vmax, what):
    scale = max(np.abs(want64).max(), vmax)
    err_gpu, err_cpu = np.abs(got - want64).max(), np.abs(want32 - want64).max()
    from conftest import record_margin
    record_margin("attention_decode_paged:" + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


# ---- decode: the bits of the contiguous entry points ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pi", range(4))
@pytest.mark.parametrize("dh", DHS)
def test_paged_decode_equals_the_contiguous_kernels_bit_for_bit(dev, dh, pi):
    """page = (16, 64, C, 2C)[pi]; T in {1, 4}; every geometry; every length of `_lengths` as what the first new row of some sample
    reads, ragged across the three samples of a call; window 0 and every window of `_windows`.  The first page size of every head
    size is also held against the f64 / f32 oracle."""
    page = _pages(dh)[pi]
    ns = _lengths(dh, page)
    ns = ns + ns[:(-len(ns)) % B]
    seed = 1000 * dh + 10 * pi
    for T in (1, 4):
        for H, Hkv in GEOMETRIES:
            for g0 in range(0, len(ns), B):
                group = ns[g0:g0 + B]
                start = np.array([n - 1 for n in group], dtype=np.int32)
                Kp, Vp, table, num_pages = _setup(seed + g0, start, T, Hkv, dh, page)
                max_pages = table.shape[1]
                cap = max_pages * page
                kc, vc = PO.gather_cache(Kp, table, page, np.nan), PO.gather_cache(Vp, table, page, np.nan)
                q = rnd(seed + g0 + 5, (B * T, H * dh), -1, 1)
                Q, S, TAB = dev.array(q), dev.int_array(start), dev.int_array(table)
                KP, VP, KC, VC = dev.array(Kp), dev.array(Vp), dev.array(kc), dev.array(vc)
                for W in [0] + _windows(dh, page):
                    what = "paged [dh %d page %d T %d H %d Hkv %d n %s W %d]" % (dh, page, T, H, Hkv, group, W)
                    got = _paged(dev, Q, H * dh, KP, VP, S, TAB, max_pages, T, H, Hkv, dh, page, num_pages, W)
                    want = _twin(dev, Q, H * dh, KC, VC, S, cap, T, H, Hkv, dh, W)
                    assert np.all(np.isfinite(got)), what
                    assert np.array_equal(got, want), (what, np.abs(got - want).max())
                    if W == 0 and pi == 0 and T == 1:
                        k0, v0 = np.repeat(np.nan_to_num(kc), H // Hkv, axis=1), np.repeat(np.nan_to_num(vc), H // Hkv, axis=1)
                        ref, ref32 = (DO.decode_forward(q.astype(dt), k0.astype(dt), v0.astype(dt), start, T, scale=_scale(dh))
                                      for dt in (np.float64, np.float32))
                        _check(got, ref, ref32, 1.0, "decode [dh %d page %d H %d Hkv %d n %s]" % (dh, page, H, Hkv, group))


@pytest.mark.parametrize("dh", DHS)
def test_the_bits_do_not_depend_on_anything_outside_the_positions_read(dev, dh):
    """NaN against 1e30 in every unowned page, every unwritten slot of an owned page and every position below the window; -1 /
    num_pages + 5 against INT_MIN / INT_MAX in the table entries past the owned ones; another permutation of the pool: same bits."""
    c = capi()
    ch = c.attention_decode_chunk(dh)
    page, T, H, Hkv = 16, 4, 4, 2
    start = np.array([ch + 3, 2 * ch + 1, page - 1], dtype=np.int32)
    q = rnd(3, (B * T, H * dh), -1, 1)
    for W in (0, ch + 1):
        lo = None if W == 0 else [max(0, int(s) + 1 - W) for s in start]      # row 0's window is the lowest
        outs = []
        for garbage, bad in ((np.nan, (-1, None)), (1e30, (-(1 << 31), (1 << 31) - 1))):
            Kp, Vp, table, num_pages = _setup(77, start, T, Hkv, dh, page, garbage, bad, lo)
            if not np.isnan(garbage):                                    # the second run on another permutation of the same pool
                perm = np.random.default_rng(5).permutation(num_pages)
                Kp2, Vp2 = np.empty_like(Kp), np.empty_like(Vp)
                Kp2[perm], Vp2[perm] = Kp, Vp
                own = (table >= 0) & (table < num_pages)
                table = np.where(own, perm[np.clip(table, 0, num_pages - 1)], table).astype(np.int32)
                Kp, Vp = Kp2, Vp2
            outs.append(_paged(dev, dev.array(q), H * dh, dev.array(Kp), dev.array(Vp), dev.int_array(start), dev.int_array(table),
                               table.shape[1], T, H, Hkv, dh, page, num_pages, W))
        assert np.all(np.isfinite(outs[0])) and np.array_equal(outs[0], outs[1]), (dh, W)


@pytest.mark.parametrize("dh", [64, 20])
def test_shared_pages_give_the_bits_of_private_copies(dev, dh):
    """Samples 0 and 1 name the SAME physical pages for a common prefix of whole pages and have equal queries and equal lengths:
    equal bits, and the bits of the run where sample 1 has private copies of those pages."""
    c = capi()
    ch = c.attention_decode_chunk(dh)
    page, T, H, Hkv = 16, 1, 4, 2
    n = ch + page + 5
    start = np.array([n - 1, n - 1, 40], dtype=np.int32)
    Kp, Vp, table, num_pages = _setup(9, start, T, Hkv, dh, page)
    shared = (ch + page) // page                                         # whole pages of the prefix
    private = table.copy()
    for a in (Kp, Vp):                                                   # sample 1: sample 0's contents throughout, in its own pages
        a[table[1, :shared + 1]] = a[table[0, :shared + 1]]
    table[1, :shared] = table[0, :shared]                                # ... and then sample 0's pages themselves for the prefix
    q = rnd(4, (B * T, H * dh), -1, 1)
    q[1] = q[0]
    for W in (0, ch - 1):
        outs = [_paged(dev, dev.array(q), H * dh, dev.array(Kp), dev.array(Vp), dev.int_array(start), dev.int_array(tab), tab.shape[1], T, H,
                       Hkv, dh, page, num_pages, W) for tab in (table, private)]
        assert np.array_equal(outs[0][0], outs[0][1]), (dh, W)
        assert np.array_equal(outs[0], outs[1]), (dh, W)


# ---- append and copy ----------------------------------------------------------------------------------------------------------------
def _guarded(dev, pools, guard=1024):
    """both pools inside one allocation, between guard bands of SENTINEL: -> (whole array, K view, V view, host image)"""
    n = pools[0].size
    host = np.full(3 * guard + 2 * n, SENTINEL, np.float32)
    host[guard:guard + n] = pools[0].ravel()
    host[2 * guard + n:2 * guard + 2 * n] = pools[1].ravel()
    whole = dev.array(host)
    return whole, whole.view_offset(guard), whole.view_offset(2 * guard + n), host


@pytest.mark.parametrize("dh,ld_extra", [(64, 0), (32, 8), (20, 0), (5, 3), (128, 2)])
def test_append_is_bit_exact_and_touches_nothing_else(dev, dh, ld_extra):
    """Rows land where the model puts them, K and V; every other pool element keeps its sentinel and the guard bands around the
    pools do not move.  Sample 1 runs past cap_v (rows dropped), sample 2's second page has the entry -1, sample 3 starts below 0,
    sample 4's entry is past the pool."""
    c = capi()
    page, T, H = 16, 5, 3
    nb, max_pages, num_pages = 5, 3, 11
    cap = max_pages * page
    start = np.array([14, cap - 2, 13, -2, 30], dtype=np.int32)
    table = np.array([[4, 9, 2], [0, 5, 7], [3, -1, 6], [1, 8, 10], [1, 8, num_pages]], dtype=np.int32)
    ld = H * dh + ld_extra
    k, v = rnd(1, (nb * T, ld), -1, 1), rnd(2, (nb * T, ld), -1, 1)
    Kp, Vp = (np.full((num_pages, H, page, dh), SENTINEL, np.float32) for _ in range(2))
    whole, KP, VP, host = _guarded(dev, (Kp, Vp))
    c.kv_pages_append(dev, KP, VP, dev.array(k), dev.array(v), ld, dev.int_array(start), dev.int_array(table), max_pages, nb, T, H, dh, page,
                      num_pages)
    PO.scatter_rows(Kp, k[:, :H * dh], start, table, T, page)
    PO.scatter_rows(Vp, v[:, :H * dh], start, table, T, page)
    n, guard = Kp.size, 1024
    host[guard:guard + n] = Kp.ravel()
    host[2 * guard + n:2 * guard + 2 * n] = Vp.ravel()
    # rows the model keeps: 5 + 2 (the rest past cap_v) + 3 (the rest behind -1) + 3 (the rest below 0) + 2 (the rest past the pool)
    assert (Kp != SENTINEL).sum() == 15 * H * dh
    assert np.array_equal(whole.numpy(), host)


@pytest.mark.parametrize("dh", [64, 5])
def test_copy_is_bit_exact_and_leaves_the_other_pages(dev, dh):
    c = capi()
    page, H, num_pages = 16, 3, 9
    Kp, Vp = rnd(1, (num_pages, H, page, dh), -1, 1), rnd(2, (num_pages, H, page, dh), -1, 1)
    whole, KP, VP, host = _guarded(dev, (Kp, Vp))
    src = np.array([2, 7, 4, -1, 1, 3], dtype=np.int32)
    dst = np.array([5, 0, 4, 6, num_pages, 8], dtype=np.int32)            # 4 -> 4: a no-op; -1 -> 6 and 1 -> num_pages: dropped
    c.kv_pages_copy(dev, KP, VP, dev.int_array(src), dev.int_array(dst), len(src), H, dh, page, num_pages)
    for a in (Kp, Vp):
        a[5], a[0], a[8] = a[2].copy(), a[7].copy(), a[3].copy()
    n, guard = Kp.size, 1024
    host[guard:guard + n] = Kp.ravel()
    host[2 * guard + n:2 * guard + 2 * n] = Vp.ravel()
    assert np.array_equal(whole.numpy(), host)
    c.kv_pages_copy(dev, KP, VP, dev.int_array(src), dev.int_array(dst), 0, H, dh, page, num_pages)       # n = 0: NK_OK, no launch
