"""GPU parity of sliding-window decoding through the C ABI: nk_attention_decode_window_fwd (position-aligned split-KV partials over
the window's chunks only, merged in chunk order; linear and rolling caches; ungrouped and grouped) and nk_kv_cache_append_ring (a
bit-exact transposing copy to slot (start + t) % cap) against tests/window_oracle.py.

Tolerance: tests/test_gpu_attention_decode.py's rule, unchanged - kernels and f32 oracle both measured against the f64 oracle; pass
iff err_gpu <= max(2 * err_cpu32, 1e-6 * scale), scale = max(|ref|max, |v|max) (SURVEY.md 8c ii), margins recorded under
`attention_window:*`.

Bit contracts checked here (include/neuronika_hip.h, "sliding-window decoding"):
  (1) n <= window: the bits of nk_attention_decode_gqa_fwd / nk_attention_decode_fwd on the same inputs;
  (2) a ring cache gives the bits of a linear cache holding the same positions' contents;
  (3) the bits of o for (b, h, t) depend on that problem's q, its keys / values at [lo, n), n, W and scale only - not on B, T, cap,
      ring, the other samples, or what a slot outside the window holds (NaN, 1e30);
  (4) grouped bits equal ungrouped bits on the cache with every kv head repeated."""
import numpy as np
import pytest

import decode_oracle as DO
import window_oracle as WO

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
DHS = [32, 64, 128, 20, 5]
GEOMETRIES = [(1, 1, 1), (2, 4, 4), (3, 4, 2), (2, 8, 1)]               # (B, H, Hkv)


def capi():
    from neuronika_amd import capi as c
    return c


def rnd(seed, shape, lo, hi):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    return np.asarray(a * np.float32(hi - lo) + np.float32(lo), dtype=np.float32)


def _check(got, want64, want32, vmax, what):
    scale = max(np.abs(want64).max(), vmax)
    err_gpu, err_cpu = np.abs(got - want64).max(), np.abs(want32 - want64).max()
    from conftest import record_margin
    record_margin("attention_window:" + what.split("[")[0].strip(), err_gpu, err_cpu, 1e-6 * scale)
    print(what, "err_gpu %.3g err_cpu32 %.3g bound %.3g" % (err_gpu, err_cpu, max(2 * err_cpu, 1e-6 * scale)))
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)   # SURVEY 8c (ii) as stated


def _scale(dh):
    return float(np.float32(1.0 / np.sqrt(dh)))


def _window(dev, q, kc, vc, start, T, H, W, ring, ldq=None):
    """nk_attention_decode_window_fwd on host arrays: q (B*T, H*dh), kc / vc (B, Hkv, cap, dh) -> (B*T, H*dh)"""
    c = capi()
    B, Hkv, cap, dh = kc.shape
    out = dev.full((B * T, H * dh), np.nan)
    ws = dev.full((c.attention_decode_window_workspace(B, T, H, dh, W),), np.nan)
    c.attention_decode_window_fwd(dev, dev.array(q), ldq or H * dh, dev.array(kc), dev.array(vc), dev.int_array(start), out, ws, B, T, H, Hkv, dh,
                                  cap, W, ring, _scale(dh))
    return out.numpy()


def _oracles(q, kc, vc, start, T, H, W, ring=False):
    dh = kc.shape[3]
    return tuple(WO.decode_forward(q.astype(dt), kc.astype(dt), vc.astype(dt), start, T, W, ring, H=H, scale=_scale(dh))
                 for dt in (np.float64, np.float32))


def _pad(a, cap, fill=np.nan):
    """a linear cache (B, Hkv, n, dh) in a capacity of cap >= n"""
    B, Hkv, n, dh = a.shape
    return np.concatenate([a, np.full((B, Hkv, cap - n, dh), fill, np.float32)], axis=2)


# ---- the grid against the oracle -------------------------------------------------------------------------------------------------
def _windows(dh):
    ch = capi().attention_decode_chunk(dh)
    return [1, 2, ch - 1, ch, ch + 1, 2 * ch + 3]


def _lengths(dh, W):
    """what the FIRST new row of a sample reads up to: lo and n on, before and after every chunk seam"""
    ch = capi().attention_decode_chunk(dh)
    return sorted({n for n in (1, W - 1, W, W + 1, ch, ch + 1, W + ch - 1, W + ch, 2 * ch + W + 5) if n >= 1})


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("B,H,Hkv", GEOMETRIES)
@pytest.mark.parametrize("dh", DHS)
def test_window_decode_equals_oracle(dev, dh, B, H, Hkv, T):
    """Every length of `_lengths` is what the first new row of some sample reads (start = n - 1; the later rows of a T = 4 slice
    read n + 1 .. n + 3, crossing the seams again), ragged across the samples of a call.  The positions' contents are drawn once
    per call group and laid out four ways - a linear cache of the tightest capacity and one 2C + 13 above it, a ring of the smallest
    legal capacity W + T - 1 and one C + 13 above it, both filled from the host in ring layout - and ONE pair of oracle runs serves
    all four.  The step's own rows reach the cache through nk_kv_cache_append / nk_kv_cache_append_ring from a packed
    (B*T, d + 2 dkv) projection, which the queries are read from in place."""
    c = capi()
    d, dkv, ch = H * dh, Hkv * dh, c.attention_decode_chunk(dh)
    ld = d + 2 * dkv
    for W in _windows(dh):
        ns = _lengths(dh, W)
        ns = ns + ns[:(-len(ns)) % B]                                    # whole groups of B
        for g0 in range(0, len(ns), B):
            group = ns[g0:g0 + B]
            start = np.array([n - 1 for n in group], dtype=np.int32)
            n_max = int(start.max()) + T
            kl, vl = rnd(10 + g0, (B, Hkv, n_max, dh), -1, 1), rnd(20 + g0, (B, Hkv, n_max, dh), -1, 1)
            qkv = rnd(30 + g0, (B * T, ld), -1, 1)
            before_k, before_v = kl.copy(), vl.copy()
            for b in range(B):                                           # what the append has yet to write, and the tail
                before_k[b, :, start[b]:] = np.nan
                before_v[b, :, start[b]:] = np.nan
            DO.append(kl, vl, qkv[:, d:d + dkv], qkv[:, d + dkv:], start, T)
            q = np.ascontiguousarray(qkv[:, :d])
            ref, ref32 = _oracles(q, kl, vl, start, T, H, W)
            vmax = max(float(np.abs(vl[b, :, :start[b] + T]).max()) for b in range(B))
            S, QKV = dev.int_array(start), dev.array(qkv)
            ws = dev.full((c.attention_decode_window_workspace(B, T, H, dh, W),), np.nan)
            layouts = [(0, n_max), (0, n_max + 2 * ch + 13), (1, W + T - 1), (1, W + T - 1 + ch + 13)]
            for ring, cap in layouts:
                if ring:
                    Kc, Vc = dev.array(WO.ring_image(before_k, start, cap)), dev.array(WO.ring_image(before_v, start, cap))
                    c.kv_cache_append_ring(dev, Kc, Vc, QKV.view_offset(d), QKV.view_offset(d + dkv), ld, S, B, T, Hkv, dh, cap)
                else:
                    Kc, Vc = dev.array(_pad(before_k, cap)), dev.array(_pad(before_v, cap))
                    c.kv_cache_append(dev, Kc, Vc, QKV.view_offset(d), QKV.view_offset(d + dkv), ld, S, B, T, Hkv, dh, cap)
                out = dev.full((B * T, d), np.nan)
                c.attention_decode_window_fwd(dev, QKV, ld, Kc, Vc, S, out, ws, B, T, H, Hkv, dh, cap, W, ring, _scale(dh))
                got = out.numpy()
                what = "window [dh %d B %d H %d Hkv %d T %d W %d n %s %s cap %d]" % (dh, B, H, Hkv, T, W, group, "ring" if ring else "linear", cap)
                assert np.all(np.isfinite(got)), what
                _check(got, ref, ref32, vmax, what)


@pytest.mark.parametrize("dh", DHS)
def test_ring_steps_that_straddle_the_wrap(dev, dh):
    """T = 4 at start % cap = cap - 2: rows 0, 1 land on the last two slots and rows 2, 3 on the first two; start > 3 * cap; the
    ring is filled from the host (every slot random: the slots outside a row's window hold other positions' keys)."""
    c = capi()
    B, H, Hkv, T = 2, 4, 2, 4
    d, dkv, ch = H * dh, Hkv * dh, c.attention_decode_chunk(dh)
    ld = d + 2 * dkv
    for W in (2, ch - 1, ch + 1, 2 * ch + 3):
        for cap in (W + T - 1, W + T - 1 + ch + 13):
            start = np.array([4 * cap + cap - 2, 3 * cap + cap - 2], dtype=np.int32)
            assert np.all(start % cap == cap - 2) and np.all(start > 3 * cap)
            kc, vc = rnd(1, (B, Hkv, cap, dh), -1, 1), rnd(2, (B, Hkv, cap, dh), -1, 1)
            qkv = rnd(3, (B * T, ld), -1, 1)
            Kc, Vc, S, QKV = dev.array(kc), dev.array(vc), dev.int_array(start), dev.array(qkv)
            c.kv_cache_append_ring(dev, Kc, Vc, QKV.view_offset(d), QKV.view_offset(d + dkv), ld, S, B, T, Hkv, dh, cap)
            WO.append(kc, vc, qkv[:, d:d + dkv], qkv[:, d + dkv:], start, T, ring=True)
            assert np.array_equal(Kc.numpy(), kc) and np.array_equal(Vc.numpy(), vc)
            out = dev.full((B * T, d), np.nan)
            ws = dev.full((c.attention_decode_window_workspace(B, T, H, dh, W),), np.nan)
            c.attention_decode_window_fwd(dev, QKV, ld, Kc, Vc, S, out, ws, B, T, H, Hkv, dh, cap, W, 1, _scale(dh))
            q = np.ascontiguousarray(qkv[:, :d])
            ref, ref32 = _oracles(q, kc, vc, start, T, H, W, ring=True)
            got = out.numpy()
            assert np.all(np.isfinite(got))
            _check(got, ref, ref32, float(np.abs(vc).max()), "wrap [dh %d W %d cap %d]" % (dh, W, cap))


# ---- the bit contract ------------------------------------------------------------------------------------------------------------
def _ragged(dh, B, Hkv, H, T, seed=0):
    """three samples whose first rows read C + 4, 3 and 2.5 C + 2 keys: positions' contents (B, Hkv, n_max, dh), queries, starts"""
    ch = capi().attention_decode_chunk(dh)
    start = np.array([ch + 3, 2, 2 * ch + ch // 2 + 1][:B], dtype=np.int32)
    n_max = int(start.max()) + T
    kl, vl = rnd(seed + 1, (B, Hkv, n_max, dh), -1, 1), rnd(seed + 2, (B, Hkv, n_max, dh), -1, 1)
    return rnd(seed + 3, (B * T, H * dh), -1, 1), kl, vl, start, n_max


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2), (8, 1)])
@pytest.mark.parametrize("dh", DHS)
def test_a_window_that_holds_every_key_gives_the_bits_of_the_unwindowed_call(dev, dh, H, Hkv, T):
    """(1): n <= window for every row - W = the longest row, one more, and far more than the capacity."""
    c = capi()
    B = 3
    q, kl, vl, start, n_max = _ragged(dh, B, Hkv, H, T)
    cap = n_max + 5
    kc, vc = _pad(kl, cap), _pad(vl, cap)
    Q, Kc, Vc, S = dev.array(q), dev.array(kc), dev.array(vc), dev.int_array(start)
    want = dev.full((B * T, H * dh), np.nan)
    ws = dev.full((c.attention_decode_workspace(B, T, H, dh, cap),), np.nan)
    c.attention_decode_gqa_fwd(dev, Q, H * dh, Kc, Vc, S, want, ws, B, T, H, Hkv, dh, cap, _scale(dh))
    want = want.numpy()
    if Hkv == H:
        plain = dev.full((B * T, H * dh), np.nan)
        c.attention_decode_fwd(dev, Q, H * dh, Kc, Vc, S, plain, ws, B, T, H, dh, cap, _scale(dh))
        assert np.array_equal(plain.numpy(), want)
    assert np.all(np.isfinite(want))
    for W in (n_max, n_max + 1, 100 * cap):
        assert np.array_equal(_window(dev, q, kc, vc, start, T, H, W, 0), want), W
    # and on a ring that has not wrapped yet (cap >= n_max): the slots are the positions
    ring_cap = n_max + T - 1
    assert np.array_equal(_window(dev, q, _pad(kl, ring_cap), _pad(vl, ring_cap), start, T, H, n_max, 1), want)


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2)])
@pytest.mark.parametrize("dh", DHS)
def test_a_ring_gives_the_bits_of_a_linear_cache(dev, dh, H, Hkv, T):
    """(2): the same positions' contents in a linear cache and in rings of two capacities that have wrapped several times."""
    ch = capi().attention_decode_chunk(dh)
    B = 3
    q, kl, vl, start, n_max = _ragged(dh, B, Hkv, H, T)
    for W in (3, ch // 2 + 1, ch + 2):
        linear = _window(dev, q, kl, vl, start, T, H, W, 0)
        assert np.all(np.isfinite(linear))
        for cap in (W + T - 1, W + T - 1 + ch // 3):
            kr, vr = WO.ring_image(kl, start + T, cap), WO.ring_image(vl, start + T, cap)
            assert np.array_equal(_window(dev, q, kr, vr, start, T, H, W, 1), linear), (W, cap)
    ref, ref32 = _oracles(q, kl, vl, start, T, H, W)
    _check(linear, ref, ref32, float(np.abs(vl).max()), "ring against linear [dh %d H %d Hkv %d T %d]" % (dh, H, Hkv, T))


def _poisoned(a, start, T, W, fill, ring, cap):
    """every slot no row of the step may read - outside [lo of row 0, n of row T - 1) - holding `fill`"""
    out = a.copy()
    for b, s in enumerate(start):
        lo, n = max(0, int(s) + 1 - W), int(s) + T
        outside = np.ones(out.shape[2], dtype=bool)
        outside[[WO.slot(p, cap, ring) for p in range(lo, n)]] = False
        out[b][:, outside] = fill
    return out


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("ring", [0, 1], ids=["linear", "ring"])
@pytest.mark.parametrize("dh", DHS)
def test_slots_outside_the_window_never_reach_the_result(dev, dh, ring, T):
    """(3): the slots outside every row's window - positions below lo and the tail, or on a ring the slots of older positions -
    holding 0, NaN and 1e30: identical bits, all finite.  (Rows t > 0 have a higher lo than row 0: the slots between are poisoned
    for them in the T = 1 runs of test_a_row_depends_on_its_own_problem_only.)"""
    ch = capi().attention_decode_chunk(dh)
    B, H, Hkv = 3, 4, 2
    q, kl, vl, start, n_max = _ragged(dh, B, Hkv, H, T)
    for W in (2, ch - 1, ch + 1):
        cap = W + T - 1 + ch + 9 if ring else n_max + ch + 9
        kc, vc = (WO.ring_image(a, start + T, cap) if ring else _pad(a, cap) for a in (kl, vl))
        runs = [_window(dev, q, _poisoned(kc, start, T, W, fill, ring, cap), _poisoned(vc, start, T, W, fill, ring, cap), start, T, H, W, ring)
                for fill in (0.0, np.nan, 1e30)]
        assert np.all(np.isfinite(runs[0])), W
        assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), W
    ref, ref32 = _oracles(q, kl, vl, start, T, H, W)
    _check(runs[1], ref, ref32, float(np.abs(vl).max()), "poisoned [dh %d T %d %s]" % (dh, T, "ring" if ring else "linear"))


@pytest.mark.parametrize("dh", DHS)
def test_a_row_depends_on_its_own_problem_only(dev, dh):
    """(3): sample b inside B = 3 equals the sample alone (B = 1); row t of a T = 4 call equals a T = 1 call at start + t with
    everything outside ITS window poisoned; two linear capacities and two ring capacities; one head of one sample alone."""
    ch = capi().attention_decode_chunk(dh)
    B, H, Hkv, T = 3, 4, 2, 4
    q, kl, vl, start, n_max = _ragged(dh, B, Hkv, H, T)
    for W in (ch - 1, ch + 1):
        together = _window(dev, q, kl, vl, start, T, H, W, 0)
        assert np.all(np.isfinite(together))
        assert np.array_equal(_window(dev, q, _pad(kl, n_max + 3 * ch + 1), _pad(vl, n_max + 3 * ch + 1), start, T, H, W, 0), together)
        for cap in (W + T - 1, W + T + ch):
            kr, vr = WO.ring_image(kl, start + T, cap), WO.ring_image(vl, start + T, cap)
            assert np.array_equal(_window(dev, q, kr, vr, start, T, H, W, 1), together), cap
        for b in range(B):
            alone = _window(dev, q[b * T:(b + 1) * T], kl[b:b + 1], vl[b:b + 1], start[b:b + 1], T, H, W, 0)
            assert np.array_equal(alone, together[b * T:(b + 1) * T]), b
            for t in range(T):
                st = start[b:b + 1] + t
                kp, vp = (_poisoned(a[b:b + 1], st, 1, W, np.nan, 0, n_max) for a in (kl, vl))
                one = _window(dev, q[b * T + t:b * T + t + 1], kp, vp, st, 1, H, W, 0)
                assert np.array_equal(one[0], together[b * T + t]), (b, t)
        # kv head 1 of sample 2 alone, with the two query heads of its group: H = 2, Hkv = 1
        b, kv, G = 2, 1, H // Hkv
        cols = slice(kv * G * dh, (kv + 1) * G * dh)
        one = _window(dev, np.ascontiguousarray(q[b * T:(b + 1) * T, cols]), kl[b:b + 1, kv:kv + 1], vl[b:b + 1, kv:kv + 1], start[b:b + 1], T, G, W, 0)
        assert np.array_equal(one, together[b * T:(b + 1) * T, cols])


@pytest.mark.parametrize("ring", [0, 1], ids=["linear", "ring"])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (8, 1), (12, 1)])
@pytest.mark.parametrize("dh", DHS)
def test_grouped_bits_equal_ungrouped_bits_on_the_repeated_cache(dev, dh, H, Hkv, ring):
    """(4): groups of 2, 8 and 12 (two blocks per kv head) against the ungrouped kernel on the cache with every kv head repeated."""
    ch = capi().attention_decode_chunk(dh)
    B, T, G = 3, 2, H // Hkv
    q, kl, vl, start, n_max = _ragged(dh, B, Hkv, H, T)
    for W in (ch // 2, ch + 1):
        cap = W + T - 1 + 11 if ring else n_max
        kc, vc = (WO.ring_image(a, start + T, cap) if ring else a for a in (kl, vl))
        grouped = _window(dev, q, kc, vc, start, T, H, W, ring)
        assert np.all(np.isfinite(grouped))
        assert np.array_equal(grouped, _window(dev, q, np.repeat(kc, G, axis=1), np.repeat(vc, G, axis=1), start, T, H, W, ring)), W
    ref, ref32 = _oracles(q, kl, vl, start, T, H, W)
    _check(grouped, ref, ref32, float(np.abs(vl).max()), "grouped [dh %d H %d Hkv %d %s]" % (dh, H, Hkv, "ring" if ring else "linear"))


def test_runs_repeat_bit_for_bit_and_a_negative_start_gives_zero(dev):
    dh, B, H, Hkv, T = 64, 4, 16, 4, 1
    ch = capi().attention_decode_chunk(dh)
    W, n = 2 * ch + 5, 4 * ch + 5                                        # three or four chunks per problem
    kl, vl, q = rnd(1, (B, Hkv, n, dh), -1, 1), rnd(2, (B, Hkv, n, dh), -1, 1), rnd(3, (B * T, H * dh), -1, 1)
    start = np.array([n - 1, -1, n - 7, -40], dtype=np.int32)
    first = _window(dev, q, kl, vl, start, T, H, W, 0)
    for _ in range(3):
        assert np.array_equal(_window(dev, q, kl, vl, start, T, H, W, 0), first)
    assert np.all(first[1] == 0) and np.all(first[3] == 0)
    ref, ref32 = _oracles(q, kl, vl, start, T, H, W)
    _check(first, ref, ref32, float(np.abs(vl).max()), "repeat")


@pytest.mark.parametrize("dh", [64, 20])
def test_one_dominant_key_in_the_window(dev, dh):
    """k_j = 8 q / |q| for one in-window j per problem, in different chunks of the window, and one just BELOW lo: the partials of the
    other chunks are rescaled by a tiny factor in the merge, and the key outside the window must not be seen at all."""
    B, H, T = 2, 2, 1
    ch = capi().attention_decode_chunk(dh)
    W, n = 2 * ch + 3, 3 * ch + 7
    lo = n - W
    kl, vl, q = rnd(1, (B, H, n, dh), -1, 1), rnd(2, (B, H, n, dh), -1, 1), rnd(3, (B * T, H * dh), -1, 1)
    for b in range(B):
        for h in range(H):
            qr = q[b, h * dh:(h + 1) * dh]
            big = np.float32(8.0) * qr / np.float32(np.linalg.norm(qr))
            kl[b, h, [lo, ch + ch // 2, 2 * ch - 1, n - 1][2 * b + h]] = big
            kl[b, h, lo - 1] = np.float32(4.0) * big                     # outside: would win by far
    start = np.full(B, n - 1, dtype=np.int32)
    ref, ref32 = _oracles(q, kl, vl, start, T, H, W)
    _check(_window(dev, q, kl, vl, start, T, H, W, 0), ref, ref32, float(np.abs(vl).max()), "dominant key [dh %d]" % dh)


def test_queries_are_read_with_their_row_stride(dev):
    c = capi()
    dh, B, H, Hkv, T, W = 64, 2, 4, 2, 3, 70
    q, kl, vl, start, n_max = _ragged(dh, B, Hkv, H, T)
    wide = rnd(9, (B * T, 3 * H * dh + 4), -1, 1)
    wide[:, 4:4 + H * dh] = q
    Wd = dev.array(wide)
    out = dev.full((B * T, H * dh), np.nan)
    ws = dev.full((c.attention_decode_window_workspace(B, T, H, dh, W),), np.nan)
    c.attention_decode_window_fwd(dev, Wd.view_offset(4), wide.shape[1], dev.array(kl), dev.array(vl), dev.int_array(start), out, ws, B, T, H, Hkv,
                                  dh, n_max, W, 0, _scale(dh))
    assert np.array_equal(out.numpy(), _window(dev, q, kl, vl, start, T, H, W, 0))


# ---- the ring append -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,H,dh", [(2, 1, 3, 64), (3, 4, 2, 32), (2, 5, 2, 20), (2, 3, 2, 5), (1, 40, 4, 128)])
@pytest.mark.parametrize("packed", [True, False])
def test_ring_append_is_a_bit_exact_copy_that_wraps_inside_a_call(dev, B, T, H, dh, packed):
    """Starts far past the capacity, the rows of one call wrapping from the last slots to the first; the caches sit inside a
    larger allocation whose guard bands must not move; every other slot keeps its sentinel."""
    c = capi()
    d, cap, guard = H * dh, 50, 64
    start = np.array([cap * 7 + cap - 2, 0, 3 * cap + 17][:B], dtype=np.int32)
    if T == 40:
        start[:] = 5 * cap + 30                                          # 20 rows before the wrap, 20 after
    kc0, vc0 = np.full((B, H, cap, dh), SENTINEL, np.float32), np.full((B, H, cap, dh), -SENTINEL, np.float32)
    big_k, big_v = dev.full((guard + kc0.size + guard,), SENTINEL), dev.full((guard + vc0.size + guard,), -SENTINEL)
    Kc, Vc, S = big_k.view_offset(guard), big_v.view_offset(guard), dev.int_array(start)
    if packed:                                                           # K and V are column blocks of one (B*T, 3d) matrix
        qkv = rnd(1, (B * T, 3 * d), -1, 1)
        QKV = dev.array(qkv)
        k, v = qkv[:, d:2 * d], qkv[:, 2 * d:]
        c.kv_cache_append_ring(dev, Kc, Vc, QKV.view_offset(d), QKV.view_offset(2 * d), 3 * d, S, B, T, H, dh, cap)
    else:
        k, v = rnd(2, (B * T, d), -1, 1), rnd(3, (B * T, d), -1, 1)
        c.kv_cache_append_ring(dev, Kc, Vc, dev.array(k), dev.array(v), d, S, B, T, H, dh, cap)
    WO.append(kc0, vc0, k, v, start, T, ring=True)
    assert np.count_nonzero(kc0 != SENTINEL) == B * T * H * dh           # every row written, none twice
    if T > 1:
        assert np.any(kc0[0, :, 0] != SENTINEL) and np.any(kc0[0, :, cap - 1] != SENTINEL)    # sample 0 wrapped inside the call
    for big, want, fill in ((big_k, kc0, SENTINEL), (big_v, vc0, -SENTINEL)):
        got = big.numpy()
        assert np.all(got[:guard] == fill) and np.all(got[-guard:] == fill)
        assert np.array_equal(got[guard:-guard].reshape(want.shape), want)


def test_ring_append_skips_negative_positions(dev):
    c = capi()
    B, T, H, dh, cap = 2, 4, 2, 8, 6
    start = np.array([-2, -9], dtype=np.int32)                           # sample 0: rows 2, 3 at positions 0, 1; sample 1: none
    k, v = rnd(1, (B * T, H * dh), -1, 1), rnd(2, (B * T, H * dh), -1, 1)
    kc0, vc0 = np.full((B, H, cap, dh), SENTINEL, np.float32), np.full((B, H, cap, dh), SENTINEL, np.float32)
    Kc, Vc = dev.array(kc0), dev.array(vc0)
    c.kv_cache_append_ring(dev, Kc, Vc, dev.array(k), dev.array(v), H * dh, dev.int_array(start), B, T, H, dh, cap)
    WO.append(kc0, vc0, k, v, start, T, ring=True)
    assert np.array_equal(Kc.numpy(), kc0) and np.array_equal(Vc.numpy(), vc0)
    assert np.all(kc0[1] == SENTINEL) and np.count_nonzero(kc0[0] != SENTINEL) == 2 * H * dh


# ---- rejections ----------------------------------------------------------------------------------------------------------------------
def _raises_invalid(fn):
    c = capi()
    with pytest.raises(c.NeuronikaHipError) as e:
        fn()
    assert e.value.code == 1, e.value                                            # NK_ERR_INVALID


def test_invalid_arguments_are_refused_and_nothing_is_written(dev):
    c = capi()
    B, T, H, Hkv, dh, cap, W = 2, 3, 4, 2, 64, 16, 8
    d, dkv = H * dh, Hkv * dh
    Q, K, V = dev.zeros((B * T, d)), dev.zeros((B * T, dkv)), dev.zeros((B * T, dkv))
    Kc, Vc, S = dev.full((B, Hkv, cap, dh), SENTINEL), dev.full((B, Hkv, cap, dh), SENTINEL), dev.int_zeros((B,))
    out = dev.full((B * T, d), SENTINEL)
    ws = dev.full((c.attention_decode_window_workspace(B, T, H, dh, W),), SENTINEL)
    good = dict(B=B, T=T, H=H, Hkv=Hkv, dh=dh, cap=cap, window=W, ring=1, scale=0.125)
    app = dict(B=B, T=T, H=Hkv, dh=dh, cap=cap)
    bad_calls = []
    for key in ("B", "T", "H", "Hkv", "dh", "cap", "window"):
        for bad in (0, -1):
            bad_calls.append(dict(good, **{key: bad}))
    bad_calls += [dict(good, Hkv=3), dict(good, Hkv=8)]
    bad_calls += [dict(good, window=cap), dict(good, window=cap - T + 2)]        # ring: window + T - 1 > cap
    bad_calls += [dict(good, scale=s) for s in (0.0, -0.125, float("nan"), float("inf"))]
    for args in bad_calls:
        _raises_invalid(lambda: c.attention_decode_window_fwd(dev, Q, d, Kc, Vc, S, out, ws, **args))
    ptrs = [Q, Kc, Vc, S, out, ws]
    for i in range(len(ptrs)):
        a = list(ptrs); a[i] = None
        _raises_invalid(lambda: c.attention_decode_window_fwd(dev, a[0], d, a[1], a[2], a[3], a[4], a[5], **good))
    _raises_invalid(lambda: c.attention_decode_window_fwd(dev, Q, d - 1, Kc, Vc, S, out, ws, **good))          # rows would overlap
    _raises_invalid(lambda: c.attention_decode_window_fwd(dev, Q, d, Kc.view_offset(1), Vc, S, out, ws, **dict(good, cap=cap - 1, window=4)))
    for key in app:
        for bad in (0, -1):
            _raises_invalid(lambda: c.kv_cache_append_ring(dev, Kc, Vc, K, V, dkv, S, **dict(app, **{key: bad})))
    _raises_invalid(lambda: c.kv_cache_append_ring(dev, Kc, Vc, K, V, dkv, S, **dict(app, cap=T - 1)))          # T > cap
    _raises_invalid(lambda: c.kv_cache_append_ring(dev, Kc, Vc, K, V, dkv - 1, S, **app))
    ptrs = [Kc, Vc, K, V, S]
    for i in range(len(ptrs)):
        a = list(ptrs); a[i] = None
        _raises_invalid(lambda: c.kv_cache_append_ring(dev, a[0], a[1], a[2], a[3], dkv, a[4], **app))
    for buf in (Kc, Vc, out, ws):                                                # nothing was written by any refused call
        assert np.all(buf.numpy() == SENTINEL)
    # the valid calls pass: the largest legal window of this ring, and the same window on a linear cache of the same capacity
    c.kv_cache_append_ring(dev, Kc, Vc, K, V, dkv, S, **app)
    c.attention_decode_window_fwd(dev, Q, d, Kc, Vc, S, out, ws, **dict(good, window=cap - T + 1))
    c.attention_decode_window_fwd(dev, Q, d, Kc, Vc, S, out, ws, **dict(good, window=cap, ring=0))
    assert np.all(np.isfinite(out.numpy()))
    assert c.attention_decode_window_workspace(B, T, H, dh, 0) == 0 and c.attention_decode_window_workspace(B, T, H, 0, W) == 0
