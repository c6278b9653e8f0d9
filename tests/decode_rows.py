"""Score rows that move the split-KV shift of the decode attention across chunks, and a NumPy replay of the kernels' arithmetic.

The kernels (nk_attention_decode.h and its three bodies) cut a problem's keys into chunks aligned to absolute positions.  A chunk's
shift is its own exact maximum, taken per wave and then over the four waves through LDS (`red`); the combine merges the chunks with
exp2(m_c - M), M = max m_c; the grouped kernels run up to eight heads, head by head, over the same registers and the same LDS
scratch.  A softmax is invariant under any shift that neither overflows nor underflows, and on uniform [-1, 1) data - every other
decode test - all chunk maxima lie within 2 log2 units of each other and of 0: the first chunk's shift, another head's shift or no
shift at all give the same result there.  The row kinds here do not (KINDS below).

Exact scores.  Every q and k entry is a multiple of 1/8 with |x| <= 16 (`attention_rows.grid`): a dot product over dh <= 128 has
fewer than 24 significant bits in ANY summation order, so the kernel's s = d * c1 has the same bits on the device and in the
replay.  v stays uniform [-1, 1).

One cache serves all kinds.  The heads of a group share K, so a row's kind is chosen by q alone.  K carries two structured
components on disjoint coordinate sets and grid noise (|x| <= 3/4) on the odd coordinates:
    coordinates 0 mod 4   a ramp in the position j: -12 + floor(64 j / C) / 8, a new level exactly at every chunk seam, capped at 12
    coordinates 2 mod 4   the constant of LIFT[dh]
and q lifts one of the two sets (LIFT[dh]; 0 on the other), with grid noise on the odd coordinates:
    plain     no lift: the control, every score within ~2 log2 units of 0
    climbing  ramp, +a: the maximum is among the newest keys (the key at kC opens a new level: at n = kC + 1 it is the one key of the
              last chunk), a whole chunk's maximum sits ~145 log2 units above the one before
    falling   ramp, -a: the maximum is in the first chunk, the later chunks underflow in the merge
    lifted    constant, +a: every score carries one offset above +130
    sunk      constant, -a: every score carries one offset below -130
    peaked    the odd coordinates are 8 x (16 x at dh 5) those of one key of the window (`peak_position`: the key of largest norm of
              a chunk that is not the first; neighbouring heads take different chunks), 0 elsewhere
    edge      window forms.  Three BEACON keys are planted in K's odd coordinates at positions lo - 1 (all +1), lo (+1, -1, ...) and
              n - 1 (all -1) of the LAST row of a step, in the kv heads that serve an edge head (no `peaked` head reads those); q's
              odd coordinates are 8 x the beacon at lo - 1: a key that would hold all the mass and must not count
    edge_in   q's odd coordinates are 4 x (beacon at lo + beacon at n - 1): the first and the last key of the window share the mass
tests/test_oracle_decode_rows.py asserts the spreads; they are not taken on trust.

`replay` restates the kernels' arithmetic per problem in f32 NumPy; `flaws` switches on wrong behaviours, the idiom of
tests/adamw_oracle.py and tests/attention_rows.py.  CASES are the committed problems, shared by the CPU and the GPU file."""
import collections
import functools

import numpy as np

from attention_rows import grid, uniform
import decode_oracle as DO
import gqa_oracle as GO
import window_oracle as WO

f32 = np.float32

DHS = (32, 64, 128, 20, 5)
KINDS = ("plain", "climbing", "falling", "lifted", "sunk", "peaked", "edge", "edge_in")
FLAWS = ("no_shift", "wave_local_max", "stale_head_max", "combine_first_m", "combine_no_rescale", "combine_l_unscaled", "lo_off_by_one")
# the flaws that are a different - but consistent - shift: invisible wherever nothing overflows or underflows
SHIFT_FLAWS = ("no_shift", "stale_head_max", "combine_first_m")

THREADS, KPG, GQA_HEADS = 256, 16, 8            # nk_attention_decode.h: ADEC_THREADS, ADEC_KPG, ADEC_GQA_HEADS
LOG2E_F32 = f32(1.44269504088896341)
TINY = f32(2.0 ** -126)                         # v_exp_f32 flushes what lies below
SPREAD = 130.0                                  # log2 units: exp2 of it overflows f32, of its negative flushes to 0

# per dh: (a on the ramp coordinates, a on the constant coordinates, the constant in K).  Chosen so that, with c1 = log2(e) /
# sqrt(dh), n0 = ceil(dh / 4) ramp coordinates and n2 constant coordinates: a * n0 * c1 * 8.125 (two chunks and one key of ramp)
# = 144 .. 152 and a * n2 * const * c1 = 144 .. 155; the noise moves a score by less than 5.
LIFT = {32: (9.0, 6.0, 12.0), 64: (6.5, 4.0, 13.0), 128: (4.5, 3.0, 12.0), 20: (11.0, 8.0, 12.0), 5: (14.0, 16.0, 14.0)}
PEAK = {32: 8.0, 64: 8.0, 128: 8.0, 20: 8.0, 5: 16.0}
K_NOISE = 0.75


def chunk(dh):
    """nk_attention_decode_chunk(dh), restated: tests/test_oracle_decode_rows.py holds it to the library's."""
    return (THREADS // (dh // 4)) * KPG if dh in (32, 64, 128) else 256


def scale_of(dh):
    return f32(1.0 / np.sqrt(dh))


def c1_of(dh):
    return f32(scale_of(dh) * LOG2E_F32)        # nk_attention_decode.h: c1 = scale * ADEC_LOG2E


def ramp(j, C):
    return np.minimum(-12.0 + np.floor(64.0 * np.asarray(j, np.float64) / C) / 8.0, 12.0)


# ---- the committed cases ---------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name form dh B H Hkv T start cap W ring kinds")


def _cases(dh):
    """Per head size, the smallest shapes at which each mechanism exists.  Lengths: C + 1 (two chunks, the second of one key),
    2C + 1, 3C + 7, and T = 4 at start = kC - 2 (four rows across a chunk seam)."""
    C = chunk(dh)
    P, U, D, L, S, K, E, I = KINDS
    eight = ((L, S, L, S, U, D, K, P), (S, L, D, U, P, K, S, L))
    return [
        # plain form: B = 2, H = 3, every head of every sample another kind
        Case("plain-two", "plain", dh, 2, 3, 3, 1, (C, 2 * C), 2 * C + 1, 0, 0, ((U, S, K), (D, L, P))),
        Case("plain-four", "plain", dh, 2, 3, 3, 1, (3 * C + 6, C), 3 * C + 20, 0, 0, ((D, U, L), (P, K, S))),
        Case("plain-seam", "plain", dh, 2, 3, 3, 4, (C - 2, 2 * C - 2), 2 * C + 7, 0, 0, ((L, D, U), (K, S, P))),
        # grouped form: lifted and sunk neighbours alternate inside a block; (12, 1) is two blocks of 8 and 4 heads
        Case("gqa-4x2", "gqa", dh, 2, 4, 2, 1, (C, 2 * C), 2 * C + 1, 0, 0, ((L, S, U, D), (K, P, S, L))),
        Case("gqa-8x1", "gqa", dh, 2, 8, 1, 4, (C - 2, 2 * C - 2), 2 * C + 7, 0, 0, eight),
        Case("gqa-12x1", "gqa", dh, 2, 12, 1, 1, (3 * C + 6, C), 3 * C + 20, 0, 0,
             ((L, S, U, D, K, P, S, L, S, L, K, U), (S, L, D, U, P, K, L, S, L, S, U, D))),
        # window form.  W = C - 1: across one seam (n = 2C + 1) and inside one chunk (n = 2C: the single-chunk write)
        Case("win-linear-1", "window", dh, 2, 4, 4, 1, (2 * C, 2 * C - 1), 2 * C + 10, C - 1, 0, ((U, D, E, I), (L, S, K, E))),
        # W = C + 5: three chunks (n = 2C + 3, two keys of the first), and the last two of four (n = 3C + 7)
        Case("win-linear-8", "window", dh, 2, 8, 1, 1, (2 * C + 2, 3 * C + 6), 3 * C + 7, C + 5, 0,
             ((L, S, U, D, E, I, P, I), (S, L, D, U, K, P, K, L))),
        # a ring of the smallest capacity W + T - 1 that has wrapped twice: sample 0's first row has lo at the last slot, sample
        # 1's four rows straddle the seam at 3C
        Case("win-ring-1", "window", dh, 2, 4, 4, 4, (3 * C + 1, 3 * C - 2), C + 2, C - 1, 1, ((U, D, E, K), (L, S, I, P))),
        # a ring with 7 slots to spare: sample 0 has lo at the last slot (n = 2C + 16), sample 1 wraps inside its window (n = 3C + 7)
        Case("win-ring-8", "window", dh, 2, 8, 1, 1, (2 * C + 15, 3 * C + 6), C + 12, C + 5, 1,
             ((S, L, K, U, D, K, P, L), (L, S, E, I, U, D, I, P))),
    ]


def all_cases():
    return [c for dh in DHS for c in _cases(dh)]


def case_id(c):
    return "%s-dh%d" % (c.name, c.dh)


# seed per case of all_cases(), found by search() below: the first seed at which every condition of
# tests/test_oracle_decode_rows.py holds and the correct replay is inside 0.6 of the bound
SEEDS = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0,
         0, 0, 0, 0, 0, 0, 0, 0, 0, 1)


def seed_of(case):
    return SEEDS[[case_id(c) for c in all_cases()].index(case_id(case))]


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def span(case, b, t, flaws=()):
    """(lo, n) of query (b, t): the positions [lo, n) it reads (adec_len and the window of the kernels)."""
    n = int(case.start[b]) + t + 1
    if not case.ring:
        n = min(n, case.cap)
    n = max(n, 0)
    if case.form != "window":
        return 0, n
    W = min(case.W, case.cap)
    if "lo_off_by_one" in flaws:
        return (n - W - 1 if n > W else 0), n
    return (n - W if n > W else 0), n


def chunks_of(case, lo, n):
    C = chunk(case.dh)
    return range(lo // C, (n - 1) // C + 1)


def peak_position(case, b, t, h, knoise):
    """`peaked`: the key of largest odd-coordinate norm of one chunk of the window - not the first where there are several, and
    another chunk for the neighbouring head."""
    lo, n = span(case, b, t)
    cs = list(chunks_of(case, lo, n))
    c = cs[0] if len(cs) == 1 else cs[1 + (h + b) % (len(cs) - 1)]
    C = chunk(case.dh)
    j = np.arange(max(lo, c * C), min(n, (c + 1) * C))
    return int(j[np.argmax((knoise[j].astype(np.float64) ** 2).sum(1))])


def beacon(which, dh):
    """(dh,) the beacon keys of `edge` on the odd coordinates, 0 elsewhere: 0 at lo - 1 (all +1), 1 at lo (+1, -1, ...), 2 at n - 1
    (all -1)."""
    out = np.zeros(dh, f32)
    n_odd = dh // 2
    out[1::2] = (np.ones(n_odd), np.where(np.arange(n_odd) % 2 == 0, 1.0, -1.0), -np.ones(n_odd))[which]
    return out


@functools.lru_cache(maxsize=None)
def build(case, seed=None):
    """dict(q (B*T, H*dh), kl / vl (B, Hkv, n_max, dh) the positions' contents, kc / vc (B, Hkv, cap, dh) the caches - NaN in every
    slot no position of the sample has reached - and start); everything read-only, q and k on the grid."""
    seed = seed_of(case) if seed is None else seed
    dh, B, H, Hkv, T, C = case.dh, case.B, case.H, case.Hkv, case.T, chunk(case.dh)
    R = H // Hkv
    a_ramp, a_const, const = LIFT[dh]
    n_max = max(case.start) + T
    odd = (np.arange(dh) % 2 == 1)
    kl = np.zeros((B, Hkv, n_max, dh), f32)
    kl[..., odd] = grid(K_NOISE * uniform(seed * 8 + 1, (B, Hkv, n_max, int(odd.sum()))))
    kl[..., 0::4] = ramp(np.arange(n_max), C)[None, None, :, None]
    kl[..., 2::4] = const
    vl = uniform(seed * 8 + 2, (B, Hkv, n_max, dh))
    knoise = kl[..., odd].copy()                 # `peaked` picks its key by the noise as drawn, before the beacons
    for b in range(B):                           # the beacons of a step's LAST row, in the kv heads that serve an edge head
        lo, n = span(case, b, T - 1)
        for kv in sorted({h // R for h in range(H) if case.kinds[b][h] in ("edge", "edge_in")}):
            for which, pos in ((0, lo - 1), (1, lo), (2, n - 1)):
                if pos >= 0:
                    kl[b, kv, pos] = np.where(odd, beacon(which, dh), kl[b, kv, pos])
    qn = grid(uniform(seed * 8 + 3, (B * T, H, dh)))
    q = np.zeros((B * T, H, dh), f32)
    for b in range(B):
        for t in range(T):
            lo, n = span(case, b, t)
            for h in range(H):
                kind, row = case.kinds[b][h], q[b * T + t, h]
                row[odd] = qn[b * T + t, h, odd]
                if kind in ("climbing", "falling"):
                    row[0::4] = a_ramp if kind == "climbing" else -a_ramp
                elif kind in ("lifted", "sunk"):
                    row[2::4] = a_const if kind == "lifted" else -a_const
                elif kind == "peaked":
                    row[:] = PEAK[dh] * np.where(odd, kl[b, h // R, peak_position(case, b, t, h, knoise[b, h // R])], 0)
                elif kind == "edge":
                    row[:] = PEAK[dh] * beacon(0, dh)
                elif kind == "edge_in":
                    row[:] = PEAK[dh] / 2 * (beacon(1, dh) + beacon(2, dh))
    q = q.reshape(B * T, H * dh)
    start = np.array(case.start, dtype=np.int32)
    if case.ring:
        kc, vc = WO.ring_image(kl, start + T, case.cap), WO.ring_image(vl, start + T, case.cap)
    else:
        kc, vc = (np.full((B, Hkv, case.cap, dh), np.nan, f32) for _ in range(2))
        for b in range(B):
            kc[b, :, :start[b] + T], vc[b, :, :start[b] + T] = kl[b, :, :start[b] + T], vl[b, :, :start[b] + T]
    assert np.array_equal(q, grid(q)) and np.array_equal(kl, grid(kl))
    out = dict(q=q, kl=kl, vl=vl, kc=kc, vc=vc, start=start, knoise=knoise)
    for a in out.values():
        a.setflags(write=False)
    return out


def kind_mask(case, kind):
    """(B*T, H*dh) bool: the outputs of the heads of `kind`."""
    m = np.zeros((case.B, case.T, case.H, case.dh), bool)
    for b in range(case.B):
        for h in range(case.H):
            m[b, :, h] = case.kinds[b][h] == kind
    return m.reshape(case.B * case.T, case.H * case.dh)


def kinds_in(case):
    return [k for k in KINDS if any(k in row for row in case.kinds)]


def slots(case, lo, n):
    return [WO.slot(p, case.cap, case.ring) for p in range(lo, n)]


# ---- the references --------------------------------------------------------------------------------------------------------------
def oracle(case, d, dt):
    """The f64 / f32 oracle of the case's form: tests/decode_oracle.py, gqa_oracle.py or window_oracle.py."""
    q, kc, vc = (d[n].astype(dt) for n in ("q", "kc", "vc"))
    sc = float(scale_of(case.dh))
    with np.errstate(invalid="ignore"):         # (the NaN tail is sliced off by the oracle, never read)
        if case.form == "plain":
            return DO.decode_forward(q, kc, vc, d["start"], case.T, sc)
        if case.form == "gqa":
            return GO.decode_forward_gqa(q, kc, vc, d["start"], case.T, case.H, sc)
        return WO.decode_forward(q, kc, vc, d["start"], case.T, case.W, bool(case.ring), H=case.H, scale=sc)


def raw_scores(case, d, b, t, h, lo, n):
    """The n - lo dot products of problem (b, t, h) in f64 (exact on the grid) and the slots they were read from."""
    sl = slots(case, lo, n)
    R = case.H // case.Hkv
    qr = d["q"][b * case.T + t, h * case.dh:(h + 1) * case.dh].astype(np.float64)
    return d["kc"][b, h // R, sl].astype(np.float64) @ qr, sl


def exponent_softmax(case, d):
    """The second plain f32 reference of the same operation: the full-row softmax in the exponent domain, s = f32(d * c1),
    p = exp2(s - max s), o = p . V / sum p.  No chunks, NumPy's own summation order."""
    dh, R = case.dh, case.H // case.Hkv
    out = np.zeros((case.B * case.T, case.H * dh), f32)
    for b in range(case.B):
        for t in range(case.T):
            lo, n = span(case, b, t)
            for h in range(case.H if n > 0 else 0):
                dots, sl = raw_scores(case, d, b, t, h, lo, n)
                s = dots.astype(f32) * c1_of(dh)
                p = np.exp2(s - s.max())
                out[b * case.T + t, h * dh:(h + 1) * dh] = (p @ d["vc"][b, h // R, sl]) / p.sum(dtype=f32)
    return out


def bound(want64, want32s, mask, vmax):
    """SURVEY 8c (ii) with err_cpu32 the larger of the two f32 references' errors: max(2 * err_cpu32, 1e-6 * yardstick), on the
    outputs `mask` selects.  Returns (bound, err_cpu32, the absolute term)."""
    err32 = max(float(np.abs(w[mask] - want64[mask]).max()) for w in want32s)
    floor = 1e-6 * max(float(np.abs(want64[mask]).max()), vmax)
    return max(2 * err32, floor), err32, floor


# ---- the kernels' arithmetic, restated ---------------------------------------------------------------------------------------------
def _exp2(x):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        p = np.exp2(np.asarray(x, f32))
    return np.where(p < TINY, f32(0), p).astype(f32)


def _fma(a, b, c):
    """One rounding: the f64 product of two f32 is exact."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _seq_sum(x):
    """((x[0] + x[1]) + x[2]) + ... along axis 0, every addition rounded to f32."""
    acc = x[0].astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(1, x.shape[0]):
            acc = (acc + x[i]).astype(f32)
    return acc


def _wave_sum(x):
    """nk_wave_sum: the xor butterfly over 64 lanes (offsets 32 .. 1); every lane ends with the same value."""
    x = x.astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        while x.shape[0] > 1:
            half = x.shape[0] // 2
            x = (x[:half] + x[half:]).astype(f32)
    return x[0]


def _partial(s, inw, v, dh, flaws, m_stale):
    """One block's pass over one chunk for one head: s (C,) f32 scores by position in the chunk (-inf outside the window), inw (C,)
    bool, v (C, dh) values (0 outside).  Returns (stored m, l, unnormalised o (dh,)).
    Vector kernels (nk_attention_decode_body.h): lane group g of G = 256 / (dh / 4) owns keys g, g + G, ... (16 of them); l and o are
    summed over a group's keys in order, then over the groups in order; a wave holds 64 / (dh / 4) groups.
    Generic kernels (nk_attention_decode_generic_body.h): one key per thread for the softmax (wave w holds keys 64w .. 64w + 63, l
    through nk_block_sum), o over a group's lpk keys in order, then over the G = 256 / lpk groups in order."""
    vector = dh in (32, 64, 128)
    C = s.shape[0]
    if vector:
        G = THREADS // (dh // 4)
        steps, wave_of_key = KPG, np.tile(np.arange(G) * (dh // 4) // 64, KPG)
    else:
        lpk = 1
        while lpk < 64 and lpk < dh:
            lpk *= 2
        G, steps, wave_of_key = THREADS // lpk, lpk, np.arange(C) // 64
    m_true = s[inw].max()
    m_key = np.full(C, m_true, f32)
    stored = m_true
    if "wave_local_max" in flaws:               # the LDS step left out: a wave's own maximum; thread 0 stores wave 0's
        wm = np.array([s[(wave_of_key == w)].max() for w in range(4)], f32)
        m_key, stored = wm[wave_of_key], wm[0]
    if m_stale is not None:
        m_key[:] = stored = m_stale
    if "no_shift" in flaws:
        m_key[:] = stored = f32(0)
    with np.errstate(invalid="ignore"):
        p = np.where(inw, _exp2(s - m_key), f32(0)).astype(f32)
    P, V = p.reshape(steps, G), v.reshape(steps, G, dh)
    acc = np.zeros((G, dh), f32)
    for i in range(steps):
        acc = _fma(P[i][:, None], V[i], acc)
    o = _seq_sum(acc)
    l = _seq_sum(_seq_sum(P)) if vector else _seq_sum(np.concatenate([[f32(0)], [_wave_sum(p[64 * w:64 * w + 64]) for w in range(4)]]))
    return f32(stored), f32(l), o


def _combine(parts, flaws):
    """nk_attention_decode_combine_body.h: M = max m_c, two fmas per chunk in ascending chunk order, o / l."""
    m = parts[0][0] if "combine_first_m" in flaws else max(pt[0] for pt in parts)
    o, l = np.zeros_like(parts[0][2]), f32(0)
    for mc, lc, oc in parts:
        with np.errstate(invalid="ignore"):
            f = f32(1) if "combine_no_rescale" in flaws else _exp2(f32(mc) - f32(m))
        o = _fma(oc, f, o)
        l = (f32(l) + lc).astype(f32) if "combine_l_unscaled" in flaws else _fma(lc, f, l)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (o / l).astype(f32)


def replay(q, kc, vc, start, T, H, Hkv, W, ring, flaws=()):
    """The device's arithmetic for nk_attention_decode_fwd (W = 0, Hkv == H), _gqa_fwd (W = 0) and _window_fwd (W > 0) on caches
    (B, Hkv, cap, dh): chunks of `chunk(dh)` keys aligned to absolute positions, the in-window selection, exp2(s - m) with results
    below 2^-126 flushed, the groups in order, the combine's two fmas per chunk in ascending chunk order.  -> (B*T, H*dh) f32.
    flaws (FLAWS): "no_shift" a partial without a shift (m = 0 in the exponent and in the workspace); "wave_local_max" a wave's
    groups use their own maximum; "stale_head_max" head hq > 0 of a block of the grouped vector kernels keeps head 0's m;
    "combine_first_m" the combine shifts by the first chunk's m; "combine_no_rescale" it adds the partials as they are;
    "combine_l_unscaled" it rescales o and not l; "lo_off_by_one" the window starts one key early."""
    flaws = set(flaws)
    assert flaws <= set(FLAWS)
    B, _, cap, dh = kc.shape
    form = "window" if W else ("gqa" if Hkv != H else "plain")
    case = Case("replay", form, dh, B, H, Hkv, T, tuple(int(s) for s in start), cap, W, ring, None)
    d = dict(q=q, kc=kc, vc=vc)
    C, R, c1 = chunk(dh), H // Hkv, c1_of(dh)
    batched = dh in (32, 64, 128) and R > 1      # the grouped vector kernels: blocks of at most 8 heads of a group
    out = np.zeros((B * T, H * dh), f32)

    def scores(b, t, h, lo, n):
        dots, sl = raw_scores(case, d, b, t, h, lo, n)
        assert np.array_equal(dots, dots.astype(f32))
        return dots.astype(f32) * c1, sl

    for b in range(B):
        for t in range(T):
            lo, n = span(case, b, t, flaws)
            if n <= 0:
                continue
            for h in range(H):
                s_all, sl = scores(b, t, h, lo, n)
                head0 = h - (h % R) % GQA_HEADS
                stale = "stale_head_max" in flaws and batched and head0 != h
                s0_all = scores(b, t, head0, lo, n)[0] if stale else None
                v_all = vc[b, h // R, sl].astype(f32)
                parts = []
                for c in chunks_of(case, lo, n):
                    j0, j1 = max(lo, c * C), min(n, (c + 1) * C)
                    s, inw, v = np.full(C, -np.inf, f32), np.zeros(C, bool), np.zeros((C, dh), f32)
                    s[j0 - c * C:j1 - c * C], inw[j0 - c * C:j1 - c * C] = s_all[j0 - lo:j1 - lo], True
                    v[j0 - c * C:j1 - c * C] = v_all[j0 - lo:j1 - lo]
                    parts.append(_partial(s, inw, v, dh, flaws, s0_all[j0 - lo:j1 - lo].max() if stale else None))
                if len(parts) == 1:              # a problem of one chunk writes O directly
                    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                        res = (parts[0][2] / parts[0][1]).astype(f32)
                else:
                    res = _combine(parts, flaws)
                out[b * T + t, h * dh:(h + 1) * dh] = res
    return out


def replay_case(case, d, flaws=()):
    return replay(d["q"], d["kc"], d["vc"], d["start"], case.T, case.H, case.Hkv, case.W if case.form == "window" else 0, case.ring, flaws)


# ---- what the CPU file asserts, and the seed search ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def evaluate(case, seed=None):
    """Everything about a case that needs no GPU, computed once: inputs, the f64 oracle, the two f32 references, the correct
    replay, and err / bound of the replay per kind.  Read-only."""
    d = build(case, seed)
    ref, ref32, ref32e = oracle(case, d, np.float64), oracle(case, d, np.float32), exponent_softmax(case, d)
    rep = replay_case(case, d)
    vmax = float(np.abs(d["vl"]).max())
    ratios = {}
    for kind in kinds_in(case):
        m = kind_mask(case, kind)
        ratios[kind] = float(np.abs(rep[m] - ref[m]).max()) / bound(ref, (ref32, ref32e), m, vmax)[0]
    for a in (ref, ref32, ref32e, rep):
        a.setflags(write=False)
    return dict(d=d, ref=ref, ref32=ref32, ref32e=ref32e, replay=rep, vmax=vmax, ratios=ratios)


def log2_scores(case, d, b, t, h):
    """(positions lo .. n - 1, their f64 scores in the exponent domain) of problem (b, t, h)."""
    lo, n = span(case, b, t)
    dots, _ = raw_scores(case, d, b, t, h, lo, n)
    return np.arange(lo, n), dots * np.float64(c1_of(case.dh))


def chunk_maxima(case, pos, sc2):
    C = chunk(case.dh)
    return np.array([sc2[pos // C == c].max() for c in np.unique(pos // C)])


def conditions(case, seed=None):
    """The properties a kind is built for, as a list of failures (empty: all hold).  For climbing / falling problems of three or
    more chunks the chunk maxima span more than SPREAD and are monotonic; every lifted / sunk score is beyond +-SPREAD; a peaked
    row has its maximum at `peak_position`; an edge row's beacon at lo - 1, where the cache still holds it, is above every score
    of the window by more than 4."""
    d, bad = build(case, seed), []
    R = case.H // case.Hkv
    for b in range(case.B):
        for t in range(case.T):
            for h in range(case.H):
                kind, (lo, n) = case.kinds[b][h], span(case, b, t)
                pos, sc2 = log2_scores(case, d, b, t, h)
                cm = chunk_maxima(case, pos, sc2)
                where = (case_id(case), b, t, h, kind)
                if kind in ("climbing", "falling") and len(cm) >= 3:
                    step = np.diff(cm) if kind == "climbing" else -np.diff(cm)
                    if not (cm.max() - cm.min() > SPREAD and (step > 0).all()):
                        bad.append(where + (cm,))
                if kind in ("lifted", "sunk") and not ((sc2 > SPREAD).all() if kind == "lifted" else (sc2 < -SPREAD).all()):
                    bad.append(where + (sc2.min(), sc2.max()))
                if kind == "plain" and not np.abs(sc2).max() < 4.0:
                    bad.append(where + (np.abs(sc2).max(),))
                if kind == "peaked":
                    # dh 5 has two odd coordinates on a grid of 13 values: other keys may tie with the chosen one, and where its
                    # chunk holds only a key or two of the window (n = kC + 1) there is no large one to choose
                    pk = peak_position(case, b, t, h, d["knoise"][b, h // R])
                    few = case.dh == 5 and (pos // chunk(case.dh) == pk // chunk(case.dh)).sum() < 16
                    if not few and (sc2[pk - lo] != sc2.max() or (case.dh >= 20 and (sc2 == sc2.max()).sum() != 1)):
                        bad.append(where + (pk, int(pos[np.argmax(sc2)])))
                if kind == "edge" and t == case.T - 1 and lo >= 1:
                    out = float(d["kl"][b, h // R, lo - 1].astype(np.float64) @ d["q"][b * case.T + t, h * case.dh:(h + 1) * case.dh]
                                * np.float64(c1_of(case.dh)))
                    held = not case.ring or lo - 1 >= int(case.start[b]) + case.T - case.cap     # the ring still holds lo - 1
                    if not (held and out > sc2.max() + 4.0):
                        bad.append(where + (held, out, sc2.max()))
                if kind == "edge_in" and t == case.T - 1 and lo >= 1 and not {int(pos[i]) for i in np.argsort(sc2)[-2:]} == {lo, n - 1}:
                    bad.append(where + (pos[np.argsort(sc2)[-2:]],))
    return bad


def search(tries=32, limit=0.6):
    """The SEEDS table: per case the first seed at which `conditions` holds and the correct replay is inside `limit` of the bound
    for every kind.  Prints it."""
    chosen = []
    for case in all_cases():
        for seed in range(tries):
            if not conditions(case, seed) and max(evaluate(case, seed)["ratios"].values()) <= limit:
                chosen.append(seed)
                break
        else:
            raise RuntimeError("no seed for %s" % case_id(case))
    print("SEEDS = (%s)" % ", ".join(map(str, chosen)))
    return tuple(chosen)
