"""Logit rows that move the running maximum of the cross-entropy kernels (nk_cross_entropy.h), and a NumPy replay of their forward
arithmetic.

lse = m + log(sum exp(x - m)) has the same value for ANY m as long as no exp(x - m) overflows (x - m > 88.72) and not all of them
flush to zero (x - m < -103.28).  Every other cross-entropy test draws its logits from N(0, 3^2) or N(0, 2^2): a row's maximum and
minimum lie about 25 apart, so a maximum folded over the wrong set of columns, a merge against a stale maximum, a fold that starts
from 0 or no shift at all read correct values there.  The row kinds here (`kinds_of`) do not.

Exact logits.  Every finite logit is a multiple of 1/8 with |x| <= 8192 (`masked_1e9` is the stated exception): x - m and every
difference of two levels is exact in f32, so the replay and the device see the same exponents.  `base` is N(0, 3^2) rounded to 1/8
and clipped to [-8, 8]: two columns of neighbouring levels are at least GAP - 16 = 96 apart and at most GAP + 16.

Kinds, one row per kind in every call of a case:
    plain            base: the control
    climbing         base + GAP * level(c); level rises by one per step of the running index of the row's own family - row<V>: each i
                     of v[i] (256 body columns); block<NT>: each slot (NT quads), so every ce_online call of every thread rescales
                     by exp(-(96 .. 128)); generic: each ceil(C / 8) columns.  The edge elements (head and tail scalars), which
                     the kernels fold last, take one level more than the last slot
    falling          base - GAP * level(c): the maximum is in the first slot, everything later underflows in the lane and in both
                     merges
    lifted / sunk    base +- 8 GAP: without a shift, or with a fold that starts from 0, the whole row overflows / flushes
    peaked:<role>    base with ONE column raised to max(base) + GAP, chosen by its role in the walk (`role_col`): head, tail,
                     last_quad (row kernels: the highest v[i] in use, the lanes beyond it idle), slot3 (slot u = 3 of a full trip of
                     a block kernel), partial (a quad of the partial trip), edge_after_body (the edge element of thread 0 or 32),
                     last_wave (owner thread >= NT - 64), wave0 (owner thread < 64)
    masked_inf       ~90% of the classes are -inf, in whole groups of four quads, so that full trips have a group maximum of -inf and
                     lanes keep m = f32::MIN; live classes remain in the head, in the tail and in one quad of the last wave
    masked_min       the same mask with finfo(f32).min: a lane that sees nothing else has m = f32::MIN and s = its COUNT, which must
                     vanish in the merge
    masked_1e9       the same mask with -1e9 (not on the 1/8 grid)
A role that a geometry does not have (no head on an aligned row, no full trip at nb <= 3 NT, one level only) leaves its row `plain` and unlabelled
(kind None) in that call.  Targets: `tA` on the row's maximum, `tB` on its lowest live class (at least GAP below the maximum on the
climbing, falling and peaked kinds: a large finite loss and dx_t close to -g w); on masked kinds always a live class.  `extra_row`
is the masked_inf row with its target on a -inf class (loss = +inf), for the comparison with the composed device path alone.

Bounds.  cross_entropy_oracle.bounds(C, xmax, ...) with xmax the largest |logit| among the row's LIVE classes (> -1e8): a masked
class contributes exp(.) = 0 exactly, to lse and to dx, and carries no rounding; the row's own xmax is never larger than the call's,
so this is the oracle's bound at its tightest honest argument.

`replay` restates each family's forward in f32 NumPy; `flaws` switches on wrong behaviours (FLAWS), the idiom of
tests/decode_rows.py.  CASES are the committed shapes, shared by the CPU and the GPU file."""
import collections
import functools

import numpy as np

import cross_entropy_oracle as X

f32 = np.float32
F32_MIN = np.finfo(np.float32).min

# exp(GAP) overflows f32 (ln(f32 max) = 88.72) and exp(-GAP) is 0 even with denormals (ln(2^-149) = -103.28); 104 would clear both
# but the base noise spans 16, and levels must stay on the 1/8 grid whatever the count: 112 is the first multiple of 8 that clears
# both limits, and GAP - 16 = 96 still overflows while exp(-96) < 2^-138 is beyond the last bit of any sum >= 1
GAP = 112.0
LN_F32_MAX, LN_F32_DENORM_MIN = 88.72, -103.28
NOISE = 8.0
LIVE_ABOVE = -1e8

ROW_MAX, BLOCK_512, BLOCK_1024, EDGE_TAIL = 2048, 16384, 65536, 32       # nk_cross_entropy.h: CE_ROW_MAX, CE_BLOCK_*, CE_EDGE_TAIL
ROW_V = ((256, 1), (512, 2), (1024, 4), (2048, 8))                          # the host's C <= limit -> row<V>

FAMILIES = ("row1", "row2", "row4", "row8", "block256", "block512", "block1024", "generic")
BASE_KINDS = ("plain", "climbing", "falling", "lifted", "sunk")
MASKED = {"masked_inf": -np.inf, "masked_min": F32_MIN, "masked_1e9": -1e9}
ROW_ROLES = ("head", "tail", "last_quad")
BLOCK_ROLES = ("head", "tail", "slot3", "partial", "edge_after_body", "last_wave", "wave0")
SPREAD_KINDS = ("climbing", "falling")

FLAWS = ("max_skips_edge", "group_max_of_three", "partial_trip_no_online", "edge_no_online", "wave_merge_first_lane_m",
         "block_merge_first_wave_m", "fold_from_zero", "no_shift", "no_rescale")
# the flaws that are a different - but consistent - shift: invisible wherever nothing overflows or underflows
SHIFT_FLAWS = tuple(f for f in FLAWS if f != "no_rescale")
ROW_FLAWS = ("max_skips_edge", "wave_merge_first_lane_m", "fold_from_zero", "no_shift")
BLOCK_FLAWS = ("group_max_of_three", "partial_trip_no_online", "edge_no_online", "wave_merge_first_lane_m", "block_merge_first_wave_m",
               "fold_from_zero", "no_shift", "no_rescale")
GENERIC_FLAWS = ("fold_from_zero", "no_shift")


def flaws_of(fam):
    """The flaws that exist in a family's kernel: the row kernels are two-pass (nothing to rescale, no trips), the generic ones have
    no lanes to merge."""
    return GENERIC_FLAWS if fam == "generic" else ROW_FLAWS if fam.startswith("row") else BLOCK_FLAWS


# ---- the walk, restated ------------------------------------------------------------------------------------------------------------
def family(C, inner, together=True):
    """the dispatch rule of include/neuronika_hip.h, restated"""
    if inner > 1 or not together:
        return "generic"
    if C <= ROW_MAX:
        return "row%d" % next(v for limit, v in ROW_V if C <= limit)
    return "block%d" % (256 if C <= BLOCK_512 else 512 if C <= BLOCK_1024 else 1024)


def walk(C, off):
    """ce_walk_of: (head, nb, tail) of a row of C floats that starts `off` floats past a 16-byte boundary"""
    head = min((4 - off) & 3, C)
    nb = (C - head) >> 2
    return head, nb, C - head - 4 * nb


def threads_of(fam):
    """the width of the unit that walks a row: a wave for row<V>, the block for block<NT>"""
    return 64 if fam.startswith("row") else int(fam[5:])


def full_trips(NT, nb, tid):
    """how often thread `tid` of a block kernel runs its four-quad loop: the j >= 0 with tid + 4 NT j + 3 NT < nb"""
    tid = np.asarray(tid)
    return np.maximum(0, -((3 * NT + tid - nb) // (4 * NT)))


Owner = collections.namedtuple("Owner", "edge thread slot trip u full")


def ownership(fam, C, off):
    """Per column, as arrays (C,): edge (0 body, 1 head, 2 tail), the owner thread (lane for a row kernel), the slot (the running
    index of the owner's quads: v[i] of a row kernel, q / NT of a block kernel; -1 on an edge element), the trip and u = slot / 4
    and slot % 4, and whether that trip is one of the owner's FULL trips (block kernels; otherwise the partial trip)."""
    NT = threads_of(fam)
    head, nb, tail = walk(C, off)
    c = np.arange(C)
    edge = np.where(c < head, 1, np.where(c >= head + 4 * nb, 2, 0))
    qd = (c - head) // 4
    thread = np.where(edge == 1, c, np.where(edge == 2, EDGE_TAIL + c - head - 4 * nb, qd % NT))
    slot = np.where(edge == 0, qd // NT, -1)
    full = (edge == 0) & (slot // 4 < full_trips(NT, nb, thread)) & fam.startswith("block")
    return Owner(edge, thread, slot, slot // 4, slot % 4, full)


def level(fam, C, off):
    """(C,) the level of `climbing` / `falling` per column"""
    if fam == "generic":
        return np.arange(C) // -(-C // 8)
    NT = threads_of(fam)
    own = ownership(fam, C, off)
    nb = walk(C, off)[1]
    return np.where(own.edge == 0, own.slot, -(-nb // NT))


def role_col(fam, C, off, role):
    """The column with `role` in the walk of a row at offset `off`, or None where the geometry has none."""
    if fam == "generic":
        return None
    NT = threads_of(fam)
    head, nb, tail = walk(C, off)
    block = fam.startswith("block")
    if role == "head":
        return head - 1 if head else None
    if role == "tail":
        return C - 1 if tail else None
    if role == "last_quad":
        return head + 4 * (nb - 1) + 2 if nb and not block else None
    if not block:
        return None
    if role == "edge_after_body":
        return 0 if head else (head + 4 * nb if tail else None)
    if role == "slot3":
        qd = 3 * NT + 5
        return head + 4 * qd + 1 if qd < nb else None
    if role == "partial":
        own = ownership(fam, C, off)
        part = np.flatnonzero((own.edge == 0) & ~own.full)
        return int(part[-1]) - 1 if part.size else None
    if role == "last_wave":
        qd = 2 * NT - 1 if 2 * NT - 1 < nb else NT - 1
        return head + 4 * qd + 3 if qd < nb else None
    if role == "wave0":
        qd = NT + 3 if NT + 3 < nb else 3
        return head + 4 * qd if qd < nb else None
    raise ValueError(role)


def _tenth(n, rng):
    """(n,) bool with round(n / 10) entries set, none below 8"""
    out = np.zeros(n, bool)
    out[rng.choice(n, int(round(n / 10.0)), replace=False)] = True
    return out


def live_mask(fam, C, off, rng):
    """(C,) bool, the classes a masked kind keeps: ~10% of the groups of four quads (16 columns), the head, the tail and one quad of
    the last wave (row kernels: the last quad)."""
    if fam == "generic":
        live = np.repeat(_tenth(-(-C // 16), rng), 16)[:C]
        live[0] = live[C - 1] = True
        return live
    head, nb, tail = walk(C, off)
    live = np.zeros(C, bool)
    live[:head] = True
    live[head + 4 * nb:] = True
    live[head:head + 4 * nb] = np.repeat(_tenth(-(-nb // 4), rng), 16)[:4 * nb]
    keep = role_col(fam, C, off, "last_wave" if fam.startswith("block") else "last_quad")
    if keep is not None and (nb >= 2 or head + tail == 0):      # (a row of one quad between a head and a tail: the quad is masked)
        q0 = head + 4 * ((keep - head) // 4)
        live[q0:q0 + 4] = True
    return live


# ---- the committed cases ---------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "C inner")
CASES = tuple(Case(C, 1) for C in (10, 255, 256, 300, 601, 1100, 2048, 2049, 4099, 9001, 16385, 20000, 65537, 70001)) + (Case(12, 5), Case(300, 7))
LEADS = (4, 5, 6, 7)
MISALIGNED_PAIR = (300, 9001)          # x at lead 4, dx at lead 5: the backward goes generic, the forward does not


def case_id(case):
    return "C%d" % case.C if case.inner == 1 else "C%dx%d" % case


def kinds_of(fam):
    roles = () if fam == "generic" else BLOCK_ROLES if fam.startswith("block") else ROW_ROLES
    return BASE_KINDS + tuple("peaked:" + r for r in roles) + tuple(MASKED)


def base_row(C, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.round(rng.standard_normal(C) * 3.0 * 8.0) / 8.0, -NOISE, NOISE).astype(f32)


def make_row(kind, fam, C, off, seed):
    """-> (row (C,) f32, live (C,) bool, the raised column or -1), or None where the kind's role does not exist at this offset."""
    base, live, col = base_row(C, seed), np.ones(C, bool), -1
    if kind == "plain":
        x = base
    elif kind in SPREAD_KINDS:
        if level(fam, C, off).max() == 0:           # one v[i] and no edge element (C = 256, aligned): nothing to climb
            return None
        x = base + f32(GAP if kind == "climbing" else -GAP) * level(fam, C, off).astype(f32)
    elif kind in ("lifted", "sunk"):
        x = base + f32(8 * GAP if kind == "lifted" else -8 * GAP)
    elif kind.startswith("peaked:"):
        col = role_col(fam, C, off, kind[7:])
        if col is None:
            return None
        x = base.copy()
        x[col] = base.max() + f32(GAP)
    else:
        live = live_mask(fam, C, off, np.random.default_rng(seed + 7919))
        x = np.where(live, base, f32(MASKED[kind])).astype(f32)
    return x.astype(f32), live, col


@functools.lru_cache(maxsize=None)
def build(case, lead=4):
    """One call of a case: dict(x (P, C) the rows by position, kinds (P,) - None on a filler -, offs, live (P, C), cols, tA, tB,
    extra_row, extra_target, fam).  Position p of the call is row n = p / inner, r = p % inner (`as_call`).  Read-only."""
    C, inner = case
    fam = family(C, inner)
    kinds = list(kinds_of(fam))
    P = -(-len(kinds) // inner) * inner
    kinds += [None] * (P - len(kinds))
    x, live, cols, offs = np.zeros((P, C), f32), np.ones((P, C), bool), [], []
    for p, kind in enumerate(kinds):
        off = (lead + p * C) % 4 if inner == 1 else 0
        made = make_row(kind, fam, C, off, C * 64 + p) if kind else None
        if made is None:
            kinds[p], made = None, make_row("plain", fam, C, off, C * 64 + p)
        x[p], live[p] = made[0], made[1]
        cols.append(made[2])
        offs.append(off)
    finite = np.isfinite(x) & (np.abs(x) <= 8192)
    assert np.array_equal(x[finite] * 8, np.round(x[finite] * 8)) and (finite | ~live).all()
    tA = np.where(live, x, -np.inf).argmax(1).astype(f32)
    tB = np.where(live, x, np.inf).argmin(1).astype(f32)
    p_inf = kinds.index("masked_inf")
    out = dict(x=x, kinds=tuple(kinds), offs=tuple(offs), live=live, cols=tuple(cols), tA=tA, tB=tB, fam=fam, extra_row=x[p_inf].copy(),
               extra_target=f32(np.flatnonzero(~live[p_inf])[0]))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def as_call(rows, inner):
    """(P, C) rows by position -> the logits of the call: (P, C), or (P / inner, C, inner)"""
    if inner == 1:
        return np.ascontiguousarray(rows)
    P, C = rows.shape
    return np.ascontiguousarray(rows.reshape(P // inner, inner, C).transpose(0, 2, 1))


def as_rows(call, inner):
    """the inverse of as_call"""
    if inner == 1:
        return call
    N, C, _ = call.shape
    return call.transpose(0, 2, 1).reshape(N * inner, C)


def as_targets(t, inner):
    return t if inner == 1 else t.reshape(-1, inner)


def grid_finite(d):
    """the positions whose row holds no mask value: what a label-smoothed call may contain (the mean of the logits is finite)"""
    return np.array([k is None or k not in MASKED for k in d["kinds"]])


def row_xmax(x_row):
    """max |logit| among the live classes of a row (module docstring, Bounds)"""
    return float(np.abs(x_row[x_row > LIVE_ABOVE]).max())


# ---- references --------------------------------------------------------------------------------------------------------------------
def oracle_row(x_row, t):
    """(lse, dx row for g w = 1) in f64"""
    lse = X.pieces(x_row[None, :], np.array([t], f32))[0]
    return float(lse[0, 0]), X.backward(x_row[None, :], np.array([t], f32), lse, 1.0, "sum")[0]


def two_pass32(x_row, t):
    """the plain f32 two-pass reference: m = max, sum(exp(x - m)) in f32 (NumPy's own order), dx = exp(x - lse) - onehot"""
    x_row = x_row.astype(f32)
    with np.errstate(all="ignore"):
        m = np.maximum(x_row.max(), f32(F32_MIN))
        lse = f32(m + np.log(np.exp(x_row - m).sum(dtype=f32)))
        dx = np.exp(x_row - lse)
    dx[int(t)] -= f32(1)
    return lse, dx


# ---- the kernels' forward arithmetic, restated -----------------------------------------------------------------------------------------
def _exp(v):
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(v, f32)).astype(f32)


def _sub(a, b):
    with np.errstate(all="ignore"):
        return (np.asarray(a, f32) - np.asarray(b, f32)).astype(f32)


def _expsum4(r, m):
    """ce_expsum4 on quads r (n, 4) with shifts m (n,)"""
    e = _exp(_sub(r, np.asarray(m, f32)[:, None]))
    with np.errstate(all="ignore"):
        return ((e[:, 0] + e[:, 1]) + (e[:, 2] + e[:, 3])).astype(f32)


def _wave_sum(v):
    """nk_wave_sum: the xor butterfly over 64 lanes (offsets 32 .. 1)"""
    v = v.astype(f32)
    with np.errstate(all="ignore"):
        while v.shape[0] > 1:
            half = v.shape[0] // 2
            v = (v[:half] + v[half:]).astype(f32)
    return v[0]


def _finish(m, s):
    with np.errstate(all="ignore"):
        return f32(f32(m) + np.log(f32(s)))


def _quads(x_row, off, NT):
    """the body as (K, NT, 4) by slot and thread, valid (K, NT), and the edge values / validity per thread"""
    C = x_row.shape[0]
    head, nb, tail = walk(C, off)
    K = max(1, -(-nb // NT))
    body = np.zeros((K * NT, 4), f32)
    body[:nb] = x_row[head:head + 4 * nb].reshape(nb, 4)
    valid = (np.arange(K * NT) < nb).reshape(K, NT)
    e, has_e = np.zeros(NT, f32), np.zeros(NT, bool)
    e[:head], has_e[:head] = x_row[:head], True
    e[EDGE_TAIL:EDGE_TAIL + tail], has_e[EDGE_TAIL:EDGE_TAIL + tail] = x_row[head + 4 * nb:], True
    return body.reshape(K, NT, 4), valid, e, has_e, nb


def _replay_row(x_row, off, V, flaws):
    """ce_fwd_row_kernel<V>: the row in registers, the maximum by a wave fold, then the sum under that one shift"""
    q, valid, e, has_e, nb = _quads(x_row, off, 64)
    assert q.shape[0] <= V
    start = f32(0) if "fold_from_zero" in flaws else f32(F32_MIN)
    m = np.full(64, start, f32)
    if "max_skips_edge" not in flaws:
        m = np.where(has_e, np.maximum(m, e), m)
    for i in range(q.shape[0]):
        m = np.where(valid[i], np.maximum(m, q[i].max(1)), m)
    mw = m[0] if "wave_merge_first_lane_m" in flaws else m.max()
    if "no_shift" in flaws:
        mw = f32(0)
    s = np.where(has_e, _exp(_sub(e, mw)), f32(0)).astype(f32)
    with np.errstate(all="ignore"):
        for i in range(q.shape[0]):
            s = np.where(valid[i], s + _expsum4(q[i], np.full(64, mw, f32)), s).astype(f32)
    return _finish(mw, _wave_sum(s))


def _replay_block(x_row, off, NT, flaws):
    """ce_fwd_block_kernel<NT>: a running (m, s) per lane over full trips of four quads, the partial trip quad by quad and the edge
    element last; merged per wave (nk_wave_max, s exp(m - wm), nk_wave_sum) and by thread 0 over the waves through LDS"""
    q, valid, e, has_e, nb = _quads(x_row, off, NT)
    tid = np.arange(NT)
    F = full_trips(NT, nb, tid)
    shift = "no_shift" not in flaws
    m = np.full(NT, f32(0) if ("fold_from_zero" in flaws or not shift) else f32(F32_MIN), f32)
    s = np.zeros(NT, f32)

    def online(m, s, cm, on, rescale=True):
        if not shift:
            return m, s
        mn = np.maximum(m, cm)
        with np.errstate(all="ignore"):
            if rescale and "no_rescale" not in flaws:
                s = np.where(on, s * _exp(_sub(m, mn)), s).astype(f32)
        return np.where(on, mn, m).astype(f32), s

    def add(m, s, r, on):
        with np.errstate(all="ignore"):
            return np.where(on, s + _expsum4(r, m), s).astype(f32)

    K = q.shape[0]
    for j in range(-(-K // 4)):
        qs = [q[4 * j + u] if 4 * j + u < K else np.zeros((NT, 4), f32) for u in range(4)]
        vs = [valid[4 * j + u] if 4 * j + u < K else np.zeros(NT, bool) for u in range(4)]
        full = j < F
        group = qs[:3] if "group_max_of_three" in flaws else qs
        m, s = online(m, s, np.max([g.max(1) for g in group], axis=0), full)
        for u in range(4):
            s = add(m, s, qs[u], full)
        part = j == F
        # "partial_trip_no_online" spares a lane without a full trip: there m is still f32::MIN and exp(x - m) overflows on ANY data
        skip = "partial_trip_no_online" in flaws
        for u in range(4):
            on = part & vs[u]
            m, s = online(m, s, qs[u].max(1), on & ~(skip & (F > 0)))
            s = add(m, s, qs[u], on)
    if "edge_no_online" not in flaws:
        m, s = online(m, s, e, has_e)
    with np.errstate(all="ignore"):
        s = np.where(has_e, s + _exp(_sub(e, m)), s).astype(f32)
    W = NT // 64
    mw, sw = m.reshape(W, 64), s.reshape(W, 64)
    wm = mw[:, 0].copy() if "wave_merge_first_lane_m" in flaws else mw.max(1)
    with np.errstate(all="ignore"):
        red1 = np.array([_wave_sum((sw[w] * _exp(_sub(mw[w], wm[w]))).astype(f32)) for w in range(W)], f32)
    bm = wm[0] if "block_merge_first_wave_m" in flaws else wm.max()
    bs = f32(0)
    with np.errstate(all="ignore"):
        for w in range(W):
            bs = f32(bs + f32(red1[w] * _exp(_sub(wm[w], bm))))
    return _finish(bm, bs)


def _replay_generic(x_row, flaws):
    """ce_fwd_generic_kernel: a sequential maximum from f32::MIN, then a sequential sum"""
    m = f32(0) if "fold_from_zero" in flaws else f32(F32_MIN)
    m = f32(0) if "no_shift" in flaws else np.maximum(m, x_row.max())
    with np.errstate(all="ignore"):
        s = np.cumsum(_exp(_sub(x_row, m)), dtype=f32)[-1]
    return _finish(m, s)


def replay(x_row, off, fam, flaws=()):
    """lse of one row as the family's forward kernel computes it, in f32 NumPy: lane ownership, trip order, ce_online, the wave merge
    and the block merge.  flaws (FLAWS; a flaw the family's kernel cannot have is ignored):
    "max_skips_edge" the row kernels leave the head / tail scalars out of m; "group_max_of_three" a full trip's group maximum is
    taken over three of its four quads; "partial_trip_no_online" a lane that has run a full trip adds its partial trip under the m
    it has; "edge_no_online" the edge element is added under the m the body left; "wave_merge_first_lane_m" the wave's shift is
    lane 0's m; "block_merge_first_wave_m" the block's shift is red[0][0]; "fold_from_zero" the max fold starts from 0;
    "no_shift" m = 0 throughout; "no_rescale" ce_online moves m and leaves s as it is."""
    flaws = set(flaws)
    assert flaws <= set(FLAWS)
    flaws &= set(flaws_of(fam))
    x_row = np.asarray(x_row, f32)
    if fam == "generic":
        return _replay_generic(x_row, flaws)
    if fam.startswith("row"):
        return _replay_row(x_row, off, int(fam[3:]), flaws)
    return _replay_block(x_row, off, threads_of(fam), flaws)


def ratio(got, want, bound):
    """err / bound; inf for a non-finite result"""
    return float(abs(float(got) - want) / bound) if np.isfinite(got) else float("inf")


@functools.lru_cache(maxsize=None)
def evaluate(case, lead=4):
    """Everything about one call that needs no GPU, per position: lse64, the correct replay, the two-pass f32 reference (lse and dx
    under both targets), the per-row bounds (g w = 1), and the ratios err / bound of the replay and the reference.  Read-only."""
    d = build(case, lead)
    C, fam, rows = case.C, d["fam"], []
    for p, kind in enumerate(d["kinds"]):
        xr = d["x"][p]
        b = X.bounds(C, row_xmax(xr), 1)
        r = dict(kind=kind, bounds=b, replay=replay(xr, d["offs"][p], fam))
        for name in ("tA", "tB"):
            t = d[name][p]
            lse64, dx64 = oracle_row(xr, t)
            lse32, dx32 = two_pass32(xr, t)
            r.update(lse64=lse64, lse32=lse32)
            r["dx64_" + name], r["dx32_err_" + name] = dx64, float(np.abs(dx32 - dx64).max())
        r["lse32_err"] = abs(float(r["lse32"]) - r["lse64"])
        rows.append(r)
    return dict(d=d, rows=rows)
