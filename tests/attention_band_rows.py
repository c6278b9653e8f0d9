"""tests/attention_rows.py's score rows under a MOVING LEFT EDGE: the sliding-window and the packed-sequence kernels (the two forms
of nk_attention_band.h's attention_band_kernel, tile body nk_attention_tile.h) carry their own compiled
copies of the online-softmax tile body, each included twice (edge tiles, whole tiles), and every other test of them draws q and k from
uniform [-1, 1): the lazy shift then moves in a row's first finite tile only, where the running sum and the accumulator are 0.

Row kinds.  `plain`, `climbing`, `falling`, `mixed` and `shifted` are attention_rows.rows as they are (q and k on the 1/8 grid: raw
scores exact in f32 in any summation order).  `under` is not carried over: its lifted tile is an absolute position, which means
nothing under a sliding left edge, and the 6.0 threshold is pinned on the causal copy.  Added here:
  peaked_in  `peaked` with the peak among the row's OWN visible keys and never in its first visible tile
  handover   (packed sequences) documents alternate between `climbing` and `low` - q and k carry `shifted`'s common offset with the
             opposite sign, every score ~48 nats down - so that the two halves of a wave that straddles a document boundary sit tens
             of nats apart; `orient` swaps the roles, and a layout with two boundaries has both orientations at once

What differs from the causal walk: a row's first finite tile is the tile of its own left edge, not tile 0; rows late in a wave sit at
m = -1e30 over all--inf tiles while an earlier row moves the shift (alpha = exp2(0) = 1 on a zero sum); a wave's rows start in up to
two different tiles, so a row is CARRIED by a neighbour's first finite tile even on uniform data (`settled_max`).

`replay_forward` is attention_rows.replay_forward with the band / seg walk; one walk serves both kernels, since the band kernel's
bounds are the seg kernel's at lo[r] = max(0, r - W + 1) (`segment_oracle.band_lo`)."""
import functools

import numpy as np

from oracle import neuronika_oracle as O
import attention_rows as R
import segment_oracle as SO

f32 = np.float32

BASE = ("plain", "climbing", "falling", "mixed", "shifted")
BAND_KINDS = BASE + ("peaked_in",)
SEG_KINDS = BASE + ("peaked_in", "handover")
MOVING = ("climbing", "mixed", "peaked_in", "handover")    # some row passes the test by itself after its first finite tile
STILL = ("plain", "falling")                               # none does
CLASSES = ("left", "whole", "diag")                        # left-edge tile, whole tile [left_end, 4 qb), diagonal square

# (B, S, H, dh, W): the smallest that reach every (dh, ragged) pair with both tile bodies
BAND = [(1, 256, 2, 64, 176),      # whole tile 3 of block 1
        (1, 384, 1, 64, 100),      # kt0 > 0 in block 2 (not W = 96: there one `falling` row whose first visible tile holds a
                                   # single, low key passes the test by itself in its second tile - a control that moves)
        (2, 197, 2, 64, 40),       # dh 64 ragged
        (2, 160, 2, 32, 40),       # dh 32 whole
        (1, 129, 1, 32, 70),       # dh 32 ragged, one valid key in the last tile
        (1, 256, 1, 128, 100),     # dh 128 whole
        (1, 300, 1, 128, 96)]      # dh 128 ragged
# (B, S, H, dh, document lengths per sample, span or None = the longest document)
SEG = [(1, 256, 2, 64, ((40, 216),), None),                      # whole tiles 2 and 3 of block 1
       (1, 384, 2, 32, ((170, 214),), None),                     # dh 32 whole; left-edge tiles 0 .. 3 of block 1 (not 130 + 254: a
                                                                 # `climbing` row over 254 keys has probabilities of 2e-32)
       (2, 197, 2, 64, ((40, 40, 117), (5, 100, 92)), None),     # dh 64 ragged
       (2, 129, 1, 32, ((5, 124), (64, 65)), None),              # dh 32 ragged
       (1, 256, 1, 128, ((96, 160),), None),                     # dh 128 whole
       (1, 300, 2, 128, ((96, 96, 108),), None),                 # dh 128 ragged
       (1, 320, 1, 64, ((200, 120),), 48)]                       # span shorter than the longest document


def is_band(geometry):
    return len(geometry) == 5


def gid(geometry):
    head = "x".join(str(n) for n in geometry[:4])
    if is_band(geometry):
        return "%s-w%d" % (head, geometry[4])
    docs = "_".join(".".join(str(n) for n in d) for d in geometry[4])
    return "%s-d%s%s" % (head, docs, "" if geometry[5] is None else "-s%d" % geometry[5])


@functools.lru_cache(maxsize=None)
def edges(geometry):
    """(B, S, H, dh, lo (B, S) int32 read-only, span)"""
    B, S, H, dh = geometry[:4]
    if is_band(geometry):
        lo, span = SO.band_lo(B, S, geometry[4]), geometry[4]
    else:
        lo, _, longest = SO.layout(S, [list(d) for d in geometry[4]])
        span = longest if geometry[5] is None else geometry[5]
    lo.setflags(write=False)
    return B, S, H, dh, lo, span


def lo_eff_rows(lo, span, H):
    """(B*H, S) int64: the clamped left edge of every (head, row)"""
    return np.repeat(SO.lo_eff(lo, span), H, axis=0)


def allowed_rows(lo, span, H):
    """(B*H, S, S) bool"""
    return np.repeat(SO.allowed(lo, span), H, axis=0)


def documents(lo):
    """(B, S) int: index of every row's document inside its sample"""
    return np.stack([np.unique(row, return_inverse=True)[1].reshape(-1) for row in np.asarray(lo)])


def _frozen(ts, B, S, H, dh, on_grid=True):
    out = []
    for t in ts:
        t = np.ascontiguousarray(np.asarray(t, dtype=f32).reshape(B * S, H * dh))
        t.setflags(write=False)
        out.append(t)
    assert not on_grid or all(np.array_equal(t, R.grid(t)) for t in out[:2])
    return tuple(out)


def _low(B, S, H, dh):
    """q and k of `low` rows: `shifted`'s offsets with the opposite sign on k - every score 47 .. 48 nats DOWN."""
    q, k = (t.reshape(B, S, H, dh) for t in R.rows("plain", B, S, H, dh)[:2])
    u = R.direction(dh)
    return q + R.grid(6.0 * np.sqrt(dh) * u), k - R.grid(8.0 * u)


@functools.lru_cache(maxsize=None)
def rows(kind, geometry, orient=0):
    """(q, k, v, g), each (B*S, H*dh) f32 and read-only; q and k on the grid.
      peaked_in  rows with at least 64 visible keys: q row (r, h) = 4 x key  lo_eff[r] + 32 + (17 r + 37 h) % (r - lo_eff[r] - 31),
                 a key of the row's own, never in its first visible tile; the other rows stay `plain`
      handover   document i of sample b is `climbing` where (i + b + orient) is even and `low` where it is odd"""
    B, S, H, dh, lo, span = edges(geometry)
    if kind in BASE:
        return R.rows(kind, B, S, H, dh)
    q, k, v, g = (np.array(t).reshape(B, S, H, dh) for t in R.rows("plain", B, S, H, dh))
    if kind == "peaked_in":
        le = SO.lo_eff(lo, span)[:, :, None]                                    # (B, S, 1)
        r, h = np.arange(S)[None, :, None], np.arange(H)[None, None, :]
        wide = r - le + 1 >= 64
        peak = le + 32 + (17 * r + 37 * h) % np.where(wide, r - le - 31, 1)     # (B, S, H)
        assert ((peak <= r) & (peak // 32 > le // 32))[np.broadcast_to(wide, peak.shape)].all()
        peaked = f32(4) * k[np.arange(B)[:, None, None], np.where(wide, peak, 0), h]
        q = np.where(wide[..., None], peaked, q)
    else:
        assert kind == "handover" and not is_band(geometry) and orient in (0, 1)
        climbs = ((documents(lo) + np.arange(B)[:, None] + orient) % 2 == 0)[:, :, None, None]
        qc, kc = (t.reshape(B, S, H, dh) for t in R.rows("climbing", B, S, H, dh)[:2])
        ql, kl = _low(B, S, H, dh)
        q, k = np.where(climbs, qc, ql), np.where(climbs, kc, kl)
    return _frozen((q, k, v, g), B, S, H, dh)


def kept_document(geometry, keep, variant):
    """(q, k, v, g, mine): document `keep` = (sample, index) holds `climbing` rows; every OTHER document (of every sample) holds
    `handover` rows of orientation 0 or 1 (variant 0, 1) or, variant "far", finite values of magnitude up to 1e3 in q, k, v and g.
    `mine`: the kept rows in the flat (B*S) layout."""
    B, S, H, dh, lo, span = edges(geometry)
    b, idx = keep
    doc = documents(lo)
    kept = np.zeros((B, S), bool)
    kept[b] = doc[b] == idx
    keptf = kept.reshape(-1)
    climbing = R.rows("climbing", B, S, H, dh)
    if variant == "far":
        other = [(np.random.default_rng(70 + i).random((B * S, H * dh), dtype=f32) * f32(2e3) - f32(1e3)).astype(f32) for i in range(4)]
    else:
        other = rows("handover", geometry, variant)
    out = _frozen([np.where(keptf[:, None], c, o) for c, o in zip(climbing, other)], B, S, H, dh, on_grid=variant != "far")
    return out + (np.flatnonzero(keptf),)


def later_rows(lo, span):
    """(B, S) bool: rows of a LATER document in a wave that straddles a boundary - the row's left edge lies right of the wave's first
    row's, at or after the wave's first row: all its keys are in the wave's diagonal tile."""
    le = SO.lo_eff(lo, span)
    S = le.shape[1]
    q0 = np.arange(S) // 32 * 32
    return (le > le[:, q0]) & (le >= q0[None, :])


def oracle(q, k, v, g, B, H, p, noise, lo, span):
    """(ref64, ref32): tests/segment_oracle.py's composition and the oracle's backward, in both dtypes, fed the same noise.  Keys: out,
    scores, probs, dropped, d_scores, dq, dk, dv."""
    ref, ref32 = {}, {}
    for dt, dst in ((np.float64, ref), (np.float32, ref32)):
        o, cache = SO.attention_core_forward(q.astype(dt), k.astype(dt), v.astype(dt), H, B, p, noise.astype(dt), lo, span)
        dst.update(O.attention_core_backward(cache, g.astype(dt)), out=o, scores=cache["scores"], probs=cache["probs"],
                   dropped=cache["dropped"])
    return ref, ref32


def first_tile_max(sc2, le):
    """(B*H, S) from the (B*H, S, S) log2-domain scores (-inf where not allowed) and the (B*H, S) left edges: the maximum over the
    row's first visible 32-key tile, the tile of its own left edge."""
    key_tile = (np.arange(sc2.shape[2]) // 32)[None, None, :]
    return np.where(key_tile == (le // 32)[..., None], sc2, -np.inf).max(2)


def must_move(sc2, le):
    """(B*H, S) bool: rows whose maximum exceeds the maximum of their first visible tile by more than 6.01.  attention_rows.must_move's
    argument carries over: in its first finite tile a row passes the test by itself (m = -1e30), whatever its wave does; while its
    shift still sits at or below that tile's maximum, the tile that holds the row maximum passes the test, and a shift only moves up."""
    return sc2.max(2) > first_tile_max(sc2, le) + R.THRESHOLD + 0.01


def settled_max(sc2, le):
    """(B*H, S): what the shift of a row that never passes the test by itself after its first finite tile ends at, when no row of its
    wave does either: the maximum over its visible keys in the tiles in which some row of its wave STARTS (a start is an unconditional
    move for the whole wave).  The rows of a wave start in at most two neighbouring tiles under a band; under documents in any tile up
    to the diagonal."""
    BH, S, _ = sc2.shape
    key_tile = np.arange(S) // 32
    out = np.empty((BH, S))
    for w0 in range(0, S, 32):
        rows_ = slice(w0, min(w0 + 32, S))
        for bh in range(BH):
            starts = np.isin(key_tile, np.unique(le[bh, rows_] // 32))
            out[bh, rows_] = np.where(starts[None, :], sc2[bh, rows_], -np.inf).max(1)
    return out


# ---- the kernels' walk and arithmetic, restated ------------------------------------------------------------------------

def walk(S, lo, span):
    """(act, cls), each (B, SP / 32 waves, SP / 32 tiles): the tiles a wave computes, lo_w .. dk inside its block's staged range
    [kt0, nt), and each one's class (index into CLASSES, -1 where not computed) by `left_end` as attention_band_kernel<..., SEG = true> computes it."""
    le = SO.lo_eff(lo, span)
    B = le.shape[0]
    ntile = (S + 31) // 32
    W = min(span, S)
    act, cls = np.zeros((B, ntile, ntile), bool), np.full((B, ntile, ntile), -1)
    for b in range(B):
        for qb in range((S + 127) // 128):
            kt0, nt = 4 * (max(0, 128 * qb - W + 1) // 128), min(ntile, 4 * qb + 4)
            lo_blk = int(le[b, min(128 * qb + 127, S - 1)])
            hi_3 = (lo_blk - 1) // 32 if lo_blk > 0 else -1
            left_end = max(kt0, min(hi_3 + 1, 4 * qb))
            for kt in range(kt0, nt):
                c = 0 if kt < left_end else (1 if kt < 4 * qb else 2)
                for w in range(4):
                    q0, dk = 128 * qb + 32 * w, 4 * qb + w
                    if q0 >= S:
                        continue
                    lo_w = int(le[b, q0]) // 32
                    assert kt0 <= lo_w <= dk < nt
                    if lo_w <= kt <= dk:
                        act[b, dk, kt], cls[b, dk, kt] = True, c
    return act, cls


def replay_forward(q, k, v, B, H, dh, lo, span, flaws=()):
    """attention_rows.replay_forward with the band / seg walk, dropout inactive: per 128-row block the staged tiles [kt0, nt), per
    wave the tiles lo_w .. dk, element mask lo_eff[row] <= key <= row with the clamped row S - 1 for a padded query's left edge, m
    starting at -1e30, the trigger uniform over a wave.
    Returns (out (B*S, H*dh), stats (B*H, S, 2) = final (m2, 1 / l), moves): moves[class] counts the (row, tile) pairs in which a
    row passed the test BY ITSELF after its first finite tile - there alpha < 2^-6 meets a non-zero sum and accumulator -
    and moves["carried"] those in which a shift moved after the row's first finite tile because a neighbour passed.
    flaws: attention_rows.replay_forward's."""
    flaws = set(flaws)
    assert flaws <= {"no_rescale", "no_l_rescale", "row_local_any"}
    S = q.shape[0] // B
    SP = (S + 31) // 32 * 32
    qh, kh, vh = (O._heads_split(np.asarray(t, f32), B, H) for t in (q, k, v))
    BH, c1 = qh.shape[0], R._c1(dh)
    ridx = np.minimum(np.arange(SP), S - 1)
    le = lo_eff_rows(lo, span, H)[:, ridx]                                                     # (BH, SP)
    keys, qrow = np.arange(SP)[None, None, :], np.arange(SP)[None, :, None]
    kept = (keys >= le[..., None]) & (keys <= qrow) & (keys < S)
    raw_all = np.full((BH, SP, SP), -np.inf, f32)
    raw_all[:, :, :S] = np.matmul(qh, kh.transpose(0, 2, 1))[:, ridx]
    raw_all[~kept] = -np.inf
    act_w, cls_w = walk(S, lo, span)
    act_all, cls_all = (np.repeat(np.repeat(t, H, axis=0), 32, axis=1) for t in (act_w, cls_w))   # (BH, SP, ntile)
    vpad = np.zeros((BH, SP, dh), f32); vpad[:, :S] = vh
    m, l = np.full((BH, SP), -1e30, f32), np.zeros((BH, SP), f32)
    oacc = np.zeros((BH, SP, dh), f32)
    real = (np.arange(SP) < S)[None, :]
    seen = np.zeros((BH, SP), bool)
    moves = dict.fromkeys(CLASSES + ("carried",), 0)
    with np.errstate(invalid="ignore", over="ignore"):
        for kt in range(SP // 32):
            act = act_all[:, :, kt]
            raw = raw_all[:, :, 32 * kt:32 * kt + 32]
            tm2 = (raw.max(2) * c1).astype(f32)
            trig = act & (tm2 > m + f32(R.THRESHOLD))
            move = trig if "row_local_any" in flaws else act & np.repeat(trig.reshape(BH, SP // 32, 32).any(2), 32, axis=1)
            m_new = np.where(move, np.maximum(m, tm2), m)
            alpha = np.where(move, np.exp2(m - m_new), f32(1)).astype(f32)
            if "no_l_rescale" not in flaws:
                l = l * alpha
            if "no_rescale" not in flaws:
                oacc = oacc * alpha[..., None]
            later = seen & real
            for c, name in enumerate(CLASSES):
                moves[name] += int((trig & later & (cls_all[:, :, kt] == c)).sum())
            moves["carried"] += int(((m_new != m) & ~trig & later).sum())
            seen |= act & np.isfinite(tm2)
            m = m_new
            e = np.where(act[..., None], np.exp2(R._fma(raw, c1, -m[..., None])), f32(0)).astype(f32)
            half = np.zeros((2, BH, SP), f32)
            for i in range(16):
                half[0] += e[:, :, i]; half[1] += e[:, :, 16 + i]
            l = l + (half[0] + half[1])
            vt = vpad[:, 32 * kt:32 * kt + 32]
            for i in range(16):
                oacc = oacc + e[:, :, i, None] * vt[:, None, i]
                oacc = oacc + e[:, :, 16 + i, None] * vt[:, None, 16 + i]
        inv = f32(1) / l
    out = O._heads_merge(np.ascontiguousarray((oacc * inv[..., None])[:, :S]), B, H)
    return out, np.stack([m, inv], axis=2)[:, :S], moves


def replay_backward(q, k, v, g, out, stats, B, H, dh, allowed):
    """attention_rows.replay_backward with the (B*H, S, S) `allowed` mask in place of the causal triangle."""
    qh, kh, vh, gh, oh = (O._heads_split(np.asarray(t, f32), B, H) for t in (q, k, v, g, out))
    scale, c1 = f32(1.0 / np.sqrt(dh)), R._c1(dh)
    raw = np.where(allowed, np.matmul(qh, kh.transpose(0, 2, 1)), f32(-np.inf)).astype(f32)
    m2, inv = stats[..., 0].astype(f32), stats[..., 1].astype(f32)
    dot = (gh * oh).sum(2, dtype=f32)
    e = np.exp2(R._fma(raw, c1, -m2[..., None]))
    dpd = np.matmul(gh, vh.transpose(0, 2, 1))
    ds = ((e * (inv * scale)[..., None]) * (dpd - dot[..., None])).astype(f32)
    pd = (e * inv[..., None]).astype(f32)
    mg = lambda t: O._heads_merge(np.ascontiguousarray(t), B, H)
    return dict(d_scores=ds, dropped=pd, dq=mg(np.matmul(ds, kh)), dk=mg(np.matmul(ds.transpose(0, 2, 1), qh)),
                dv=mg(np.matmul(pd.transpose(0, 2, 1), gh)))
