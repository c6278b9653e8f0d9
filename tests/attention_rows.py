"""Score rows that move the fused attention core's online-softmax shift, and a NumPy replay of the kernel's row arithmetic.

The kernels (nk_attention.hip, tile body nk_attention_tile.h) keep a LAZY running shift: a row's shift m2 (base-2 exponent domain)
moves only when a 32-key tile's maximum exceeds it by more than 6, the test is uniform over the 32 queries of a wave, and only then
are the running sum and the out accumulator multiplied by alpha = exp2(m_old - m_new).  Uniform [-1, 1) data never gets there after
the first tile.  The row kinds here do, and each isolates one mechanism (KINDS below).

Exact scores.  Every q and k entry is a multiple of 1/8 with |x| <= 16: a product is a multiple of 1/64 below 2^8, a dot product over
dh <= 128 a multiple of 1/64 below 2^15 - fewer than 24 significant bits in ANY summation order.  The f64 oracle, the f32 oracle and
the MFMA therefore agree on the raw scores bit for bit, and the parity policy of tests/test_gpu_attention.py (`bound`) applies to
everything downstream without the f32 score rounding amplified by |z| up to 60.  v and g stay uniform [-1, 1).

`replay_forward` / `replay_backward` restate the kernel's per-row operations in f32 NumPy (tests/test_oracle_attention_rows.py uses
them to prove, without a GPU, that the inputs reach the rescale branch and that the policy bound is satisfiable); `flaws` switches on
wrong behaviours, the idiom of tests/adamw_oracle.py."""
import functools

import numpy as np

from oracle import neuronika_oracle as O
import causal_oracle as CO

f32 = np.float32

KINDS = ("plain", "climbing", "falling", "mixed", "under", "peaked", "shifted")
MOVING = ("climbing", "mixed", "peaked")      # the shift moves after tile 0
STILL = ("plain", "falling", "under")         # it does not

# (B, S, H, dh): the smallest geometries at which each mechanism exists
GEOMETRIES = [(1, 64, 1, 64),      # two key tiles: the minimum for a rescale
              (2, 100, 2, 32),     # ragged last tile (-inf), per-(b, h) statistics
              (1, 160, 2, 64),     # five tiles; a second, partial 128-row query block
              (1, 96, 1, 128),     # four output column tiles
              (1, 129, 1, 64)]     # ONE valid key in the last tile (it carries the row maximum of `climbing`)

THRESHOLD = 6.0                     # log2 units: nk_attention_tile.h, `tm2 > m_run + 6.f`
LOG2E_F32 = f32(1.44269504088896341)


def grid(a):
    """Rounded to multiples of 1/8, clipped to |x| <= 16."""
    return np.clip(np.round(np.asarray(a, np.float64) * 8.0) / 8.0, -16.0, 16.0).astype(f32)


def uniform(seed, shape):
    """Uniform [-1, 1) f32: the data of tests/test_gpu_attention.py."""
    a = np.random.default_rng(seed).random(shape, dtype=f32)
    return np.asarray(a * f32(2) - f32(1), dtype=f32)


def direction(dh):
    """The fixed unit-norm direction of the structured components: equal entries on every second coordinate."""
    u = np.zeros(dh)
    u[::2] = np.sqrt(2.0 / dh)
    return u


def under_tile(S):
    """The late key tile `under` lifts: the last WHOLE tile."""
    return S // 32 - 1


def peak_key(S, H):
    """(S, H) key index that carries row (r, h)'s mass in `peaked`: never in tile 0, neighbouring rows in different tiles."""
    r, h = np.arange(S)[:, None], np.arange(H)[None, :]
    return 32 + (17 * r + 37 * h) % (S - 32)


@functools.lru_cache(maxsize=None)
def rows(kind, B, S, H, dh, seed=0):
    """(q, k, v, g), each (B*S, H*dh) f32 and read-only; q and k on the grid.  z below is the scaled score in nats (6 in log2
    units = 4.16 nats).
      plain     uniform data on the grid: the control, spread ~2.5 nats, the shift stays after tile 0
      climbing  q += 2 sqrt(dh) u, key j += j/8 u: z rises ~0.25 nat per key, ~8 nats per tile - the shift moves in every tile
      falling   the same with j reversed: the same spread, the maximum in tile 0 - the shift moves in tile 0 only
      mixed     `climbing` on the ODD query rows only: the even rows of a wave are carried along by the wave-uniform test
      under     one late tile (`under_tile`) lies 3.7 nats (5.4 in log2 units) above the others: below the threshold, the shift
                stays and the terms reach 2^5.4 (the kernel comment's "terms stay <= 64").  The random part of z lives on the
                coordinates u leaves free and is small (|q| <= 1/4 there), so that no row crosses the threshold by chance
      peaked    q row (r, h) = 4 x key `peak_key`: that key has z ~ 4 |k|^2 / sqrt(dh) = 7.5 .. 15 nats, the others ~N(0, 1.3)
      shifted   q += 6 sqrt(dh) u, k += 8 u: every score carries a common offset of 47 .. 48 nats, spread ~20"""
    assert kind in KINDS and S >= 64
    shape = (B, S, H, dh)
    q, k, v, g = (uniform(seed * 16 + i, shape) for i in (1, 2, 3, 4))
    q, k = grid(q), grid(k)
    u = direction(dh)
    j = np.arange(S, dtype=np.float64)[None, :, None, None]
    lift = grid(2.0 * np.sqrt(dh) * u)
    if kind in ("climbing", "falling", "mixed"):
        k = k + grid(0.125 * (S - 1 - j if kind == "falling" else j) * u)
        if kind == "mixed":
            q[:, 1::2] += lift
        else:
            q = q + lift
    elif kind == "under":
        free = u == 0
        q = np.where(free, grid(q * 0.25), grid(20.0 / np.sqrt(dh))).astype(f32)          # a on u's coordinates
        late = (j // 32 == under_tile(S))
        k = np.where(free, k, np.where(late, f32(0.375), f32(0))).astype(f32)              # sqrt(dh) / 2 * a * 0.375 = 3.7 nats
    elif kind == "peaked":
        pk = peak_key(S, H)
        q = f32(4) * k[:, pk, np.arange(H)[None, :], :]
    elif kind == "shifted":
        q, k = q + grid(6.0 * np.sqrt(dh) * u), k + grid(8.0 * u)
    out = []
    for t in (q, k, v, g):
        t = np.ascontiguousarray(np.asarray(t, dtype=f32).reshape(B * S, H * dh))
        t.setflags(write=False)
        out.append(t)
    assert all(np.array_equal(t, grid(t)) for t in out[:2])
    return tuple(out)


def visible(S, causal):
    """(S, S) bool: key visible to query."""
    r, c = np.arange(S)[:, None], np.arange(S)[None, :]
    return (c <= r) if causal else np.ones((S, S), bool)


def oracle(q, k, v, g, B, H, p, noise, causal):
    """(ref64, ref32): the oracle's node-by-node composition (tests/causal_oracle.py adds the mask) and its backward, in both
    dtypes, fed the same noise.  Keys: out, scores, probs, dropped, d_scores, dq, dk, dv."""
    ref, ref32 = {}, {}
    for dt, dst in ((np.float64, ref), (np.float32, ref32)):
        o, cache = CO.attention_core_forward(q.astype(dt), k.astype(dt), v.astype(dt), H, B, p, noise.astype(dt), causal=causal)
        dst.update(O.attention_core_backward(cache, g.astype(dt)), out=o, scores=cache["scores"], probs=cache["probs"],
                   dropped=cache["dropped"])
    return ref, ref32


def terms(ref, q, k, v, g, p):
    """The yardsticks of test_attention_core_equals_oracle: for a contraction, the size of the summed terms."""
    return {"out": float(np.abs(v).max() / (1 - p)),
            "dq": float(np.abs(ref["d_scores"]).sum(2).max() * np.abs(k).max()),
            "dk": float(np.abs(ref["d_scores"]).sum(1).max() * np.abs(q).max()),
            "dv": float(np.abs(ref["dropped"]).sum(1).max() * np.abs(g).max())}


def cancelling_terms(ref, q, k, v, g, B, H, p, noise):
    """Yardsticks of dS, dQ and dK on rows where the score gradient CANCELS, derived from the kernel's operations (DESIGN.md
    section 5).  The backward forms  dS_i = scale * P_i * (dP_i - dot)  with the softmax dot taken through the forward's output,
    dot = keep * dO . O = sum_k P_k noise_k (dO . v_k): a contraction over the dh columns of a contraction over the keys, whose
    summed terms have the size  A = sum_k P_k noise_k (|dO| . |v_k|).  On a peaked row P_i -> 1 and dP_i - dot -> 0: the result
    shrinks, the rounding of dot (and of the O it is read from) does not, and the oracle - which sums dP * P directly - has no such
    term to set against it.  SURVEY 8c (ii) measures a contraction by its summed terms, not by the cancelling result
    (test_gpu_attention.py does so for O, dQ, dK, dV, and for S = 1, where the cancellation is total, measures dS by dP's size):
        t_i = scale * P_i * (|dP_i| + A)  >=  |dS_i|,
    and dQ = dS . K, dK = dS^T . Q inherit sum_i t_i * max|k| and sum_r t * max|q|.  Everything from the f64 oracle."""
    dh = q.shape[1] // H
    ga, va, gh, vh = (O._heads_split(t.astype(np.float64), B, H) for t in (np.abs(g), np.abs(v), g, v))
    n = noise.astype(np.float64) if p != 0.0 else 1.0          # (dropout inactive: `noise` is not read)
    pn = ref["probs"] * n
    a = (pn * np.matmul(ga, va.transpose(0, 2, 1))).sum(2, keepdims=True)
    t = np.float64(f32(1.0 / np.sqrt(dh))) * ref["probs"] * (np.abs(np.matmul(gh, vh.transpose(0, 2, 1))) * n + a)
    assert (t >= np.abs(ref["d_scores"]) * (1 - 1e-12)).all()
    return {"d_scores": float(t.max()), "dq": float(t.sum(2).max() * np.abs(k).max()), "dk": float(t.sum(1).max() * np.abs(q).max())}


def bound(want64, want32, floor=0.0):
    """SURVEY.md 8c (ii) as `_check` of tests/test_gpu_attention.py states it: max(2 * err_cpu32, 1e-6 * yardstick)."""
    return max(2 * np.abs(want32 - want64).max(), 1e-6 * max(np.abs(want64).max(), floor))


def log2_scores(ref_scores, dh, vis):
    """f64 scores in the kernel's exponent domain (s * c1 with the f32 scale), -inf where invisible."""
    c1 = np.float64(f32(1.0 / np.sqrt(dh))) * np.log2(np.e)
    return np.where(vis, ref_scores * c1, -np.inf)


def must_move(sc2):
    """(B*H, S) bool from the (B*H, S, S) `log2_scores`: rows whose maximum exceeds their tile-0 maximum by more than 6.01.
    Whatever the neighbours of the wave do, such a row's shift has to end above its tile-0 maximum: while it still sits there, the
    tile that holds the maximum passes the kernel's test, and a shift only ever moves up."""
    return sc2.max(2) > sc2[:, :, :32].max(2) + THRESHOLD + 0.01


# ---- the kernel's arithmetic, restated ---------------------------------------------------------------------------------

def _c1(dh):
    return f32(f32(1.0 / np.sqrt(dh)) * LOG2E_F32)          # nk_attention.hip: a.c1 = scale * 1.44269504088896341f


def _fma(a, b, c):
    """One rounding: the f64 product of two f32 is exact."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(f32)


def _padded_scores(qh, kh, S, SP, causal):
    """(B*H, SP, SP) f32 raw scores as a wave sees them: padded queries are copies of row S - 1, padded keys and (causal) keys above
    the query's position hold -inf."""
    ridx = np.minimum(np.arange(SP), S - 1)
    raw = np.full((qh.shape[0], SP, SP), -np.inf, f32)
    raw[:, :, :S] = np.matmul(qh, kh.transpose(0, 2, 1))[:, ridx]
    if causal:
        raw[:, np.arange(SP)[None, :] > np.arange(SP)[:, None]] = -np.inf
    return raw, ridx


def replay_forward(q, k, v, B, H, dh, causal, flaws=()):
    """The forward tile recurrence of nk_attention_tile.h in f32, dropout inactive: 32-key tiles, 32-query waves with the
    wave-uniform trigger, c1 = f32(scale) * f32(log2 e), one rounding per fma(raw, c1, -m), exp2, m starting at -1e30, -inf for
    ragged keys and keys above the diagonal, (causal) a wave walks the tiles up to its own.  The second product accumulates in the
    MFMA's key order (step e pairs key e with key 16 + e of the tile).
    Returns (out (B*S, H*dh), stats (B*H, S, 2) = final (m2, 1 / l), number of (row, tile > 0) pairs in which a row's shift moved).
    flaws: "no_rescale" skips oacc *= alpha, "no_l_rescale" skips l_run *= alpha, "row_local_any" lets only a row that passes
    the test itself move."""
    flaws = set(flaws)
    assert flaws <= {"no_rescale", "no_l_rescale", "row_local_any"}
    S = q.shape[0] // B
    SP = (S + 31) // 32 * 32
    qh, kh, vh = (O._heads_split(np.asarray(t, f32), B, H) for t in (q, k, v))
    raw_all, ridx = _padded_scores(qh, kh, S, SP, causal)
    BH, c1 = qh.shape[0], _c1(dh)
    vpad = np.zeros((BH, SP, dh), f32); vpad[:, :S] = vh
    m, l = np.full((BH, SP), -1e30, f32), np.zeros((BH, SP), f32)
    oacc = np.zeros((BH, SP, dh), f32)
    wave = np.arange(SP) // 32
    real = np.arange(SP) < S
    moved = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for kt in range(SP // 32):
            act = (wave >= kt)[None, :] if causal else np.ones((1, SP), bool)
            raw = raw_all[:, :, 32 * kt:32 * kt + 32]
            tm2 = (raw.max(2) * c1).astype(f32)
            trig = act & (tm2 > m + f32(THRESHOLD))
            move = trig if "row_local_any" in flaws else act & np.repeat(trig.reshape(BH, SP // 32, 32).any(2), 32, axis=1)
            m_new = np.where(move, np.maximum(m, tm2), m)
            alpha = np.where(move, np.exp2(m - m_new), f32(1)).astype(f32)
            if "no_l_rescale" not in flaws:
                l = l * alpha
            if "no_rescale" not in flaws:
                oacc = oacc * alpha[..., None]
            if kt:
                moved += int(((m_new != m) & real[None, :]).sum())
            m = m_new
            e = np.where(act[..., None], np.exp2(_fma(raw, c1, -m[..., None])), f32(0)).astype(f32)
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
    return out, np.stack([m, inv], axis=2)[:, :S], moved


def replay_backward(q, k, v, g, out, stats, B, H, dh, causal):
    """The backward's recomputation in f32, dropout inactive: every probability from the stored (shift, 1 / sum) pair,
    e = exp2(fma(s, c1, -m2)), the softmax dot as dO . O, dS = (e * (inv * scale)) * (dPd - dot), Pd = e * inv, then the three
    products.  Returns dict(d_scores, dropped, dq, dk, dv) in the oracle's layouts."""
    S = q.shape[0] // B
    qh, kh, vh, gh, oh = (O._heads_split(np.asarray(t, f32), B, H) for t in (q, k, v, g, out))
    vis = visible(S, causal)
    scale, c1 = f32(1.0 / np.sqrt(dh)), _c1(dh)
    raw = np.where(vis, np.matmul(qh, kh.transpose(0, 2, 1)), f32(-np.inf)).astype(f32)
    m2, inv = stats[..., 0].astype(f32), stats[..., 1].astype(f32)
    dot = (gh * oh).sum(2, dtype=f32)
    e = np.exp2(_fma(raw, c1, -m2[..., None]))
    dpd = np.matmul(gh, vh.transpose(0, 2, 1))
    ds = ((e * (inv * scale)[..., None]) * (dpd - dot[..., None])).astype(f32)
    pd = (e * inv[..., None]).astype(f32)
    mg = lambda t: O._heads_merge(np.ascontiguousarray(t), B, H)
    return dict(d_scores=ds, dropped=pd, dq=mg(np.matmul(ds, kh)), dk=mg(np.matmul(ds.transpose(0, 2, 1), qh)),
                dv=mg(np.matmul(pd.transpose(0, 2, 1), gh)))
