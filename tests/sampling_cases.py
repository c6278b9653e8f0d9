"""The fixed inputs of the GPU sampling tests (tests/test_gpu_sampling.py, tests/test_gpu_tape_sampling.py), shared with
tests/test_oracle_sampling.py, which checks on the CPU that none of them is ambiguous at EPS: that is what lets the GPU tests demand
equality of every id.

A case is (V, layout, mode) with an input kind and a seed number chosen ON THE CPU, by search (`search()` below, run by
hand when the lists change), as the first (kind, s) in a fixed preference order for which `sampling_oracle.ambiguity` is empty.  At
large V only peaked inputs can be unambiguous at all - with 10^5 tokens of comparable mass the CDF boundaries lie closer than EPS - so
there the draws come from `ladder` and `dominant` rows, while the flat kinds (`uniform`, `integers`, `equal`, `masked`, `nan`) meet the
greedy-like modes at every V and the drawing modes at the sizes where a row can avoid its boundaries."""
from collections import namedtuple

import numpy as np

import sampling_oracle as SO

EPS = 1e-4
V_TAGS = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099, "L-1", "L", "L+1", "L+4", 50257, 131072)
BOTH_FAMILIES = ("L-1", "L", "L+1", "L+4", 50257)          # every mode on the vector layout AND on a scalar one
# name -> (temperature, top_k, top_p); top_k may name V
MODES = (("greedy", 0.0, 0, 1.0), ("T0.7", 0.7, 0, 1.0), ("T1", 1.0, 0, 1.0), ("T1.5", 1.5, 0, 1.0),
         ("k1", 1.0, 1, 1.0), ("k2", 1.0, 2, 1.0), ("k40", 1.0, 40, 1.0), ("kV-1", 1.0, "V-1", 1.0), ("kV", 1.0, "V", 1.0), ("kV+5", 1.0, "V+5", 1.0),
         ("p1e-6", 1.0, 0, 1e-6), ("p0.5", 1.0, 0, 0.5), ("p0.9", 1.0, 0, 0.9), ("p0.999", 1.0, 0, 0.999), ("p1", 1.0, 0, 1.0),
         ("k40p0.9", 1.0, 40, 0.9), ("k2p0.5", 1.0, 2, 0.5))
KINDS = ("uniform", "integers", "equal", "masked", "nan", "ladder", "dominant")
Case = namedtuple("Case", "tag V layout rows ld lead mode prm kind data_seed seed offset")


def resolve(tag, L):
    return tag if isinstance(tag, int) else L + int(tag[1:] or 0)


def params(mode, V):
    _, T, k, p = mode
    k = {"V-1": V - 1, "V": V, "V+5": V + 5}.get(k, k)
    return SO.Params(T, k, p)


def layout(name, V):
    """-> (rows, ld, lead).  A: the vector family (16-byte aligned base, ld % 4 == 0); B, C, D: leads that take the alignment away."""
    small = V <= 4099
    if name == "A":
        return (17 if small else 3), next(ld for ld in (V, V + 1, V + 3, 2 * V) if ld % 4 == 0), 4
    if name == "B":
        return 1, V, 5
    if name == "C":
        return (17 if small or V == 50257 else 3), V + 1, 6
    return 3, 2 * V, 7


def make(kind, rows, V, data_seed):
    """(rows, V) f32 logits of one input kind"""
    rng = np.random.default_rng(data_seed)
    base = (rng.random((rows, V), dtype=np.float32) * np.float32(16) - np.float32(8)).astype(np.float32)
    if kind == "uniform":
        return base
    if kind == "integers":                                      # massive ties: the threshold-tie rules decide the kept set
        return rng.integers(-3, 4, (rows, V)).astype(np.float32)
    if kind == "equal":
        return np.repeat(rng.integers(-5, 6, (rows, 1)).astype(np.float32), V, axis=1)
    if kind == "masked":                                        # -inf blocks: the shape of a masked vocabulary
        for r in range(rows):
            a, b = sorted(rng.integers(0, V + 1, 2))
            base[r, a:b] = -np.inf
            base[r, :V // 3] = -np.inf if r % 2 else base[r, :V // 3]
        base[:, rng.integers(0, V)] = np.float32(1.5)          # one finite token at least
        return base
    if kind == "nan":
        base[rng.random((rows, V)) < 0.05] = np.nan
        base[:, rng.integers(0, V)] = np.float32(2.5)
        return base
    if kind == "ladder":                                        # token of rank j at -step * j, ranks scattered over the row
        step = np.float32(0.8 + 0.4 * rng.random())
        for r in range(rows):
            rank = rng.permutation(V).astype(np.float32)
            base[r] = np.maximum(-step * rank, np.float32(-60) - np.abs(base[r]))
        return base
    if kind == "dominant":                                      # one to three tokens far above the rest, one of them near the end
        for r in range(rows):
            n = int(rng.integers(1, 4))
            where = rng.choice(V, size=min(n, V), replace=False)
            where[0] = V - 1 - min(int(rng.integers(0, 3)), V - 1)
            base[r, where] = np.float32(30) + rng.random(where.size, dtype=np.float32) * np.float32(3)
        return base
    raise ValueError(kind)


def plan():
    """every (V tag, layout, mode) of the grid, in order: each V meets each of the 17 modes, the layouts (both access families, the
    three row counts, the four strides and leads) rotate over them"""
    out = []
    for vi, tag in enumerate(V_TAGS):
        for mi, mode in enumerate(MODES):
            if tag in BOTH_FAMILIES:
                out += [(tag, "A", mode), (tag, "BCD"[(mi + vi) % 3], mode)]
            else:
                out.append((tag, "ABCD"[(mi + vi) % 4], mode))
    return out


def build(i, tag, lay, mode, kind, s, L):
    V = resolve(tag, L)
    rows, ld, lead = layout(lay, V)
    return Case(tag, V, lay, rows, ld, lead, mode[0], params(mode, V), kind, 1000 * s + i, ((s + 1) * 0x100000001B3 + i) & (2 ** 64 - 1),
                i * 0x40000001)


def search(L, tries=48):
    """the (kind, s) of every entry of plan(): prints the CHOSEN table"""
    chosen = []
    for i, (tag, lay, mode) in enumerate(plan()):
        peaked = KINDS[5:] if i % 2 else KINDS[:4:-1]
        kinds = KINDS[i % 5:5] + KINDS[:i % 5] + peaked if i % 3 else peaked + KINDS[:5]
        for kind, s in ((k, s) for k in kinds for s in range(tries if k in KINDS[5:] else 6)):
            c = build(i, tag, lay, mode, kind, s, L)
            if not SO.ambiguity(make(kind, c.rows, c.V, c.data_seed), c.prm, c.seed, c.offset, EPS):
                chosen.append((kind, s))
                break
        else:
            raise RuntimeError("no unambiguous input for %r" % ((tag, lay, mode),))
    return chosen


def cases(L):
    todo = plan()
    assert len(todo) == len(CHOSEN), (len(todo), len(CHOSEN))
    return [build(i, tag, lay, mode, KINDS[k], s, L) for i, ((tag, lay, mode), (k, s)) in enumerate(zip(todo, CHOSEN))]


def logits(case):
    return make(case.kind, case.rows, case.V, case.data_seed)


# (index into KINDS, s) per entry of plan(), found by search(32768)
CHOSEN = (
    (6, 0), (1, 0), (2, 0), (5, 0), (4, 0), (0, 0), (6, 0), (2, 0), (3, 0), (5, 0), (0, 0), (1, 0), (6, 0), (3, 0), (4, 0), (5, 0), (1, 0),
    (2, 0), (6, 0), (4, 0), (0, 0), (5, 0), (2, 0), (3, 0), (6, 0), (0, 0), (1, 0), (5, 0), (3, 0), (4, 0), (6, 0), (1, 0), (2, 0), (5, 0),
    (4, 0), (0, 0), (6, 0), (2, 0), (3, 0), (5, 0), (0, 0), (1, 0), (6, 0), (3, 0), (4, 0), (5, 0), (1, 0), (2, 0), (6, 0), (4, 0), (0, 0),
    (5, 0), (2, 0), (3, 0), (6, 0), (0, 0), (1, 0), (5, 0), (3, 0), (4, 0), (6, 0), (1, 0), (2, 0), (5, 0), (4, 0), (0, 0), (6, 0), (2, 0),
    (3, 0), (5, 0), (0, 0), (1, 0), (6, 0), (3, 0), (4, 0), (5, 0), (1, 0), (2, 0), (6, 0), (4, 0), (0, 0), (5, 0), (2, 0), (3, 0), (6, 0),
    (0, 0), (1, 0), (5, 0), (3, 1), (4, 0), (6, 0), (1, 0), (2, 0), (5, 0), (4, 0), (0, 0), (6, 0), (2, 0), (2, 0), (5, 0), (0, 0), (1, 0),
    (6, 0), (3, 0), (4, 0), (5, 0), (1, 0), (2, 0), (6, 0), (4, 0), (0, 0), (5, 0), (2, 0), (3, 0), (6, 1), (1, 0), (1, 0), (5, 0), (3, 0),
    (4, 0), (6, 0), (1, 0), (2, 2), (5, 0), (4, 0), (0, 0), (6, 0), (2, 0), (3, 0), (5, 0), (0, 0), (1, 0), (6, 0), (3, 0), (4, 0), (5, 0),
    (1, 0), (2, 0), (6, 0), (4, 0), (0, 0), (5, 0), (2, 1), (3, 0), (6, 0), (0, 0), (1, 0), (5, 0), (3, 0), (1, 0), (6, 0), (1, 0), (2, 1),
    (5, 0), (4, 1), (0, 0), (6, 0), (2, 0), (3, 0), (5, 0), (0, 0), (1, 0), (6, 0), (3, 0), (4, 0), (5, 0), (1, 0), (2, 0), (6, 0), (4, 0),
    (0, 0), (5, 0), (3, 1), (3, 0), (6, 0), (0, 0), (1, 0), (5, 0), (3, 1), (4, 0), (6, 0), (1, 0), (3, 2), (5, 0), (4, 2), (0, 0), (6, 0),
    (2, 0), (3, 0), (5, 0), (0, 0), (1, 0), (6, 0), (3, 0), (1, 5), (5, 0), (2, 3), (2, 0), (6, 0), (4, 0), (6, 0), (5, 0), (2, 4), (3, 0),
    (6, 0), (0, 0), (3, 3), (5, 0), (3, 0), (4, 0), (6, 0), (1, 0), (3, 0), (5, 0), (4, 0), (0, 0), (6, 0), (2, 0), (3, 1), (5, 0), (0, 0),
    (1, 0), (6, 0), (3, 1), (6, 0), (5, 0), (1, 2), (3, 0), (6, 0), (4, 0), (0, 2), (5, 0), (6, 0), (3, 0), (6, 0), (0, 0), (1, 3), (5, 0),
    (3, 0), (4, 0), (6, 0), (3, 0), (3, 0), (5, 0), (6, 0), (5, 0), (6, 0), (3, 0), (3, 0), (5, 0), (0, 0), (3, 0), (6, 0), (3, 2), (4, 0),
    (5, 0), (6, 0), (3, 0), (6, 0), (4, 0), (6, 0), (5, 0), (6, 0), (5, 0), (6, 0), (5, 2), (3, 1), (5, 0), (3, 0), (4, 0), (6, 0), (3, 0),
    (2, 0), (5, 0), (4, 1), (5, 0), (6, 0), (3, 2), (6, 0), (5, 0), (0, 0), (3, 0), (6, 0), (3, 0), (4, 0), (5, 0), (3, 1), (4, 4), (6, 0),
    (3, 5), (3, 0), (5, 0), (3, 0), (3, 0), (6, 0), (5, 0), (6, 0), (5, 0), (6, 0), (5, 0), (6, 0), (5, 0), (3, 0), (5, 0), (4, 1), (0, 4),
    (6, 0), (2, 0), (6, 0), (5, 0), (6, 0), (3, 0), (6, 0), (5, 0), (4, 0), (5, 0), (3, 0), (3, 0), (6, 0), (4, 0), (3, 2), (5, 0), (3, 2),
    (3, 0), (6, 0), (4, 0), (3, 0), (5, 0), (6, 0), (4, 4), (6, 0), (5, 0), (6, 0), (5, 1), (6, 0), (3, 0), (6, 0), (3, 0), (6, 0), (5, 0),
    (0, 0), (1, 0), (6, 0), (3, 1), (6, 0), (5, 0), (6, 0), (5, 0), (6, 0), (4, 0), (0, 0), (5, 0), (3, 0), (3, 0), (6, 0), (0, 0), (6, 0),
    (5, 1), (3, 2), (5, 0), (6, 0), (3, 0), (3, 3), (5, 0), (6, 0), (5, 0), (6, 0), (5, 0), (3, 0), (5, 0), (0, 0), (3, 0), (6, 0), (3, 2),
    (4, 0), (5, 0), (3, 5), (5, 0), (6, 0), (5, 0), (6, 0), (5, 0), (3, 0), (3, 0), (6, 0), (0, 0), (3, 0), (5, 0), (6, 0), (5, 0), (6, 0),
    (5, 0), (6, 0), (5, 0), (4, 0), (0, 0), (6, 0), (5, 0), (6, 0), (5, 0), (6, 0), (5, 0), (6, 0), (3, 1), (4, 0), (5, 0), (6, 0), (5, 0),
    (6, 0), (5, 0), (3, 0), (5, 0), (3, 0), (3, 0), (6, 0), (5, 0), (6, 0), (5, 0), (3, 0), (5, 0), (6, 0), (5, 0), (6, 0), (5, 0), (6, 0),
)


# One input drawn at eight consecutive offsets (test_gpu_sampling: different offsets give the oracle's different draws), and the
# inputs of the tape tests: (batch, T, V, params, kind) with logits of batch * T rows, of which the last row of every sample is drawn
# twice (offsets 0 and 1).  The seed number of each is the first for which no draw is ambiguous (`search_extras`).
OFFSETS = dict(rows=3, V=64, prm=SO.Params(0.9, 0, 1.0), kind="uniform", offsets=tuple(range(8)))
TAPE = ((3, 1, 64, SO.Params(0.8, 8, 1.0), "uniform"), (2, 3, 257, SO.Params(1.0, 0, 0.9), "integers"), (4, 3, 1000, SO.Params(0.0, 0, 1.0), "uniform"),
        (2, 1, 40000, SO.Params(0.7, 40, 0.95), "ladder"))
OFFSETS_S, TAPE_S = 0, (0, 0, 0, 0)                          # found by search_extras()


def extra_seed(s, i):
    return (0xC0FFEE + 7919 * s + i) & (2 ** 64 - 1)


def offsets_input(s=None):
    s = OFFSETS_S if s is None else s
    return make(OFFSETS["kind"], OFFSETS["rows"], OFFSETS["V"], 500 + s), extra_seed(s, 99)


def tape_input(i, s=None):
    """-> (logits (batch * T, V), the rows that are drawn (batch, V), sampler seed)"""
    s = TAPE_S[i] if s is None else s
    batch, T, V, _, kind = TAPE[i]
    x = make(kind, batch * T, V, 700 + 10 * s + i)
    return x, x.reshape(batch, T, V)[:, -1], extra_seed(s, i)


def search_extras(tries=200):
    def first(ok):
        return next(s for s in range(tries) if ok(s))
    o = first(lambda s: not any(SO.ambiguity(offsets_input(s)[0], OFFSETS["prm"], offsets_input(s)[1], off, EPS) for off in OFFSETS["offsets"]))
    t = tuple(first(lambda s, i=i: not any(SO.ambiguity(tape_input(i, s)[1], TAPE[i][3], tape_input(i, s)[2], off, EPS) for off in (0, 1)))
              for i in range(len(TAPE)))
    return o, t
