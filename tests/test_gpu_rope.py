"""nk_rope_* through the C ABI (`capi`) against tests/rope_oracle.py in f64.  Every device array sits between guard bands that must
come back intact (tests/test_gpu_embedding.py's `Guarded`).

Bound (include/neuronika_hip.h fixes the expression): with a table entry at most 1 ulp off and
    y1 = fmaf(x1, c, -(x2 * s)),  y2 = fmaf(x2, c, x1 * s)
each element carries the rounding of one product (2^-24 |x2 s|), of the fused sum (2^-24 |y|) and the table's error in both terms
(2^-23 (|x1| + |x2|) at the very most): |y - y64| <= 2^-22 (|x1| + |x2|).  A pass-through column is exact.  `+=` adds one rounding
of the sum: bound (1 + 2^-24) + 2^-24 |dx0 + r|.  err / bound is recorded under `rope:*`."""
import itertools

import numpy as np
import pytest

import rope_oracle as RO
from test_gpu_embedding import Guarded, same_bits

pytestmark = pytest.mark.gpu

MAX_POS = 200
U = 2.0 ** -24
RAGGED = [0, 9, 130]
# (dh, rot): full vector 32 / 64 / 128, smallest half-split vector, interleaved vector, scalar by rot, partial x 2, smallest
SHAPES = [(32, 32), (64, 64), (128, 128), (8, 8), (4, 4), (20, 20), (64, 32), (20, 8), (2, 2)]
# name -> (heads in the launch as a multiple of NH, row stride as a function of (heads, dh), lead of the data arrays, lead of the table)
LAYOUTS = {"dense": (1, lambda n, dh: n * dh, 4, 4), "packed": (2, lambda n, dh: 3 * (n // 2) * dh, 4, 4), "ld + 1": (1, lambda n, dh: n * dh + 1, 4, 4),
           "packed, off 2": (2, lambda n, dh: 3 * (n // 2) * dh, 6, 4),
           "off 1": (1, lambda n, dh: n * dh, 5, 4), "off 2": (1, lambda n, dh: n * dh, 6, 4), "off 3, table off 1": (1, lambda n, dh: n * dh, 7, 5)}
_WORST = {}


@pytest.fixture(scope="module")
def tables(dev):
    """(rot, lead) -> (Guarded device table, f64 oracle table); filled by the library once per shape"""
    from neuronika_amd import capi as c
    made = {}

    def get(rot, lead=4):
        if (rot, lead) not in made:
            t = Guarded(dev, np.zeros((MAX_POS, rot // 2, 2), np.float32), lead)
            c.rope_table(dev, t.body, MAX_POS, rot)
            made[(rot, lead)] = (t, RO.table(MAX_POS, rot))
        return made[(rot, lead)]
    yield get
    for t, _ in made.values():
        t.numpy()                                                        # guards of every table


def uniform(seed, shape):
    return (np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(6) - np.float32(3)).astype(np.float32)


def embed(logical, ld, fill):
    """(rows, n*dh) logical columns into a (rows, ld) buffer whose other columns hold `fill`"""
    a = np.array(fill[:, :ld], dtype=np.float32)
    a[:, :logical.shape[1]] = logical
    return a


def pair_sum(x, n, dh, rot, il):
    """|x1| + |x2| per rotated element, 0 in the pass-through columns"""
    xh = np.abs(x.astype(np.float64)).reshape(-1, n, dh)
    out = np.zeros_like(xh)
    c1, c2 = RO.pair_columns(rot, il)
    out[:, :, c1] = out[:, :, c2] = xh[:, :, c1] + xh[:, :, c2]
    return out.reshape(x.shape)


def margin(what, err, bound):
    r = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    _WORST[what] = max(_WORST.get(what, 0.0), r)
    from conftest import record_margin
    record_margin("rope:" + what, r, 0.5, 1.0)                          # err / bound, on both scales of the table
    return r


def launch_all(dev, c, tab, x, g, dx0, fill, ld, lead, start, B, T, n, dh, rot, il):
    """Forward out of place and in place, assign backward out of place and in place, `+=` backward; -> the five (rows, ld) results."""
    st = None if start is None else dev.int_array(np.asarray(start, np.int32))
    X, G = Guarded(dev, embed(x, ld, fill), lead), Guarded(dev, embed(g, ld, fill), lead)
    Y, DA = Guarded(dev, fill[:, :ld], lead), Guarded(dev, fill[:, :ld], lead)
    XI, GI = Guarded(dev, embed(x, ld, fill), lead), Guarded(dev, embed(g, ld, fill), lead)
    DX = Guarded(dev, embed(dx0, ld, fill), lead)
    geom = (tab.body, st, B, T, n, dh, rot, MAX_POS, il)
    c.rope_fwd(dev, X.body, ld, Y.body, ld, *geom)
    c.rope_fwd(dev, XI.body, ld, XI.body, ld, *geom)
    c.rope_bwd(dev, DA.body, ld, G.body, ld, *geom, assign=True)
    c.rope_bwd(dev, GI.body, ld, GI.body, ld, *geom, assign=True)
    c.rope_bwd(dev, DX.body, ld, G.body, ld, *geom)
    same_bits(X.numpy(), embed(x, ld, fill), "x is read only")
    same_bits(G.numpy(), embed(g, ld, fill), "g is read only")
    return Y.numpy(), XI.numpy(), DA.numpy(), GI.numpy(), DX.numpy()


@pytest.mark.parametrize("il", [False, True], ids=["half-split", "interleaved"])
@pytest.mark.parametrize("dh,rot", SHAPES)
def test_grid(dev, tables, dh, rot, il):
    from neuronika_amd import capi as c
    fill = uniform(99, (201, 3 * 8 * 128 + 8))
    for NH, (B, T), start_kind in itertools.product((1, 3, 8), ((1, 1), (2, 5), (3, 67)), ("null", "zero", "ragged")):
        start = {"null": None, "zero": [0] * B, "ragged": RAGGED[-B:]}[start_kind]
        rows, bits = B * T, {}
        for name, (mult, ld_of, lead, tlead) in LAYOUTS.items():
            n = NH * mult
            ld, w = ld_of(n, dh), n * dh
            tab, tab64 = tables(rot, tlead)
            key = (n,)
            if key not in bits:                                          # one logical problem and one f64 reference per head count
                x, g, dx0 = (uniform(s * 1000 + n * 7 + rows, (rows, w)) for s in (1, 2, 3))
                y64 = RO.rope(x.astype(np.float64), start, T, n, dh, rot, il, tab64)
                d64 = RO.rope(g.astype(np.float64), start, T, n, dh, rot, il, tab64, inverse=True)
                bits[key] = dict(x=x, g=g, dx0=dx0, y64=y64, d64=d64, bx=2.0 ** -22 * pair_sum(x, n, dh, rot, il),
                                 bg=2.0 ** -22 * pair_sum(g, n, dh, rot, il), first=None)
            p = bits[key]
            y, yi, da, dai, dx = launch_all(dev, c, tab, p["x"], p["g"], p["dx0"], fill[:rows], ld, lead, start, B, T, n, dh, rot, il)
            what = "%s dh %d rot %d NH %d B %d T %d start %s" % (name, dh, rot, n, B, T, start_kind)
            # the bound, as the issue states it
            assert margin("fwd", np.abs(y[:, :w] - p["y64"]), p["bx"]) <= 1.0, what
            assert margin("bwd_assign", np.abs(da[:, :w] - p["d64"]), p["bg"]) <= 1.0, what
            acc = p["dx0"].astype(np.float64) + p["d64"]
            assert margin("bwd", np.abs(dx[:, :w] - acc), p["bg"] * (1 + U) + U * np.abs(acc)) <= 1.0, what
            # columns past the heads (the V block of a packed buffer, the ld + 1 column): bit for bit what they held
            for out in (y, yi, da, dai, dx):
                same_bits(out[:, w:], fill[:rows, w:ld], what + ": columns >= NH*dh")
            # pass-through columns: a copy, dx + g
            for h in range(n if rot < dh else 0):
                lo, hi = h * dh + rot, (h + 1) * dh
                same_bits(y[:, lo:hi], p["x"][:, lo:hi], what + ": pass-through forward")
                same_bits(da[:, lo:hi], p["g"][:, lo:hi], what + ": pass-through assign")
                same_bits(dx[:, lo:hi], p["dx0"][:, lo:hi] + p["g"][:, lo:hi], what + ": pass-through +=")
            same_bits(yi[:, :w], y[:, :w], what + ": in place == out of place (forward)")
            same_bits(dai[:, :w], da[:, :w], what + ": in place == out of place (assign backward)")
            # every layout of one logical problem - aligned and misaligned bases, strides: the vector and the scalar family - same bits
            if p["first"] is None:
                p["first"] = (y[:, :w].copy(), da[:, :w].copy(), dx[:, :w].copy(), name)
            else:
                for got, want in zip((y, da, dx), p["first"]):
                    same_bits(got[:, :w], want, what + ": against layout " + p["first"][3])
            if start_kind != "ragged":                                   # position 0: the finite input unchanged
                same_bits(y[0::T, :w], p["x"][0::T], what + ": position 0")
            # the round trip: within twice the bound of x
            if name == "dense":
                Y, XR = Guarded(dev, y[:, :w], 4), Guarded(dev, np.zeros_like(y[:, :w]), 4)
                st = None if start is None else dev.int_array(np.asarray(start, np.int32))
                c.rope_bwd(dev, XR.body, w, Y.body, w, tab.body, st, B, T, n, dh, rot, MAX_POS, il, assign=True)
                back = XR.numpy()
                assert margin("round trip", np.abs(back.astype(np.float64) - p["x"]), 2 * p["bx"]) <= 1.0, what
    print("worst err / bound so far:", {k: round(v, 3) for k, v in _WORST.items()})


def test_a_row_depends_on_its_position_only(dev, tables):
    """Row p of a (B = 3, T = 67, NH = 8, packed stride) call against (start = p, t = 0, B = 1, NH = 1, dense), head by head; two runs
    of the large call agree."""
    from neuronika_amd import capi as c
    for (dh, rot), il in itertools.product(((64, 64), (64, 32), (20, 8), (4, 4)), (False, True)):
        tab, _ = tables(rot)
        B, T, n = 3, 67, 8
        ld, w = 3 * (n // 2) * dh, n * dh
        x = uniform(5, (B * T, ld))
        runs = []
        for _ in range(2):
            X, Y = Guarded(dev, x, 4), Guarded(dev, np.zeros_like(x), 4)
            c.rope_fwd(dev, X.body, ld, Y.body, ld, tab.body, None, B, T, n, dh, rot, MAX_POS, il)
            runs.append(Y.numpy())
        same_bits(runs[0], runs[1], "two runs")
        for b, t, h in ((0, 0, 0), (0, 66, 7), (1, 33, 3), (2, 1, 5), (2, 66, 0)):
            one = np.ascontiguousarray(x[b * T + t, h * dh:(h + 1) * dh].reshape(1, dh))
            X, Y = Guarded(dev, one, 4), Guarded(dev, np.zeros_like(one), 4)
            c.rope_fwd(dev, X.body, dh, Y.body, dh, tab.body, dev.int_array(np.array([t], np.int32)), 1, 1, 1, dh, rot, MAX_POS, il)
            same_bits(Y.numpy()[0], runs[0][b * T + t, h * dh:(h + 1) * dh], "row (%d, %d) head %d dh %d rot %d il %d" % (b, t, h, dh, rot, il))
        # how p splits into start[b] + t does not matter: the rows of sample 1 as a call of their own starting at 20
        X, Y = Guarded(dev, x[T + 20:2 * T], 4), Guarded(dev, np.zeros_like(x[T + 20:2 * T]), 4)
        c.rope_fwd(dev, X.body, ld, Y.body, ld, tab.body, dev.int_array(np.array([20], np.int32)), 1, T - 20, n, dh, rot, MAX_POS, il)
        same_bits(Y.numpy()[:, :w], runs[0][T + 20:2 * T, :w], "start 20 + t")


@pytest.mark.parametrize("dh,rot,lead", [(64, 64, 4), (64, 32, 4), (20, 8, 4), (64, 64, 5)])
def test_positions_outside_the_table_are_clamped(dev, tables, dh, rot, lead):
    """start beyond max_pos and negative: no fault, the guard bands of the table intact, the clamped positions' values."""
    from neuronika_amd import capi as c
    B, T, n = 3, 5, 3
    tab, _ = tables(rot)
    x = uniform(6, (B * T, n * dh))
    start = np.array([-3, MAX_POS - 2, 2 ** 31 - 3], np.int32)
    want_pos = RO.positions(start, B, T, MAX_POS)
    assert list(want_pos[:5]) == [0, 0, 0, 0, 1] and list(want_pos[5:]) == [198, 199, 199, 199, 199] + [199] * 5
    for il in (False, True):
        X, Y, W = Guarded(dev, x, lead), Guarded(dev, np.zeros_like(x), lead), Guarded(dev, np.zeros_like(x), lead)
        c.rope_fwd(dev, X.body, n * dh, Y.body, n * dh, tab.body, dev.int_array(start), B, T, n, dh, rot, MAX_POS, il)
        c.rope_fwd(dev, X.body, n * dh, W.body, n * dh, tab.body, dev.int_array(want_pos.astype(np.int32)), B * T, 1, n, dh, rot, MAX_POS, il)
        same_bits(Y.numpy(), W.numpy(), "clamped positions")
        tab.numpy()


def _ulps_off(got, want64):
    want = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def test_table(dev):
    """Every entry within 1 f32 ulp of the f64 value's rounding: max_pos = 4096 in full, and the far end of 131072 positions."""
    from neuronika_amd import capi as c
    for max_pos, rot in ((4096, 128), (4096, 6), (131072, 16)):
        T = Guarded(dev, np.full((max_pos, rot // 2, 2), np.nan, np.float32), 4)
        c.rope_table(dev, T.body, max_pos, rot)
        got = T.numpy()
        lo = 0 if max_pos == 4096 else 131072 - 8
        want = RO.table(max_pos, rot, positions=np.arange(lo, max_pos))
        off = _ulps_off(got[lo:], want)
        print("table max_pos %d rot %d: worst %.2f ulp, exact %.4f" % (max_pos, rot, off.max(), (off == 0).mean()))
        assert np.all(np.isfinite(got)) and off.max() <= 1.0
        assert np.all(got[0, :, 0] == 1.0) and np.all(got[0, :, 1] == 0.0)
        assert got[max_pos - 1, 0, 0] == np.float32(np.cos(float(max_pos - 1)))      # position 131071 at frequency 1: f64 cos, not an f32 angle
    base = Guarded(dev, np.zeros((64, 4, 2), np.float32), 4)
    c.rope_table(dev, base.body, 64, 8, 500000.0)
    assert _ulps_off(base.numpy(), RO.table(64, 8, 500000.0)).max() <= 1.0


def test_refusals_write_nothing(dev, tables):
    from neuronika_amd import capi as c
    B, T, n, dh = 2, 3, 2, 8
    tab, _ = tables(8)
    x = uniform(7, (B * T, n * dh))
    mark = uniform(8, (B * T, n * dh))
    good = dict(ldx=n * dh, ldy=n * dh, B=B, T=T, NH=n, dh=dh, rot=8, max_pos=MAX_POS)
    bad = [dict(rot=7), dict(rot=0), dict(rot=10), dict(rot=-2), dict(ldx=n * dh - 1), dict(ldy=n * dh - 1), dict(B=0), dict(T=0), dict(NH=0),
           dict(dh=0), dict(max_pos=0), dict(T=3, max_pos=2), dict(B=-1)]
    for change in bad:
        a = dict(good, **change)
        for op in ("fwd", "bwd", "bwd_assign"):
            X, Y = Guarded(dev, x, 4), Guarded(dev, mark, 4)
            with pytest.raises(c.NeuronikaHipError):
                if op == "fwd":
                    c.rope_fwd(dev, X.body, a["ldx"], Y.body, a["ldy"], tab.body, None, a["B"], a["T"], a["NH"], a["dh"], a["rot"], a["max_pos"], False)
                else:
                    c.rope_bwd(dev, Y.body, a["ldy"], X.body, a["ldx"], tab.body, None, a["B"], a["T"], a["NH"], a["dh"], a["rot"], a["max_pos"], False,
                               assign=op == "bwd_assign")
            same_bits(Y.numpy(), mark, "%s %s wrote" % (op, change))
            same_bits(X.numpy(), x, "%s %s wrote its input" % (op, change))
    X = Guarded(dev, x, 4)
    with pytest.raises(c.NeuronikaHipError):                             # dx == g is legal for the assign form only
        c.rope_bwd(dev, X.body, n * dh, X.body, n * dh, tab.body, None, B, T, n, dh, 8, MAX_POS, False)
    same_bits(X.numpy(), x, "+= in place wrote")
    # T > max_pos is legal with a start array: the kernel clamps
    Y = Guarded(dev, mark, 4)
    c.rope_fwd(dev, X.body, n * dh, Y.body, n * dh, tab.body, dev.int_array(np.zeros(B, np.int32)), B, T, n, dh, 8, 2, False)
    for bad_table in (dict(max_pos=0, rot=8), dict(max_pos=4, rot=7), dict(max_pos=4, rot=0)):
        with pytest.raises(c.NeuronikaHipError):
            c.rope_table(dev, tab.body, bad_table["max_pos"], bad_table["rot"])
    with pytest.raises(c.NeuronikaHipError):
        c.rope_table(dev, tab.body, 4, 8, -1.0)
    tab.numpy()
