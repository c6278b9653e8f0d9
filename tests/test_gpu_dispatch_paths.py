"""Parity of the streaming kernels at every branch their dispatchers can take (tests/dispatch_paths.py is the inventory).

The entry points of nk_elementwise / nk_reduce / nk_layout / nk_loss / nk_gemv look at extents, strides, pointer alignment and
bytes touched and launch one of several kernels, each with unrolled loops and tail tiers.  The grids below are read off those
conditions: threshold t -> t - 1, t, t + 1; unroll factor u -> extents 0 .. u mod u.  Every case

  * is compared with a NumPy float64 restatement (oracle/neuronika_oracle.py where it has one);
  * pointwise results: rtol 1e-5 / atol 1e-6; anything that sums R terms: tolerance.assert_contraction with K = R and the
    operands' real maxima; pure data movement: np.array_equal;
  * `+=` starts from a random destination, its `_assign` twin from NaN and must equal `+=` into zeros bit for bit;
  * the destination is a window inside a larger allocation whose neighbours hold a sentinel pattern that must survive;
  * reductions run twice and must repeat bit for bit (fixed order, no atomics);
  * inputs depend on the flat index (a swapped row or lane changes the result), plus seeded noise.

All calls go through neuronika_amd.capi.  Only host-side rejections are provoked; no kernel is handed an extent or a pointer
it would fault on.  Three groups are large (marked LARGE): the cases past the 384 MiB cache switch, the sub-block planes
around 2^23 elements and the pad plane above it; no tensor exceeds 256 MiB."""
import re

import numpy as np
import pytest

import tolerance
from oracle import neuronika_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 16                       # sentinel floats on either side of a destination window (64 bytes: alignment is kept)
SENTINEL = np.uint32(0xDEADBEEF)
RTOL, ATOL = tolerance.ELEMENTWISE_RTOL, tolerance.ELEMENTWISE_ATOL


def capi():
    from neuronika_amd import capi as c
    return c


def numel(shape):
    return int(np.prod(shape, dtype=np.int64)) if len(shape) else 1


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def pattern(seed, shape, lo=-1.0, hi=1.0):
    """seeded noise in [lo, hi) plus a ramp over the flat index: two swapped rows, or a lane reading its neighbour's
    element, change a sum instead of cancelling in it"""
    n = numel(shape)
    noise = np.random.default_rng(seed).random(n, dtype=np.float32)
    ramp = ((np.arange(n, dtype=np.int64) * 2654435761 >> 7) % 1021).astype(np.float32) / np.float32(1021)
    v = (np.float32(0.75) * noise + np.float32(0.25) * ramp) * np.float32(hi - lo) + np.float32(lo)
    return v.astype(np.float32).reshape(shape)


def away_from_zero(a, eps=0.25):
    return np.where(a >= 0, a + np.float32(eps), a - np.float32(eps)).astype(np.float32)


def view(base, first, shape):
    """`shape`d alias `first` floats into the allocation `base`"""
    v = base.view_offset(first)
    v.shape, v.size = tuple(int(s) for s in shape), numel(shape)
    return v


def put(dev, a, off=0):
    """upload `a`; off > 0: at `off` floats past a 16-byte boundary (an operand the float4 kernels cannot take)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if off == 0 and a.size:
        return dev.array(a)
    base = dev.array(np.concatenate([np.zeros(off, np.float32), a.reshape(-1), np.zeros(1, np.float32)]))
    return view(base, off, a.shape)


class Window:
    """a destination of `shape` holding `init`, `off` floats past a 16-byte boundary, between two sentinel runs"""

    def __init__(self, dev, shape, init, off=0):
        self.shape, self.n, self.first = tuple(shape), numel(shape), GUARD + off
        host = np.full(self.first + self.n + GUARD, 0, np.uint32)
        host[:] = SENTINEL
        host[self.first:self.first + self.n] = bits(np.broadcast_to(np.asarray(init, np.float32), self.shape)).reshape(-1)
        self.base = dev.array(host.view(np.float32))
        self.v = view(self.base, self.first, self.shape)

    def read(self):
        host = bits(self.base.numpy())
        assert (host[:self.first] == SENTINEL).all(), "cells BEFORE the destination were written"
        assert (host[self.first + self.n:] == SENTINEL).all(), "cells AFTER the destination were written"
        return host[self.first:self.first + self.n].view(np.float32).reshape(self.shape).copy()


def close(got, ref):
    np.testing.assert_allclose(np.asarray(got, np.float64), np.asarray(ref, np.float64), rtol=RTOL, atol=ATOL)


def check(label, got, ref64, K=None, amax=1.0, bmax=1.0, scale=1.0):
    """pointwise bound (K None) or the contraction bound over K summed terms, plus the pointwise bound for the arithmetic
    after the sum"""
    if K is None or K <= 1:
        close(got, ref64)
    else:
        assert np.isfinite(np.asarray(got)).all(), label
        tolerance.assert_contraction(label, got, ref64, K, amax, bmax, scale=scale, epilogue=True)


def accumulate_forms(dev, shape, launch, inc64, label, K=None, amax=1.0, bmax=1.0, off=0, exact=False, seed=0, has_assign=True,
                     repeat=True):
    """launch(dst, assign) through `+=` into a random destination, `+=` into zeros (twice: determinism) and the assign twin
    into NaN; returns the `+=`-into-zeros result"""
    d0 = pattern(seed + 991, shape, -2.0, 2.0)
    w = Window(dev, shape, d0, off); launch(w.v, False); got = w.read()
    z = Window(dev, shape, 0.0, off); launch(z.v, False); zero = z.read()
    if repeat:
        z2 = Window(dev, shape, 0.0, off); launch(z2.v, False)
        assert same_bits(z2.read(), zero), f"{label}: two runs differ"
    if has_assign:
        a = Window(dev, shape, np.nan, off); launch(a.v, True)
        assert same_bits(a.read(), zero), f"{label}: assign differs from += into zeros"
    if exact:
        assert np.array_equal(zero, np.asarray(inc64, np.float32)), label
        assert np.array_equal(got, d0 + np.asarray(inc64, np.float32)), label     # one f32 add per element
    else:
        check(label, zero, inc64, K, amax, bmax)
        check(label, got, d0.astype(np.float64) + inc64, K, amax, bmax)
    return zero


def rejected(fn, *a, **k):
    with pytest.raises(capi().NeuronikaHipError):
        fn(*a, **k)


# ======================================================================================================================
# binary forward
# ======================================================================================================================
OPS = ("add", "sub", "mul", "div")
BINARY_FWD = [
    # (id, left shape, right shape, float offsets of (out, l, r))                       branch
    ("vec", (33, 260), (33, 260), (0, 0, 0)),                 # <OP, true>, one collapsed dim, span-walk tail (2145 quads)
    ("vec_small", (1, 4), (1, 4), (0, 0, 0)),                 # <OP, true>, a single quad
    ("splat_l", (5, 1), (5, 1028), (0, 0, 0)),                # <OP, true>, ld4 of the left operand with inner stride 0
    ("splat_r", (37, 256), (37, 1), (0, 0, 0)),               # <OP, true>, ld4 of the right operand with inner stride 0
    ("row_bcast", (260,), (31, 260), (0, 0, 0)),              # <OP, true>, outer stride 0, inner stride 1
    ("inner17", (37, 17), (37, 17), (0, 0, 0)),               # <OP, false>: inner extent % 4 != 0
    ("inner1", (100, 1), (1, 3), (0, 0, 0)),                  # <OP, false>: both operands broadcast, inner extent 3
    ("scalar_r", (5, 252), (), (0, 0, 0)),                    # <OP, true>, right operand a 0-d tensor (all strides 0)
    ("one", (1,), (1,), (0, 0, 0)),                           # <OP, false>, one element
] + [   # <OP, false> because one of out / l / r sits 1, 2 or 3 floats past a 16-byte boundary, each in turn
    (f"off_{w}{k}", (33, 260), (33, 260), tuple(k if i == j else 0 for i in range(3))) for j, w in enumerate(("out", "l", "r")) for k in (1, 2, 3)
]


@pytest.mark.parametrize("case", BINARY_FWD, ids=[c[0] for c in BINARY_FWD])
@pytest.mark.parametrize("op", OPS)
def test_binary_fwd(dev, op, case):
    c = capi()
    _, ls, rs, (oo, lo, ro) = case
    l, r = pattern(1, ls, -2, 2), away_from_zero(pattern(2, rs, -2, 2))
    out_shape = O.cobroadcast(tuple(ls), tuple(rs))
    ref = np.zeros(out_shape)
    O.binary_forward(op, l.astype(np.float64), r.astype(np.float64), ref)
    w = Window(dev, out_shape, np.nan, oo)
    c.binary_fwd(dev, op, w.v, put(dev, l, lo), put(dev, r, ro))
    got = w.read()
    close(got, ref)
    if oo or lo or ro:                                            # the scalar kernel against the float4 kernel
        a = Window(dev, out_shape, np.nan, 0)
        c.binary_fwd(dev, op, a.v, put(dev, l), put(dev, r))
        close(got, a.read())


# ======================================================================================================================
# binary backward / un-broadcast: bwd_dispatch<MODE>
# ======================================================================================================================
# MODE of bwd_dispatch -> the (op, side) that reaches it: 0 g, 1 -g, 2 g * o, 3 g / o, 4 -g * o / q^2
MODES = {0: ("add", "left"), 1: ("sub", "right"), 2: ("mul", "left"), 3: ("div", "left"), 4: ("div", "right")}

# (id, gradient shape, target shape, operand shape or None = gradient shape, offsets (d, g, o, q))
BWD_SAME = [
    ("same_vec", (33, 260), (33, 260), None, (0, 0, 0)),          # binary_bwd_same<M, true>
    ("same_quad", (4,), (4,), None, (0, 0, 0)),                   # ... one quad
    ("same_17", (37, 17), (37, 17), None, (0, 0, 0)),             # binary_bwd_same<M, false>: total % 4 != 0
    ("same_row_o", (31, 260), (31, 260), (260,), (0, 0, 0)),      # <M, true>, operand broadcast over rows (outer stride 0)
    ("same_splat_o", (5, 1028), (5, 1028), (5, 1), (0, 0, 0)),    # <M, true>, ld4 of the operand with inner stride 0
]
# <M, false> because d, g, o (MODE >= 2) or q (MODE 4) sits 1, 2 or 3 floats past a 16-byte boundary, each in turn
BWD_SAME += [(f"same_off_{w}{k}", (33, 260), (33, 260), None, tuple(k if i == j else 0 for i in range(4))) for j, w in enumerate("dgoq")
             for k in (1, 2, 3)]
# column reductions [R0][K] -> [K]: reduce_cols4 (MODE <= 1, K % 4 == 0, g aligned) or reduce_cols, then reduce_finish
BWD_COLS = [
    ("cols_1x4", (1, 4), (4,)),            # R0 = 1 -> no reduced extent: same-shape kernel after the collapse
    ("cols_3x4", (3, 4), (4,)),            # cols4 third tier only (rows_per_chunk 3); cols: tail of 3 after no unrolled trip
    ("cols_5x252", (5, 252), (252,)),      # cols4 tiers two and three in one chunk; K < 256: `k < p.K` guard; cols: 4 + 1
    ("cols_31x256", (31, 256), (256,)),    # one chunk of 31 rows: cols4 tier two, lanes with 7 and 8 rows; cols: 28 + 3
    ("cols_32x260", (32, 260), (260,)),    # R0 = 32 exactly, K = 256 + 4: second column block nearly empty; cols4 tier one
    ("cols_33x17", (33, 17), (17,)),       # R0 = 32 + 1: two chunks (17 + 16); K % 4 != 0 -> reduce_cols for every MODE
    ("cols_37x256", (37, 256), (256,)),    # two chunks of 19 / 18 rows: tiers two and three
    ("cols_100x1028", (100, 1028), (1028,)),   # four chunks of 25; five column blocks, the last with 4 columns
    ("cols_1000x260", (1000, 260), (260,)),    # 32 chunks of 32 rows (last 8): tier one; finish: 32 chunks, two full trips
    ("cols_4097x4", (4097, 4), (4,)),      # 129 chunks (last 1 row): finish with 129 = 16 * 8 + 1 chunks; K one quad
    ("cols_1000x1", (1000, 1), (1,)),      # K = 1 -> scalar target after the collapse (R1 = 8)
    ("cols_37x17_keep", (37, 17), (1, 17)),    # target keeps the reduced axis with extent 1
    ("cols_off_g1", (37, 256), (256,)),    # g offset by one, two, three floats: cols4 refused -> reduce_cols<0|1>
    ("cols_off_g2", (37, 256), (256,)),
    ("cols_off_g3", (37, 256), (256,)),
    ("cols_off_d1", (37, 256), (256,)),    # the target offset: reduce_finish writes scalars, cols4 stays
    ("cols_3d", (5, 7, 252), (252,)),      # two leading axes collapse into R0 = 35
]
# [K][R1] -> [K][1] and [R0][K][R1] -> [K][1]: reduce_rkr (vector when R1 % 4 == 0 and aligned), then reduce_finish
BWD_RKR = [
    ("rows_17x30", (17, 30), (17, 1), None),            # R0 = 1, scalar loop, R1 < 256
    ("rows_252x64", (252, 64), (252, 1), None),         # vector loop, one quad per lane for 16 lanes
    ("rows_4x1028", (4, 1028), (4, 1), None),           # vector loop, second trip for one lane (1028 = 1024 + 4)
    ("rkr_3x5x4", (3, 5, 4), (5, 1), None),             # R1 == 4: one lane per row
    ("rkr_2x3x30", (2, 3, 30), (3, 1), None),           # R1 % 4 != 0 (the suite's old case)
    ("rkr_5x17x64", (5, 17, 64), (17, 1), None),        # chunks = R0 (1024 / K > R0): one row per chunk
    ("rkr_33x4x1024", (33, 4, 1024), (4, 1), None),     # R1 == 1024: exactly one trip for all 256 lanes
    ("rkr_3x4x3136", (3, 4, 3136), (4, 1), None),       # several trips with a ragged last one (3136 = 3 * 1024 + 64)
    ("rkr_conv_bias", (3, 5, 56, 56), (5, 1, 1), None),     # (N, C, H, W) -> (C, 1, 1), H * W % 4 == 0: the conv bias gradient
    ("rkr_1000x4x4", (1000, 4, 4), (4, 1), None),       # 256 chunks of 4 rows (last of 4): finish with many chunks
    ("rkr_splat_o", (5, 17, 64), (17, 1), (5, 17, 1)),  # operand inner stride 0: ld4 splat in the vector loop
    ("rkr_off_g1", (5, 17, 64), (17, 1), None),         # g offset by one, two, three floats: scalar loop although R1 % 4 == 0
    ("rkr_off_g2", (5, 17, 64), (17, 1), None),
    ("rkr_off_g3", (5, 17, 64), (17, 1), None),
    ("rkr_off_o1", (5, 17, 64), (17, 1), None),         # the operand offset (MODE >= 2): scalar loop
    ("rkr_off_o2", (5, 17, 64), (17, 1), None),
    ("rkr_off_o3", (5, 17, 64), (17, 1), None),
    ("rkr_off_q2", (5, 17, 64), (17, 1), None),         # the divisor offset (MODE 4): scalar loop
    ("rkr_off_d3", (5, 17, 64), (17, 1), None),         # the target offset: the vector loop stays
    ("rkr_bcast_o", (2, 3, 4), (1, 3, 1), (2, 1, 4)),   # the operand is broadcast along the kept axis (osk = 0)
    ("rkr_1300x3x4", (1300, 3, 4), (3, 1), None),       # chunks capped by ceil(1024 / K) = 342 -> 4 rows per chunk, 325 chunks
]
BWD_SCALAR = [
    ("scalar_7x5", (7, 5), (), None),                   # odd total: R1 = 1 -> the column kernels with K = 1
    ("scalar_1", (1,), (), None),                       # one element: nothing reduced, same-shape kernel
    ("scalar_3x8192", (3, 8192), (), None),             # R1 = 8192: eight trips of the vector loop, R0 = 3
    ("scalar_4097x4", (4097, 4), (1,), None),           # R1 = 4, R0 = 4097 -> 1024 chunks of 5 rows (last of 2)
    ("scalar_nd2", (7, 12), (), (12,)),                 # the operand's broadcast stops the collapse: nd != 1 -> generic (MODE >= 2)
]
BWD_GENERIC = [
    ("generic_krkr", (3, 5, 4, 6), (3, 1, 4, 1), None),     # two kept groups
    ("generic_rkrk", (3, 5, 4, 6), (5, 1, 6), None),        # reduced - kept - reduced - kept
    ("generic_rank6", (2, 3, 2, 3, 2, 5), (3, 1, 3, 1, 5), None),   # more than three collapsed dims
]


def _bwd_case(dev, mode, gshape, tshape, oshape, offs, label):
    c = capi()
    op, side = MODES[mode]
    oshape = gshape if oshape is None else oshape
    do, go, oo, qo = (tuple(offs) + (0,))[:4]
    g = pattern(11, gshape, -1, 1)
    o = away_from_zero(pattern(12, oshape, -2, 2))
    if mode == 4:      # div right: the target operand r = q has the target's shape, o = l
        q = away_from_zero(pattern(13, tshape, -2, 2), 0.5)
    g64, o64 = g.astype(np.float64), o.astype(np.float64)
    if mode == 0: local, fac = g64 + 0, 1.0
    elif mode == 1: local, fac = -g64, 1.0
    elif mode == 2: local, fac = g64 * o64, np.abs(o64).max()
    elif mode == 3: local, fac = g64 / o64, (1 / np.abs(o64)).max()
    else:
        q64 = q.astype(np.float64)
        f = np.broadcast_to(o64, gshape) / np.broadcast_to(q64.reshape((1,) * (len(gshape) - q64.ndim) + q64.shape) ** 2, gshape)
        local, fac = -g64 * f, np.abs(f).max()
    local = np.broadcast_to(local, gshape)
    inc = np.zeros(tshape)
    O.accumulate(inc, np.array(local))
    K = numel(gshape) // max(1, numel(tshape))
    G, Oo = put(dev, g, go), put(dev, o, oo)
    Q = put(dev, q, qo) if mode == 4 else None

    def launch(dst, assign):
        if side == "left":
            c.binary_bwd_left(dev, op, dst, G, Oo if mode >= 2 else None, assign=assign)
        elif mode == 1:
            c.binary_bwd_right(dev, op, dst, G, None, None, assign=assign)
        else:
            c.binary_bwd_right(dev, op, dst, G, Oo, Q, assign=assign)

    return accumulate_forms(dev, tshape, launch, inc, label, K, np.abs(g64).max(), fac, off=do, seed=mode)


def _offs(cid):
    """ids ending in _off_<d|g|o|q><k>: that operand k floats past a 16-byte boundary"""
    m = re.search(r"_off_([dgoq])([123])$", cid)
    return tuple(int(m.group(2)) if m and "dgoq"[i] == m.group(1) else 0 for i in range(4))


def _mode_cases(cases):
    """(mode, case) pairs; a case with an operand shape of its own exists for the modes that read an operand only"""
    reads = lambda m, cid: not ((m < 2 and re.search(r"_off_o\d$", cid)) or (m < 4 and re.search(r"_off_q\d$", cid)))
    return [pytest.param(m, c, id=f"m{m}-{c[0]}") for m in sorted(MODES) for c in cases if (m >= 2 or c[3] is None) and reads(m, c[0])]


@pytest.mark.parametrize("mode,case", _mode_cases(BWD_SAME))
def test_binary_bwd_same(dev, mode, case):
    cid, gs, ts, os_, offs = case
    _bwd_case(dev, mode, gs, ts, os_, offs, f"dispatch/binary_bwd_same/{cid}/m{mode}")


@pytest.mark.parametrize("mode,case", _mode_cases([c + (None,) for c in BWD_COLS]))
def test_binary_bwd_cols(dev, mode, case):
    cid, gs, ts, _ = case
    _bwd_case(dev, mode, gs, ts, None, _offs(cid), f"dispatch/binary_bwd_cols/{cid}/m{mode}")


@pytest.mark.parametrize("mode,case", _mode_cases(BWD_RKR + BWD_SCALAR + BWD_GENERIC))
def test_binary_bwd_reduce(dev, mode, case):
    cid, gs, ts, os_ = case
    _bwd_case(dev, mode, gs, ts, os_, _offs(cid), f"dispatch/binary_bwd_reduce/{cid}/m{mode}")


UNBROADCAST = [
    ("same", (33, 260), (33, 260)),              # binary_bwd_same<0, true>
    ("cols4_tiers", (37, 256), (256,)),          # reduce_cols4<0> tiers two and three
    ("cols", (33, 17), (17,)),                   # reduce_cols<0>
    ("bias", (3, 5, 56, 56), (5, 1, 1)),         # reduce_rkr<0>, vector
    ("scalar", (3, 8192), ()),                   # R1 = 8192
    ("rank8", (2, 1, 3, 2, 1, 2, 3, 4), (3, 1, 1, 2, 1, 4)),   # the maximum rank; generic
]


@pytest.mark.parametrize("case", UNBROADCAST, ids=[c[0] for c in UNBROADCAST])
def test_unbroadcast(dev, case):
    c = capi()
    cid, ss, ds = case
    src = pattern(21, ss, -1, 1)
    inc = np.zeros(ds)
    O.accumulate(inc, src.astype(np.float64))
    S = put(dev, src)
    accumulate_forms(dev, ds, lambda d, assign: c.unbroadcast_add(dev, d, S, assign=assign), inc, f"dispatch/unbroadcast/{cid}",
                     numel(ss) // numel(ds), np.abs(src).max(), 1.0)


# ======================================================================================================================
# softmax / log-softmax
# ======================================================================================================================
def _softmax_ref(log, x64, axis):
    y = np.zeros_like(x64)
    with np.errstate(divide="ignore"):
        (O.log_softmax_forward if log else O.softmax_forward)(x64, y, axis)
    return y


def _softmax_case(dev, log, x, axis, label, offs=(0, 0, 0), backward=True):
    c = capi()
    fwd, bwd = (c.log_softmax_fwd, c.log_softmax_bwd) if log else (c.softmax_fwd, c.softmax_bwd)
    shape, L = x.shape, x.shape[axis]
    x64 = x.astype(np.float64)
    y64 = _softmax_ref(log, x64, axis)
    finite = np.isfinite(x64)
    xmax = max(1.0, float(np.abs(x64[finite]).max())) if finite.any() else 1.0
    X = put(dev, x, offs[1])
    w = Window(dev, shape, np.nan, offs[0]); fwd(dev, X, w.v, axis); y = w.read()
    w2 = Window(dev, shape, np.nan, offs[0]); fwd(dev, X, w2.v, axis)
    assert same_bits(w2.read(), y), f"{label}: two forward runs differ"
    ok = np.isfinite(y64)
    assert np.array_equal(y[~ok], y64[~ok].astype(np.float32)), label          # -inf stays -inf
    if log: tolerance.assert_contraction(label + "/fwd", y[ok], y64[ok], L, xmax, 1.0, epilogue=True)
    else: tolerance.assert_contraction(label + "/fwd", y[ok], y64[ok], L, 1.0, float(np.abs(y64).max()), epilogue=True)
    if not backward:
        return y
    # backward on the oracle's f64 output rounded to f32 (what the node keeps), an independent gradient
    yk = y64.astype(np.float32)
    g = pattern(31, shape, -1, 1)
    inc = np.zeros(shape)
    (O.log_softmax_backward if log else O.softmax_backward)(inc, g.astype(np.float64), yk.astype(np.float64), axis)
    G, Y = put(dev, g, offs[2]), put(dev, yk, offs[1])
    accumulate_forms(dev, shape, lambda d, assign: bwd(dev, d, G, Y, axis, assign=assign), inc, label + "/bwd", L,
                     float(np.abs(g).max()), 1.0 if log else float(np.abs(yk).max()), off=offs[0])
    return y


# L: 1, 2 (block kernel, a row shorter than a quad); 4 (row<1>, one lane); 60 / 64 / 68 (lanes past the row: 15, 16, 17 of 64 in
# use); 252 / 256 / 260 (row<1> full, row<2> begins); 512 / 516 (row<2> -> row<4>); 1024 / 1028 (row<4> -> row<8>); 2044 / 2048 (row<8>
# full); 2052 (block kernel because L > 2048); 3000 / 5000 (block kernel, 12 and 20 trips, ragged); 1023 / 255 (block, L % 4 != 0)
SOFTMAX_L = (1, 2, 4, 60, 64, 68, 252, 255, 256, 260, 512, 516, 1023, 1024, 1028, 2044, 2048, 2052, 3000, 5000)
# outer: 1, 3, 4, 5 (a block holds 4 rows: part of one block, one block exactly, one row into the second), 33
SOFTMAX_ROWS = [(L, 5) for L in SOFTMAX_L] + [(L, o) for L in (64, 260, 1028, 2048, 3000) for o in (1, 3, 4, 33)]


@pytest.mark.parametrize("L,outer", SOFTMAX_ROWS, ids=[f"L{L}-o{o}" for L, o in SOFTMAX_ROWS])
@pytest.mark.parametrize("log", (False, True), ids=("soft", "log"))
def test_softmax_rows(dev, log, L, outer):
    _softmax_case(dev, log, pattern(L * 7 + outer, (outer, L), -3, 3), 1, f"dispatch/softmax_rows/{'log' if log else 'soft'}/L{L}")


# a row of L % 4 == 0 takes the block kernel when one pointer is not 16-byte aligned (offsets of dx|y, x|y-kept, g)
SOFTMAX_OFFSETS = [(f"{w}{k}", tuple(k if i == j else 0 for i in range(3))) for j, w in enumerate(("dst", "src", "g")) for k in (1, 2, 3)]
SOFTMAX_OFFSETS.append(("all", (3, 1, 2)))


@pytest.mark.parametrize("which,offs", SOFTMAX_OFFSETS, ids=[w for w, _ in SOFTMAX_OFFSETS])
@pytest.mark.parametrize("log", (False, True), ids=("soft", "log"))
def test_softmax_offset(dev, log, which, offs):
    x = pattern(41, (5, 256), -3, 3)
    y = _softmax_case(dev, log, x, 1, f"dispatch/softmax_offset/{'log' if log else 'soft'}", offs)
    a = _softmax_case(dev, log, x, 1, "", backward=False)
    close(y, a)                                                    # row kernel and block kernel: same value within the bound


# the strided kernel: (shape, axis); inner = 1 as axis 0 of a 2-D tensor goes to the row / block kernels with outer = 1
SOFTMAX_STRIDED = [
    ("axis0_inner1", (64, 1), 0),          # inner == 1, outer == 1 -> row<1>
    ("axis0_inner12", (17, 12), 0),        # strided, one outer, 12 lanes
    ("mid_inner12", (3, 17, 12), 1),       # strided, id / inner and id % inner both in use
    ("long_inner1000", (3, 17, 1000), 1),  # a long inner extent: 3000 lanes, 12 blocks, the last one ragged
    ("axis0_long_L", (3000, 5), 0),        # a long lane walked with stride 5
    ("rank4_axis2", (2, 3, 5, 7), 2),
]


@pytest.mark.parametrize("case", SOFTMAX_STRIDED, ids=[c[0] for c in SOFTMAX_STRIDED])
@pytest.mark.parametrize("log", (False, True), ids=("soft", "log"))
def test_softmax_strided(dev, log, case):
    cid, shape, axis = case
    _softmax_case(dev, log, pattern(51, shape, -3, 3), axis, f"dispatch/softmax_strided/{'log' if log else 'soft'}/{cid}")


@pytest.mark.parametrize("L", (5, 64, 260, 1028, 2052), ids=lambda L: f"L{L}")       # block, row<1>, row<2>, row<8>, block
@pytest.mark.parametrize("log", (False, True), ids=("soft", "log"))
def test_softmax_extremes(dev, log, L):
    """the max subtraction: large magnitudes, all-equal rows, -inf entries (forward only: the oracle defines those results)"""
    x = np.empty((6, L), np.float32)
    x[0] = np.linspace(-1e4, 1e4, L, dtype=np.float32)            # exp(x) alone would overflow / underflow
    x[1] = 1e4                                                    # all equal, large
    x[2] = -1e4
    x[3] = 0.0
    x[4] = pattern(61, (L,), -3, 3); x[4, ::3] = -np.inf          # masked entries: probability 0, log-probability -inf
    x[5] = -np.inf; x[5, L // 2] = 2.0                            # one live entry
    y = _softmax_case(dev, log, x, 1, f"dispatch/softmax_extremes/{'log' if log else 'soft'}", backward=False)
    if not log:
        assert np.array_equal(y[1], np.full(L, np.float32(1) / np.float32(L)))
        assert y[5, L // 2] == 1.0 and y[5].sum() == 1.0


# ======================================================================================================================
# fused attention probabilities (scale, softmax, dropout in one row kernel; nk_reduce.hip)
# ======================================================================================================================
@pytest.mark.parametrize("L", (4, 256, 260, 516, 1028, 2048), ids=lambda L: f"L{L}")     # V = 1, 1, 2, 4, 8, 8
def test_attn_probs(dev, L):
    c = capi()
    rows, scale, p, seed, offset = 5, 0.125, 0.3, 77, 5
    s = pattern(71, (rows, L), -8, 8)
    g = pattern(72, (rows, L), -1, 1)
    y64 = _softmax_ref(False, s.astype(np.float64) * scale, 1)
    noise = O.dropout_noise(rows * L, p, seed, offset).reshape(rows, L)
    dscale = 1.0 / (1.0 - p)
    S, G = put(dev, s), put(dev, g)

    def fwd(p_, train, with_noise, with_probs=True):
        P, Ow, N = Window(dev, (rows, L), np.nan), Window(dev, (rows, L), np.nan), Window(dev, (rows, L), np.nan)
        c.scale_softmax_dropout_fwd(dev, S, P.v if with_probs else None, Ow.v, N.v if with_noise else None, scale, p_, train, seed, offset)
        return P.read(), Ow.read(), N.read()

    lab = f"dispatch/attn_probs/L{L}"
    probs, out, _ = fwd(0.0, True, False)                         # <V, 0, false>
    tolerance.assert_contraction(lab + "/probs", probs, y64, L, 1.0, float(y64.max()), epilogue=True)
    assert same_bits(out, probs)
    _, out_e, _ = fwd(p, False, False, with_probs=False)          # evaluation mode, probabilities not stored
    assert same_bits(out_e, probs)
    _, out1, _ = fwd(1.0, True, False)                            # <V, 2, false>
    assert np.array_equal(out1, np.zeros((rows, L), np.float32))
    pm, om, nz = fwd(p, True, True)                               # <V, 1, true>
    assert same_bits(pm, probs) and np.array_equal(nz, noise)
    tolerance.assert_contraction(lab + "/out", om, y64 * noise * dscale, L, 1.0, float(y64.max()) * dscale, epilogue=True)
    _, om2, _ = fwd(p, True, False)                               # <V, 1, false>
    assert same_bits(om2, om)

    Pk, Nz = put(dev, probs), put(dev, noise)
    pk64 = probs.astype(np.float64)
    for masked, p_, train in ((False, 0.0, True), (True, p, True), (True, 1.0, True)):
        nm = noise if p_ == p else (np.zeros_like(noise) if p_ == 1.0 else np.ones_like(noise))
        gp = g.astype(np.float64) * nm
        inc = pk64 * (gp - (gp * pk64).sum(axis=1, keepdims=True)) * scale
        amax = float(np.abs(g).max())
        for with_noise in ((False, True) if masked and p_ == p else (False,)):
            noise_arg = Nz if with_noise else None
            z = accumulate_forms(dev, (rows, L), lambda d, a: c.scale_softmax_dropout_bwd(dev, d, G, Pk, noise_arg, scale, p_, train, seed, offset, assign=a),
                                 inc, f"{lab}/bwd", L, amax, float(pk64.max()))
            # recomputing form: the probabilities are rebuilt from the scores with the forward kernel's sequence
            zr = accumulate_forms(dev, (rows, L), lambda d, a: c.scale_softmax_dropout_bwd_from_scores(dev, d, G, S, noise_arg, scale, p_, train, seed, offset, assign=a),
                                  inc, f"{lab}/bwd_recompute", L, amax, float(pk64.max()))
            assert same_bits(z, zr)


@pytest.mark.parametrize("L", (4, 260, 1028, 2048), ids=lambda L: f"L{L}")               # V = 1, 2, 8, 8
def test_attn_probs_extremes(dev, L):
    """the max subtraction of the fused kernel and of the backward that recomputes from the scores, held against `_softmax_ref` as
    test_softmax_extremes holds the plain kernels: test_attn_probs draws scaled scores in [-1, 1), where any shift - or none - gives
    the same probabilities"""
    c = capi()
    rows, scale, seed, offset = 5, 0.125, 77, 5
    s = np.empty((rows, L), np.float32)
    s[0] = np.linspace(-1e4, 1e4, L, dtype=np.float32) / np.float32(scale)   # exp(x) alone would overflow / underflow
    s[1] = 1e4 / scale                                                        # all equal, large
    s[2] = -np.inf; s[2, L // 2] = 2.0 / scale                                # one live entry among -inf
    s[3] = pattern(62, (L,), -3, 3) / np.float32(scale); s[3, 4:] -= np.float32(1e3 / scale)     # the maximum in the first lane only
    s[4] = -1e4 / scale
    y64 = _softmax_ref(False, s.astype(np.float64) * scale, 1)
    assert np.isfinite(y64).all() and (L == 4 or y64[3, 4:].max() == 0.0)
    S = put(dev, s)
    lab = f"dispatch/attn_probs_extremes/L{L}"
    P, Ow = Window(dev, (rows, L), np.nan), Window(dev, (rows, L), np.nan)
    c.scale_softmax_dropout_fwd(dev, S, P.v, Ow.v, None, scale, 0.0, True, seed, offset)
    probs, out = P.read(), Ow.read()
    assert np.isfinite(probs).all(), lab
    tolerance.assert_contraction(lab + "/probs", probs, y64, L, 1.0, float(y64.max()), epilogue=True)
    assert same_bits(out, probs)
    for r in (1, 4):
        assert np.array_equal(probs[r], np.full(L, np.float32(1) / np.float32(L)))
    assert probs[2, L // 2] == 1.0 and probs[2].sum() == 1.0
    g = pattern(72, (rows, L), -1, 1)
    G = put(dev, g)
    inc = y64 * (g - (g * y64).sum(axis=1, keepdims=True)) * scale
    zr = accumulate_forms(dev, (rows, L), lambda d, a: c.scale_softmax_dropout_bwd_from_scores(dev, d, G, S, None, scale, 0.0, True, seed, offset, assign=a),
                          inc, lab + "/bwd_recompute", L, float(np.abs(g).max()), float(y64.max()))
    Pk = put(dev, probs)
    z = accumulate_forms(dev, (rows, L), lambda d, a: c.scale_softmax_dropout_bwd(dev, d, G, Pk, None, scale, 0.0, True, seed, offset, assign=a),
                         probs.astype(np.float64) * (g - (g * probs.astype(np.float64)).sum(axis=1, keepdims=True)) * scale,
                         lab + "/bwd", L, float(np.abs(g).max()), float(y64.max()))
    assert same_bits(z, zr)


# ======================================================================================================================
# full reductions and their backward
# ======================================================================================================================
# n: 1 .. 5 (below and around one quad), 255 / 256 / 257 (quads of a partial wave), 1025 (one block of 256 quads + 1),
# 2^20 + 3 (the grid reaches MAX_PART = 1024 blocks: several quads per lane, tail of 3)
REDUCE_N = (1, 2, 3, 4, 5, 255, 256, 257, 1025, (1 << 20) + 3)
REDUCE_N_LARGE = REDUCE_N + ((1 << 24) + 1,)      # LARGE: 64 MiB per operand; 16 trips of the 4-way unrolled span walk per lane


@pytest.mark.parametrize("n", REDUCE_N_LARGE, ids=lambda n: f"n{n}")
@pytest.mark.parametrize("kind", ("sum", "mean", "mse_sum", "mse_mean"))
def test_full_reduce(dev, kind, n):
    c = capi()
    x, t = pattern(81, (n,), -1, 1), pattern(82, (n,), -1, 1)
    x64, t64 = x.astype(np.float64), t.astype(np.float64)
    X, T = put(dev, x), put(dev, t)
    red = "mean" if kind.endswith("mean") else "sum"
    term = x64 if kind in ("sum", "mean") else (x64 - t64) ** 2
    ref = term.sum() / (n if red == "mean" else 1)
    outs = []
    for _ in range(2):
        w = Window(dev, (1,), np.nan)
        if kind == "sum": c.sum_fwd(dev, X, w.v)
        elif kind == "mean": c.mean_fwd(dev, X, w.v)
        else: c.mse_fwd(dev, X, T, w.v, red)
        outs.append(w.read())
    assert same_bits(outs[0], outs[1])
    check(f"dispatch/full_reduce/{kind}", outs[0], np.array([ref]), n, float(np.abs(term).max()), 1.0, scale=1.0 / n if red == "mean" else 1.0)
    gs = np.float32(0.75)
    Gs = put(dev, np.array([gs]))
    den = n if red == "mean" else 1
    inc = (np.full(n, float(gs)) if kind in ("sum", "mean") else 2.0 * (x64 - t64) * float(gs)) / den

    def launch(d, assign):
        if kind == "sum": c.sum_bwd(dev, d, Gs, assign=assign)
        elif kind == "mean": c.mean_bwd(dev, d, Gs, assign=assign)
        else: c.mse_bwd(dev, d, Gs, X, T, red, assign=assign)
    accumulate_forms(dev, (n,), launch, inc, f"dispatch/full_reduce_bwd/{kind}", repeat=False)


def _loss_inputs(loss, n):
    x, t = pattern(91, (n,), -2, 2), pattern(92, (n,), 0, 1)
    if loss == "bce":
        x = pattern(91, (n,), 0.02, 0.98)
    if loss == "kldiv":
        t[::5] = 0.0                                               # zero targets contribute nothing
    if loss == "mae" and n > 2:
        t[1] = x[1]                                                # a zero difference: gradient 0, not signum(0)
    return x, t


@pytest.mark.parametrize("n", REDUCE_N, ids=lambda n: f"n{n}")
@pytest.mark.parametrize("red", ("sum", "mean"))
@pytest.mark.parametrize("loss", ("mae", "bce", "bce_with_logits", "kldiv"))
def test_loss(dev, loss, red, n):
    c = capi()
    x, t = _loss_inputs(loss, n)
    x64, t64 = x.astype(np.float64), t.astype(np.float64)
    X, T = put(dev, x), put(dev, t)
    fwd = {"mae": O.mae_forward, "bce": O.bce_forward, "bce_with_logits": O.bce_with_logits_forward, "kldiv": O.kldiv_forward}[loss]
    ref = float(fwd(x64, t64, red))
    tmax = 4.0      # a term's magnitude: |x - t| <= 3; -ln 0.02 = 3.9; (1 - t) x + softplus(-x) <= 4.2 at |x| <= 2; t (ln t - x) <= 2
    outs = []
    for _ in range(2):
        w = Window(dev, (1,), np.nan)
        c.loss_fwd(dev, loss, X, T, w.v, red)
        outs.append(w.read())
    assert same_bits(outs[0], outs[1])
    check(f"dispatch/loss/{loss}", outs[0], np.array([ref]), n, tmax, 1.0, scale=1.0 / n if red == "mean" else 1.0)
    gs = 0.75
    Gs = put(dev, np.array([gs], np.float32))
    inc = np.zeros(n)
    if loss == "kldiv": O.kldiv_backward(inc, gs, t64, red)
    else: {"mae": O.mae_backward, "bce": O.bce_backward, "bce_with_logits": O.bce_with_logits_backward}[loss](inc, gs, x64, t64, red)
    accumulate_forms(dev, (n,), lambda d, a: c.loss_bwd(dev, loss, d, Gs, X, T, red), inc, f"dispatch/loss_bwd/{loss}", has_assign=False,
                     repeat=False)


NLL = [("3x5", (3, 5)), ("257x7x3", (257, 7, 3)), ("4x3x1025", (4, 3, 1025)), ("1x1", (1, 1)), ("70000x3", (70000, 3))]


@pytest.mark.parametrize("case", NLL, ids=[c[0] for c in NLL])
@pytest.mark.parametrize("red", ("sum", "mean"))
def test_nll(dev, red, case):
    c = capi()
    _, shape = case
    x = pattern(95, shape, -4, 0)
    tshape = (shape[0],) + tuple(shape[2:])
    t = np.floor(np.random.default_rng(96).random(tshape) * shape[1]).astype(np.float32)
    tf = t.reshape(-1)
    if tf.size > 4:
        tf[0], tf[1], tf[2], tf[3] = shape[1], -1.0, np.nan, 0.5       # selects nothing, saturates to 0, NaN -> 0, truncates
    x64, t64 = x.astype(np.float64), t.astype(np.float64)
    X, T = put(dev, x), put(dev, t)
    pos = numel(tshape)
    outs = []
    for _ in range(2):
        w = Window(dev, (1,), np.nan)
        c.nll_fwd(dev, X, T, w.v, red)
        outs.append(w.read())
    assert same_bits(outs[0], outs[1])
    check("dispatch/nll", outs[0], np.array([float(O.nll_forward(x64, t64, red))]), pos, 4.0, 1.0, scale=1.0 / shape[0] if red == "mean" else 1.0)
    gs = 0.75
    Gs = put(dev, np.array([gs], np.float32))
    inc = np.zeros(shape)
    O.nll_backward(inc, gs, t64, red)
    accumulate_forms(dev, shape, lambda d, a: c.nll_bwd(dev, d, Gs, T, red), inc, "dispatch/nll_bwd", has_assign=False, repeat=False)


# ======================================================================================================================
# sub-block users: chunk, concat, pad backward
# ======================================================================================================================
# (id, x shape, chunk shape, chunk_no, offsets (chunk side, x side))
CHUNK = [
    ("vec", (4, 8, 56), (2, 4, 56), 3, (0, 0)),               # float4: collapsed rows of 224, origin % 4 == 0
    ("vec_rank1", (96,), (8,), 5, (0, 0)),                    # rank 1, float4 (origin 40)
    ("generic_rank1", (100,), (7,), 3, (0, 0)),               # rank 1, W % 4 != 0: one collapsed dim -> scalar generic kernel
    ("plane_w9", (6, 9, 3), (2, 3, 3), 4, (0, 0)),            # plane kernel: the last two axes merge, H = 2, W = 9
    ("plane_w1", (5, 7, 4), (5, 7, 1), 2, (0, 0)),            # plane kernel with W == 1 (H = 35)
    ("plane_w3", (64, 9), (64, 3), 1, (0, 0)),                # W = 3
    ("plane_w56_odd_origin", (3, 58, 57), (3, 58, 56), 0, (0, 0)),   # W = 56 but the row stride 57 is odd
    ("plane_w41", (3, 7, 82), (3, 7, 41), 1, (0, 0)),         # W = 41: (float)41 * (1.f / 41) < 1 - fast_div needs its +1 at i = 41
    ("plane_w4099", (9, 8198), (9, 4099), 1, (0, 0)),         # a large prime W, odd origin
    ("plane_w16381", (3, 32762), (3, 16381), 1, (0, 0)),      # large prime where the reciprocal quotient is one short at every row start
    ("rank8", (2, 2, 3, 2, 2, 3, 2, 6), (1, 2, 3, 1, 2, 3, 1, 3), 13, (0, 0)),     # the maximum rank, W = 3: plane kernel, five outer dims
    ("rank8_vec", (2, 2, 3, 2, 2, 3, 2, 8), (1, 2, 3, 1, 2, 3, 1, 4), 13, (0, 0)),     # the maximum rank, float4
    ("vec_off_small1", (4, 8, 56), (2, 4, 56), 3, (1, 0)),    # float4 refused: the chunk side is offset by 1, 2, 3 floats -> plane
    ("vec_off_small2", (4, 8, 56), (2, 4, 56), 3, (2, 0)),
    ("vec_off_small3", (4, 8, 56), (2, 4, 56), 3, (3, 0)),
    ("vec_off_big1", (4, 8, 56), (2, 4, 56), 3, (0, 1)),      # ... the x side
    ("vec_off_big2", (4, 8, 56), (2, 4, 56), 3, (0, 2)),
    ("vec_off_big3", (4, 8, 56), (2, 4, 56), 3, (0, 3)),
    ("vec_rank1_off3", (96,), (8,), 5, (3, 0)),               # rank 1 offset: generic
]


@pytest.mark.parametrize("case", CHUNK, ids=[c[0] for c in CHUNK])
def test_chunk(dev, case):
    c = capi()
    _, xs, cs, no, (so, bo) = case
    x = pattern(101, xs, -2, 2)
    ref = np.zeros(cs, np.float32)
    O.chunk_forward(x, ref, no)
    w = Window(dev, cs, np.nan, so)
    c.chunk_fwd(dev, put(dev, x, bo), w.v, no)                  # subblock<0, false>
    assert np.array_equal(w.read(), ref)
    g = pattern(102, cs, -2, 2)
    d0 = pattern(103, xs, -2, 2)
    want = d0.copy()
    O.chunk_backward(want, g, no)                               # f32: one add per touched element, the rest untouched
    wd = Window(dev, xs, d0, bo)
    c.chunk_bwd(dev, wd.v, put(dev, g, so), no)                 # subblock<1, true>
    assert np.array_equal(wd.read(), want)


# (id, out shape, axis, operand extents along it, offsets (operand side, out side))
CONCAT = [
    ("vec", (5, 24, 8), 1, (8, 12, 4), (0, 0)),               # float4 for every part
    ("odd_parts", (5, 9, 7), 1, (2, 3, 4), (0, 0)),           # W = 7 rows merge with the part: plane, odd origins
    ("last_axis", (37, 13), 1, (1, 3, 4, 5), (0, 0)),         # W = 1, 3, 4 (origin 4 but row stride 13), 5: plane
    ("rank1", (100,), 0, (5, 37, 8, 50), (0, 0)),             # rank 1: generic, generic, float4 refused (origin 42), generic
    ("rank1_vec", (96,), 0, (8, 40, 48), (0, 0)),             # rank 1, float4
    ("axis0", (9, 6, 4), 0, (2, 3, 4), (0, 0)),               # whole rows merge into one dim: float4 with one collapsed dim
    ("vec_off_op1", (5, 24, 8), 1, (8, 12, 4), (1, 0)),       # operand side offset by 1, 2, 3 floats: plane
    ("vec_off_op2", (5, 24, 8), 1, (8, 12, 4), (2, 0)),
    ("vec_off_op3", (5, 24, 8), 1, (8, 12, 4), (3, 0)),
    ("vec_off_out1", (5, 24, 8), 1, (8, 12, 4), (0, 1)),      # out side offset: plane
    ("vec_off_out2", (5, 24, 8), 1, (8, 12, 4), (0, 2)),
    ("vec_off_out3", (5, 24, 8), 1, (8, 12, 4), (0, 3)),
    # LARGE (33.6 MB per tensor): a plane of 2047 x 4097 = 2^23 - 2049 elements still takes the plane kernel ...
    ("plane_below_2p23", (2047, 4098), 1, (1, 4097), (0, 0)),
    # ... and 2048 x 4097 = 2^23 + 2048 elements must take the scalar generic kernel (fast_div is not valid there)
    ("generic_above_2p23", (2048, 4098), 1, (1, 4097), (0, 0)),
]


@pytest.mark.parametrize("case", CONCAT, ids=[c[0] for c in CONCAT])
def test_concat(dev, case):
    c = capi()
    _, oshape, axis, lens, (po, oo) = case
    shapes = [tuple(l if i == axis else s for i, s in enumerate(oshape)) for l in lens]
    parts = [pattern(110 + i, s, -2, 2) for i, s in enumerate(shapes)]
    ref = np.concatenate(parts, axis=axis)
    w = Window(dev, oshape, np.nan, oo)
    c.concat_fwd(dev, [put(dev, p, po) for p in parts], w.v, axis)      # subblock<1, false>
    assert np.array_equal(w.read(), ref)
    g = pattern(120, oshape, -2, 2)
    G = put(dev, g, oo)
    incs = np.split(g, np.cumsum(lens)[:-1], axis=axis)
    d0s = [pattern(130 + i, s, -2, 2) for i, s in enumerate(shapes)]
    acc = [Window(dev, s, d, po) for s, d in zip(shapes, d0s)]
    c.concat_bwd(dev, [a.v for a in acc], G, axis)                      # subblock<0, true>
    asg = [Window(dev, s, np.nan, po) for s in shapes]
    c.concat_bwd(dev, [a.v for a in asg], G, axis, assign=True)         # subblock<0, false>
    for a, s, d0, inc in zip(acc, asg, d0s, incs):
        assert np.array_equal(a.read(), d0 + inc)
        assert np.array_equal(s.read(), inc)


# (id, x shape (N, C, spatial...), padding, offsets (dx, g))
PAD_BWD = [
    ("2d_centre", (2, 3, 56, 56), (1, 1), (0, 0)),            # origin 59, rows of 56 in rows of 58: plane
    ("2d_vec", (2, 3, 56, 56), (4, 4), (0, 0)),               # origin 260, row stride 64: float4
    ("2d_pad0", (2, 3, 8, 8), (0, 0), (0, 0)),                # nothing padded: one collapsed dim, float4
    ("2d_pad_w_only", (2, 3, 8, 56), (0, 2), (0, 0)),         # padding 0 on H: origin 2 -> plane
    ("2d_pad_h_only", (2, 3, 8, 56), (2, 0), (0, 0)),         # padding 0 on W: rows merge, origin 112 -> float4
    ("1d", (2, 3, 17), (3,), (0, 0)),                         # one spatial dim, W = 17: plane with H = 6
    ("1d_vec", (2, 3, 16), (4,), (0, 0)),                     # float4
    ("3d", (1, 2, 3, 5, 8), (1, 0, 2), (0, 0)),               # three spatial dims, padding 0 in the middle
    ("3d_w41", (1, 2, 3, 5, 41), (1, 1, 1), (0, 0)),          # W = 41 (fast_div correction), three outer dims
]
# float4 refused because dx, then g, sits 1, 2 or 3 floats past a 16-byte boundary: plane kernel, same values
PAD_BWD += [(f"2d_vec_off_{w}{k}", (2, 3, 56, 56), (4, 4), (k, 0) if w == "dx" else (0, k)) for w in ("dx", "g") for k in (1, 2, 3)]


@pytest.mark.parametrize("case", PAD_BWD, ids=[c[0] for c in PAD_BWD])
def test_pad_bwd(dev, case):
    c = capi()
    cid, xs, pad, (do, go) = case
    gshape = tuple(xs[:2]) + tuple(s + 2 * p for s, p in zip(xs[2:], pad))
    g = pattern(140, gshape, -2, 2)
    inc = np.zeros(xs, np.float32)
    O.pad_backward(inc, g, pad)
    G = put(dev, g, go)
    accumulate_forms(dev, xs, lambda d, a: c.pad_bwd(dev, d, G, pad, assign=a), inc, f"pad_bwd/{cid}", off=do, exact=True, repeat=False)


# ======================================================================================================================
# pad forward
# ======================================================================================================================
# (id, x shape, padding, float offset of y)
PAD_FWD = [
    ("1d_odd", (2, 3, 17), (3,), 0),              # out 23: plane kernel for every mode
    ("1d_even", (2, 3, 16), (2,), 0),             # out 20: constant -> pairs kernel
    ("1d_pad0", (2, 3, 16), (0,), 0),             # nothing padded
    ("2d_even", (2, 3, 5, 8), (1, 1), 0),         # out 7 x 10: pairs
    ("2d_odd", (2, 3, 5, 7), (1, 1), 0),          # out 7 x 9: plane
    ("2d_pad_w_only", (1, 2, 6, 6), (0, 2), 0),   # padding 0 on H
    ("2d_pad_h_only", (1, 2, 6, 6), (2, 0), 0),   # padding 0 on W
    ("2d_w41", (1, 2, 5, 35), (2, 3), 0),         # out 9 x 41: fast_div by 41 needs its correction at every row start
    ("2d_w82", (1, 2, 5, 80), (2, 1), 0),         # out 9 x 82: the pairs kernel divides by 41
    ("3d_h41", (1, 2, 3, 39, 6), (0, 1, 1), 0),   # out 3 x 41 x 8: the second division is by 41
    ("3d", (1, 2, 3, 4, 6), (1, 0, 2), 0),        # three spatial dims, out 5 x 4 x 10: pairs
    ("3d_odd", (1, 2, 3, 4, 5), (1, 2, 1), 0),    # out 5 x 8 x 7: plane
    ("2d_even_off1", (2, 3, 5, 8), (1, 1), 1),    # y not 8-byte aligned: constant falls back to the plane kernel
    ("2d_even_off2", (2, 3, 5, 8), (1, 1), 2),    # y 8-byte but not 16-byte aligned: pairs still
    ("2d_odd_off3", (2, 3, 5, 7), (1, 1), 3),
    ("1x1", (1, 1, 1), (1,), 0),                  # one input element (replicative / constant; reflective needs extent > padding)
    # LARGE (33.6 MB): a padded plane of 2049 x 4096 = 2^23 + 4096 elements takes the generic kernel of every mode
    ("plane_above_2p23", (1, 1, 2049, 4094), (0, 1), 0),
    ("plane_below_2p23", (1, 1, 2047, 4094), (0, 1), 0),     # LARGE: 2047 x 4096 = 2^23 - 4096: the last plane-kernel size
]


@pytest.mark.parametrize("case", PAD_FWD, ids=[c[0] for c in PAD_FWD])
@pytest.mark.parametrize("mode", ("constant", "reflective", "replicative"))
def test_pad_fwd(dev, mode, case):
    c = capi()
    _, xs, pad, yo = case
    if mode == "reflective" and any(p and p >= s for p, s in zip(pad, xs[2:])):
        rejected(c.pad_mode_fwd, dev, put(dev, pattern(150, xs)), Window(dev, (4,), 0.0).v, pad, mode)    # host-side rejection
        return
    x = pattern(150, xs, -2, 2)
    oshape = tuple(xs[:2]) + tuple(s + 2 * p for s, p in zip(xs[2:], pad))
    ref = np.zeros(oshape, np.float32)
    if mode == "constant": O.pad_constant_forward(x, ref, pad, 1.5)
    else: O.pad_mode_forward(x, ref, pad, mode)
    w = Window(dev, oshape, np.nan, yo)
    X = put(dev, x)
    if mode == "constant": c.pad_const_fwd(dev, X, w.v, pad, 1.5)
    else: c.pad_mode_fwd(dev, X, w.v, pad, mode)
    assert np.array_equal(w.read(), ref)


# ======================================================================================================================
# transpose, heads
# ======================================================================================================================
TRANSPOSE = [(37, 70), (32, 32), (33, 31), (1, 100), (100, 1), (64, 96), (1, 1), (17,), (3, 5, 7), (2, 3, 4, 5), (2, 3, 2, 3, 5),
             (2, 1, 3, 2, 1, 2, 3, 4)]      # 2-D tiles ragged on both sides, full tiles, 1 x N, N x 1; ranks 1, 3, 4, 5 and 8 (generic kernel)


@pytest.mark.parametrize("shape", TRANSPOSE, ids=lambda s: "x".join(map(str, s)))
def test_transpose(dev, shape):
    c = capi()
    x = pattern(160, shape, -2, 2)
    rshape = tuple(reversed(shape))
    w = Window(dev, rshape, np.nan)
    c.transpose_fwd(dev, put(dev, x), w.v)
    assert np.array_equal(w.read(), x.T)
    g = pattern(161, rshape, -2, 2)
    G = put(dev, g)
    accumulate_forms(dev, shape, lambda d, a: c.transpose_bwd(dev, d, G, assign=a), np.ascontiguousarray(g.T), "transpose_bwd", exact=True,
                     repeat=False)


# (dh, S, H, offsets (flat side, heads side)); B = 2.  dh % 4 == 0 and aligned: float4
HEADS = [(4, 1, 1, (0, 0)), (6, 5, 3, (0, 0)), (8, 5, 3, (0, 0)), (32, 128, 16, (0, 0)), (64, 197, 3, (0, 0)), (128, 197, 1, (0, 0)),
         (6, 197, 16, (0, 0)), (64, 1, 16, (0, 0)), (128, 5, 3, (0, 0)), (32, 197, 3, (0, 0)),
         (8, 197, 3, (3, 3))] + [(64, 5, 3, o) for o in ((1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3))]
# ... offset pointers, each side in turn at 1, 2, 3 floats: the scalar kernel although dh % 4 == 0


@pytest.mark.parametrize("dh,S,H,offs", HEADS, ids=[f"dh{d}-S{s}-H{h}" + (f"-off{o[0]}{o[1]}" if any(o) else "") for d, s, h, o in HEADS])
def test_heads(dev, dh, S, H, offs):
    c = capi()
    B = 2
    fo, ho = offs
    fshape, hshape = (B * S, H * dh), (B * H, S, dh)
    split, merge = (lambda a: O._heads_split(a, B, H)), (lambda a: O._heads_merge(a, B, H))
    x = pattern(170, fshape, -2, 2)
    w = Window(dev, hshape, np.nan, ho)
    c.split_heads_fwd(dev, put(dev, x, fo), w.v, B, S, H, dh)                     # heads<true, false>
    assert np.array_equal(w.read(), split(x))
    gh = pattern(171, hshape, -2, 2)
    GH = put(dev, gh, ho)
    accumulate_forms(dev, fshape, lambda d, a: c.split_heads_bwd(dev, d, GH, B, S, H, dh, assign=a), merge(gh), "split_heads_bwd", off=fo,
                     exact=True, repeat=False)                                    # heads<false, true | false>
    w = Window(dev, fshape, np.nan, fo)
    c.merge_heads_fwd(dev, GH, w.v, B, S, H, dh)                                  # heads<false, false>
    assert np.array_equal(w.read(), merge(gh))
    GF = put(dev, x, fo)
    accumulate_forms(dev, hshape, lambda d, a: c.merge_heads_bwd(dev, d, GF, B, S, H, dh, assign=a), split(x), "merge_heads_bwd", off=ho,
                     exact=True, repeat=False)                                    # heads<true, true | false>


# ======================================================================================================================
# dropout
# ======================================================================================================================
@pytest.mark.parametrize("n", (1, 3, 4, 5, 6, 7, 8, 1027, 3 * 4096 + 2), ids=lambda n: f"n{n}")      # n % 4 = 1, 3, 0, 1, 2, 3, 0, 3, 2
@pytest.mark.parametrize("p", (0.0, 0.5, 1.0), ids=lambda p: f"p{p}")
def test_dropout(dev, n, p):
    c = capi()
    seed, offset = 1234, 7
    x, g = pattern(180, (n,), -2, 2), pattern(181, (n,), -2, 2)
    X, G = put(dev, x), put(dev, g)
    noise = O.dropout_noise(n, p, seed, offset)
    ref = np.zeros(n, np.float32)
    O.dropout_forward(x, ref, noise, p, True)
    y, nz = Window(dev, (n,), np.nan), Window(dev, (n,), np.nan)
    c.dropout_fwd(dev, X, y.v, nz.v, p, True, seed, offset)
    got_noise = nz.read()
    assert np.array_equal(y.read(), ref)                                           # one f32 product and one division: exact
    if 0.0 < p < 1.0:
        assert np.array_equal(got_noise, noise)
        # the mask belongs to (seed, offset), not to the buffers: other (16-byte aligned) addresses, same draws
        y2, nz2 = Window(dev, (n,), np.nan, 4), Window(dev, (n,), np.nan, 8)
        c.dropout_fwd(dev, put(dev, np.concatenate([np.zeros(4, np.float32), x])).view_offset(4), y2.v, nz2.v, p, True, seed, offset)
        assert np.array_equal(nz2.read(), noise) and np.array_equal(y2.read(), ref)
        if n >= 64:
            nz3 = Window(dev, (n,), np.nan)
            c.dropout_fwd(dev, X, Window(dev, (n,), np.nan).v, nz3.v, p, True, seed + 1, offset)
            assert not np.array_equal(nz3.read(), noise)
        rejected(c.dropout_fwd, dev, put(dev, x, 1), y.v, nz.v, p, True, seed, offset)      # alignment is required: host-side error
    else:
        assert (bits(got_noise) == bits(np.float32(np.nan))).all()                 # p == 0 / p == 1 leave the noise buffer alone
    N = put(dev, noise)
    inc = g if p == 0.0 else g * noise                                             # `g * noise` exactly (not divided by 1 - p)
    accumulate_forms(dev, (n,), lambda d, a: c.dropout_bwd(dev, d, G, N, p, True, assign=a), inc, "dropout_bwd", exact=True, repeat=False)
    accumulate_forms(dev, (n,), lambda d, a: c.dropout_bwd(dev, d, G, None, p, False, assign=a), g, "dropout_bwd_eval", exact=True, repeat=False)


# ======================================================================================================================
# pointwise: relu, relu_mask_inplace, fill, the unary ops
# ======================================================================================================================
POINTWISE_N = (1, 3, 4, 5, 1027, 4 * 1024 * 4 + 6)      # below / at / above one quad, a ragged tail, four unrolled trips + remainder


@pytest.mark.parametrize("off", (0, 1, 2, 3), ids=lambda o: f"off{o}")       # off > 0: the <false> kernels
@pytest.mark.parametrize("n", POINTWISE_N, ids=lambda n: f"n{n}")
def test_relu(dev, n, off):
    c = capi()
    x, g = pattern(190, (n,), -2, 2), pattern(191, (n,), -2, 2)
    x[::7] = 0.0
    w = Window(dev, (n,), np.nan, off)
    X, G = put(dev, x, off), put(dev, g, off)
    c.relu_fwd(dev, X, w.v)
    y = w.read()
    assert np.array_equal(y, np.maximum(x, 0))
    inc = np.where(x > 0, g, np.float32(0) * g)
    accumulate_forms(dev, (n,), lambda d, a: c.relu_bwd(dev, d, G, X, assign=a), inc, "relu_bwd", off=off, exact=True, repeat=False)
    m = Window(dev, (n,), g, off)
    c.relu_mask_inplace(dev, m.v, put(dev, y, off))
    assert np.array_equal(m.read(), inc)
    if off:                                                                        # mixed alignment: one aligned, one offset operand
        m = Window(dev, (n,), g, 0)
        c.relu_mask_inplace(dev, m.v, put(dev, y, off))
        assert np.array_equal(m.read(), inc)


@pytest.mark.parametrize("n", POINTWISE_N, ids=lambda n: f"n{n}")
def test_fill(dev, n):
    w = Window(dev, (n,), np.nan)
    w.v.fill(2.5)                                                                  # fill_kernel
    assert np.array_equal(w.read(), np.full(n, 2.5, np.float32))
    w.v.fill(0.0)                                                                  # memset path
    assert np.array_equal(w.read(), np.zeros(n, np.float32))


UNARY = ("neg", "exp", "ln", "sqrt", "sigmoid", "tanh", "softplus", "leaky_relu", "pow")


@pytest.mark.parametrize("n", POINTWISE_N, ids=lambda n: f"n{n}")
@pytest.mark.parametrize("op", UNARY)
def test_unary(dev, op, n):
    c = capi()
    lo, hi = (0.1, 3.0) if op in ("ln", "sqrt") else (-2.0, 2.0)
    x, g = pattern(200, (n,), lo, hi), pattern(201, (n,), -1, 1)
    e = 3 if op == "pow" else 0
    x64 = x.astype(np.float64)
    ref = np.zeros(n)
    O.unary_forward(op, x64, ref, e)
    X, G = put(dev, x), put(dev, g)
    w = Window(dev, (n,), np.nan)
    c.unary_fwd(dev, op, X, w.v, e)
    close(w.read(), ref)
    # the buffer the node keeps: its output for exp / sqrt / sigmoid / tanh (as the oracle's backward takes it), else its input
    keep = ref.astype(np.float32) if op in O.UNARY_KEEPS_OUTPUT else x
    inc = np.zeros(n)
    O.unary_backward(op, inc, g.astype(np.float64), keep.astype(np.float64), e)
    Kp = put(dev, keep)
    accumulate_forms(dev, (n,), lambda d, a: c.unary_bwd(dev, op, d, G, None if op == "neg" else Kp, e, assign=a), inc, f"unary_bwd/{op}",
                     repeat=False)


def test_alignment_required(dev):
    """entry points that REQUIRE 16-byte alignment return their error without launching (host-side check only)"""
    c = capi()
    n = 8
    a, b, s = put(dev, pattern(210, (n,))), put(dev, pattern(211, (n,))), put(dev, np.zeros(1, np.float32))
    for off in (1, 2, 3):
        u = put(dev, pattern(212, (n,)), off)
        rejected(u.fill, 2.5)                                                      # nk_fill with a non-zero value
        rejected(c.unary_fwd, dev, "exp", u, a)
        rejected(c.unary_fwd, dev, "exp", a, u)
        rejected(c.unary_bwd, dev, "exp", u, a, b)
        rejected(c.unary_bwd, dev, "exp", a, u, b)
        rejected(c.unary_bwd, dev, "exp", a, b, u)
        rejected(c.sum_fwd, dev, u, s)
        rejected(c.mse_fwd, dev, a, u, s)
        rejected(c.sum_bwd, dev, u, s)
        rejected(c.mse_bwd, dev, a, s, u, b)
        rejected(c.loss_fwd, dev, "mae", u, a, s)
        rejected(c.loss_bwd, dev, "mae", u, s, a, b)
        rejected(c.dropout_bwd, dev, u, a, b, 0.5)
        L = 4
        rejected(c.scale_softmax_dropout_fwd, dev, view(u, 0, (2, L)), None, view(a, 0, (2, L)), None, 1.0, 0.0)
    u.fill(0.0)                                                                    # value 0 is a memset: any alignment


# ======================================================================================================================
# GEMV / dot
# ======================================================================================================================
# (rows, cols, float offset of the matrix)
GEMV = [(5, 7, 0),            # scalar, block per row; cols_comb scalar, one split
        (37, 64, 0),          # float4, block per row (16 of 256 lanes busy); cols_comb float4, two splits -> cols_final
        (17, 1028, 0),        # float4, second trip of one lane; cols_comb: one split, written directly (ACC reads y)
        (2049, 12, 0),        # float4, wave per row (rows >= 2048), 3 of 64 lanes busy
        (2050, 7, 0),         # scalar, wave per row
        (33, 260, 0),         # float4; 33 rows: two splits of 17 / 16
        (1000, 1028, 0),      # 32 splits; two column blocks in the float4 form
        (37, 64, 1), (37, 64, 2), (37, 64, 3), (2049, 12, 2), (17, 1028, 3)]     # the matrix (then each vector) offset: the scalar variants


@pytest.mark.parametrize("rows,cols,off", GEMV, ids=[f"{r}x{k}" + (f"-off{o}" if o else "") for r, k, o in GEMV])
def test_gemv(dev, rows, cols, off):
    c = capi()
    A = pattern(220, (rows, cols), -1, 1)
    xv, gv = pattern(221, (cols,), -1, 1), pattern(222, (rows,), -1, 1)
    A64, x64, g64 = A.astype(np.float64), xv.astype(np.float64), gv.astype(np.float64)
    dA, dX, dG = put(dev, A, off), put(dev, xv), put(dev, gv)
    lab = "dispatch/gemv"
    # y = A x (rows_dot<false>), dv += B g (rows_dot<true>)
    outs = []
    for _ in range(2):
        w = Window(dev, (rows,), np.nan); c.mv_fwd(dev, dA, dX, w.v); outs.append(w.read())
    assert same_bits(outs[0], outs[1])
    check(lab + "/mv_fwd", outs[0], A64 @ x64, cols, 1.0, 1.0)
    accumulate_forms(dev, (rows,), lambda d, a: c.vm_bwd_left(dev, d, dA, dX), A64 @ x64, lab + "/vm_bwd_left", cols, 1.0, 1.0, has_assign=False)
    # y = v B (cols_comb<false>), dx += A^T g (cols_comb<true>)
    outs = []
    for _ in range(2):
        w = Window(dev, (cols,), np.nan); c.vm_fwd(dev, dG, dA, w.v); outs.append(w.read())
    assert same_bits(outs[0], outs[1])
    check(lab + "/vm_fwd", outs[0], g64 @ A64, rows, 1.0, 1.0)
    accumulate_forms(dev, (cols,), lambda d, a: c.mv_bwd_right(dev, d, dA, dG), g64 @ A64, lab + "/mv_bwd_right", rows, 1.0, 1.0, has_assign=False)
    # dA += g (x) x (outer_add) through both entry points; the destination matrix itself offset
    outer = np.outer(g64, x64)
    accumulate_forms(dev, (rows, cols), lambda d, a: c.mv_bwd_left(dev, d, dG, dX), outer, lab + "/mv_bwd_left", off=off, has_assign=False,
                     repeat=False)
    accumulate_forms(dev, (rows, cols), lambda d, a: c.vm_bwd_right(dev, d, dG, dX), outer, lab + "/vm_bwd_right", off=off, has_assign=False,
                     repeat=False)
    if off:     # offset vectors: x for rows_dot, y for cols_comb, v for outer_add
        w = Window(dev, (rows,), np.nan); c.mv_fwd(dev, put(dev, A), put(dev, xv, off), w.v)
        check(lab + "/mv_fwd", w.read(), A64 @ x64, cols, 1.0, 1.0)
        w = Window(dev, (cols,), np.nan, off); c.vm_fwd(dev, dG, put(dev, A), w.v)
        check(lab + "/vm_fwd", w.read(), g64 @ A64, rows, 1.0, 1.0)
        accumulate_forms(dev, (rows, cols), lambda d, a: c.mv_bwd_left(dev, d, dG, put(dev, xv, off)), outer, lab + "/mv_bwd_left",
                         has_assign=False, repeat=False)


@pytest.mark.parametrize("n", (1, 3, 255, 256, 257, (1 << 18) + 3, (1 << 20) + 5), ids=lambda n: f"n{n}")
@pytest.mark.parametrize("off", (0, 1, 2, 3), ids=lambda o: f"off{o}")
def test_dot(dev, n, off):
    c = capi()
    a, b = pattern(230, (n,), -1, 1), pattern(231, (n,), -1, 1)
    A, B = put(dev, a, off), put(dev, b)
    outs = []
    for _ in range(2):
        w = Window(dev, (1,), np.nan); c.vv_fwd(dev, A, B, w.v); outs.append(w.read())
    assert same_bits(outs[0], outs[1])
    check("dispatch/dot", outs[0], np.array([a.astype(np.float64) @ b.astype(np.float64)]), n, 1.0, 1.0)
    Gs = put(dev, np.array([0.75], np.float32))
    accumulate_forms(dev, (n,), lambda d, _a: c.vv_bwd(dev, d, B, Gs), b.astype(np.float64) * 0.75, "vv_bwd", off=off, has_assign=False,
                     repeat=False)


# ======================================================================================================================
# optimizers
# ======================================================================================================================
OPT_N = (1, 3, 4, 5, 4096, 4097, 2 * 4096 + 1027)      # below one float4 .. one SGD chunk exactly (the float4 path), + 1, ragged


def _opt_state(n, k):
    return [pattern(240 + i, (n,), 0.1 if i >= 2 else -1, 1) for i in range(k)]


@pytest.mark.parametrize("n", OPT_N, ids=lambda n: f"n{n}")
@pytest.mark.parametrize("variant", ("plain", "momentum", "nesterov_l1l2"))
def test_sgd(dev, variant, n):
    c = capi()
    kw = {"plain": dict(), "momentum": dict(momentum=0.9, dampening=0.1), "nesterov_l1l2": dict(momentum=0.9, nesterov=True, l1=1e-3, l2=1e-2)}[variant]
    w, g, v = _opt_state(n, 3)
    w[0] = 0.0                                                                    # signum(+0) = 1 in the L1 penalty
    w64, g64, v64 = (a.astype(np.float64) for a in (w, g, v))
    O.sgd_step(w64, g64, 0.05, v64 if variant != "plain" else None, **kw)
    Ww, Gw, Vw = Window(dev, (n,), w), Window(dev, (n,), g), Window(dev, (n,), v)
    c.sgd_step(dev, Ww.v, Gw.v, Vw.v if variant != "plain" else None, lr=0.05, **kw)
    close(Ww.read(), w64); close(Gw.read(), g64); close(Vw.read(), v64 if variant != "plain" else v)
    for off in (1, 2, 3):                                                         # offset pointers: the scalar loop
        Wo, Go, Vo = Window(dev, (n,), w, off), Window(dev, (n,), g, off), Window(dev, (n,), v, off)
        c.sgd_step(dev, Wo.v, Go.v, Vo.v if variant != "plain" else None, lr=0.05, **kw)
        close(Wo.read(), w64); close(Go.read(), g64); close(Vo.read(), v64 if variant != "plain" else v)


def test_sgd_multi_ragged(dev):
    """one table with zero-length, sub-quad, whole-chunk and ragged members (more than SGD_MULTI_MAX = 8 non-empty ones: two
    launches) against one call per member"""
    c = capi()
    sizes = (0, 1, 5, 4096, 4099, 0, 3, 8192, 4, 7, 4100, 2)
    kw = dict(lr=0.05, momentum=0.9, dampening=0.1, nesterov=True, l1=1e-3, l2=1e-2)
    host = [tuple(pattern(250 + 3 * i + j, (max(n, 1),), -1, 1) for j in range(3)) for i, n in enumerate(sizes)]

    def windows():
        ws = [tuple(Window(dev, (max(n, 1),), a) for a in h) for n, h in zip(sizes, host)]
        for n, trio in zip(sizes, ws):
            for w in trio:
                w.v.shape, w.v.size = (n,), n                                     # a zero-length member keeps a valid pointer
        return ws
    one, each = windows(), windows()
    c.sgd_step_multi(dev, [t[0].v for t in one], [t[1].v for t in one], [t[2].v for t in one], **kw)
    for n, t in zip(sizes, each):
        c.sgd_step(dev, t[0].v, t[1].v, t[2].v, **kw)
    for n, h, a, b in zip(sizes, host, one, each):
        w64, g64, v64 = (x.astype(np.float64) for x in h)
        if n:
            O.sgd_step(w64, g64, kw["lr"], v64, kw["momentum"], kw["dampening"], kw["nesterov"], kw["l1"], kw["l2"])
        for x, y, r in zip(a, b, (w64, g64, v64)):
            got = x.read()
            assert same_bits(got, y.read())
            close(got, r)                                                         # n == 0: untouched


@pytest.mark.parametrize("n", OPT_N, ids=lambda n: f"n{n}")
def test_adam_adagrad_rmsprop(dev, n):
    c = capi()
    w, g, m, v, vm = _opt_state(n, 5)
    for amsgrad in (False, True):
        r = [a.astype(np.float64) for a in (w, g, m, v, vm)]
        O.adam_step(r[0], r[1], r[2], r[3], 1e-2, 0.9, 0.999, 1e-8, 3, r[4] if amsgrad else None, l1=1e-3, l2=1e-2)
        W = [Window(dev, (n,), a) for a in (w, g, m, v, vm)]
        c.adam_step(dev, W[0].v, W[1].v, W[2].v, W[3].v, W[4].v if amsgrad else None, lr=1e-2, step=3, l1=1e-3, l2=1e-2)
        for x, ref in zip(W, r):
            close(x.read(), ref)
    r = [a.astype(np.float64) for a in (w, g, v)]
    O.adagrad_step(r[0], r[1], r[2], 1e-2, 0.1, 1e-10, 4, l2=1e-2)
    W = [Window(dev, (n,), a) for a in (w, g, v)]
    c.adagrad_step(dev, W[0].v, W[1].v, W[2].v, lr=1e-2, lr_decay=0.1, step=4, l2=1e-2)
    for x, ref in zip(W, r):
        close(x.read(), ref)
    for centered, mom in ((False, 0.0), (True, 0.0), (False, 0.9), (True, 0.9)):
        ga = (pattern(260, (n,), -0.05, 0.05))                                    # |mean|^2 well below the mean square
        r = [a.astype(np.float64) for a in (w, g, v, ga, m)]
        O.rmsprop_step(r[0], r[1], r[2], 1e-2, 0.99, 1e-8, r[3] if centered else None, r[4] if mom else None, mom, l1=1e-3)
        W = [Window(dev, (n,), a) for a in (w, g, v, ga, m)]
        c.rmsprop_step(dev, W[0].v, W[1].v, W[2].v, W[3].v if centered else None, W[4].v if mom else None, lr=1e-2, momentum=mom, l1=1e-3)
        for x, ref in zip(W, r):
            close(x.read(), ref)


# ======================================================================================================================
# past the cache switch (nk_streams_past_cache: more than 384 MiB touched -> `nt` loads)           LARGE: 128 MiB per tensor
# ======================================================================================================================
def _ramp(n, mod, scale, shift):
    return (((np.arange(n, dtype=np.int64) * 7919) % mod).astype(np.float32) - np.float32(shift)) * np.float32(scale)


def test_past_cache_switch(dev):
    """one set of 128 MiB buffers through every kernel that changes its load flavour above 384 MiB touched: binary_bwd_same
    (12 B / element), relu backward and mask (16 / 12), dropout backward (16), mse backward (16), softmax backward rows (12)"""
    c = capi()
    rows, L = 32769, 1024
    n = rows * L + 3                       # 33 555 459 elements: 12 n and 16 n both exceed 384 Mi; n % 4 == 3, rows * L % 4 == 0
    assert 12 * (n - 3) > (384 << 20)
    x, g, d0 = _ramp(n, 2039, 1 / 512, 1000), _ramp(n, 1021, 1 / 256, 500), _ramp(n, 509, 1 / 128, 250)
    X, G = put(dev, x), put(dev, g)

    def run(launch, nn=n, shape=None):
        shape = shape or (nn,)
        w = Window(dev, (nn,), d0[:nn])
        launch(view(w.base, w.first, shape))
        return w.read()
    vs = lambda a, shape: view(a, 0, shape)
    # relu backward (+=: 16 n bytes) and the in-place mask (12 n)
    want = d0 + np.where(x > 0, g, np.float32(0) * g)
    assert np.array_equal(run(lambda d: c.relu_bwd(dev, d, G, X)), want)
    assert np.array_equal(run(lambda d: c.relu_mask_inplace(dev, d, X)), np.where(x > 0, d0, np.float32(0) * d0))
    # dropout backward with x standing in for a 0 / 1 noise buffer of the same size
    close(run(lambda d: c.dropout_bwd(dev, d, G, X, 0.5, True)), d0.astype(np.float64) + g.astype(np.float64) * x)
    assert np.array_equal(run(lambda d: c.dropout_bwd(dev, d, G, None, 0.0, True)), d0 + g)
    # mse backward, sum reduction: d += (2 (x - t)) g0, every step one f32 rounding
    g0 = np.float32(0.75)
    got = run(lambda d: c.mse_bwd(dev, d, put(dev, np.array([g0])), X, G, "sum"))
    close(got, d0.astype(np.float64) + 2.0 * (x.astype(np.float64) - g) * 0.75)
    del got
    # binary backward, same shape, mul: d += g * o over n - 3 elements (float4 kernel)
    m = n - 3
    got = run(lambda d: c.binary_bwd_left(dev, "mul", d, vs(G, (m,)), vs(X, (m,))), m)
    close(got, d0[:m].astype(np.float64) + g[:m].astype(np.float64) * x[:m])
    # ... and add (MODE 0, no operand)
    assert np.array_equal(run(lambda d: c.binary_bwd_left(dev, "add", d, vs(G, (m,))), m), d0[:m] + g[:m])
    del got
    # softmax backward over (32769, 1024): y = a valid probability row pattern, dx += y (g - sum(g y))
    y = (np.abs(x[:m]) + np.float32(0.5)).reshape(rows, L)
    y /= y.sum(axis=1, keepdims=True, dtype=np.float64).astype(np.float32)
    Y = put(dev, y)
    got = run(lambda d: c.softmax_bwd(dev, d, vs(G, (rows, L)), Y, 1), m, (rows, L)).reshape(rows, L)
    g2 = g[:m].reshape(rows, L).astype(np.float64)
    ref = d0[:m].reshape(rows, L) + y * (g2 - (g2 * y).sum(axis=1, keepdims=True))
    tolerance.assert_contraction("dispatch/past_cache/softmax_bwd", got, ref, L, float(np.abs(g).max()), float(y.max()), epilogue=True)
    got = run(lambda d: c.log_softmax_bwd(dev, d, vs(G, (rows, L)), Y, 1), m, (rows, L)).reshape(rows, L)
    ref = d0[:m].reshape(rows, L) + g2 - np.exp(y.astype(np.float64)) * g2.sum(axis=1, keepdims=True)
    tolerance.assert_contraction("dispatch/past_cache/log_softmax_bwd", got, ref, L, float(np.abs(g).max()), float(np.exp(y.max())), epilogue=True)
