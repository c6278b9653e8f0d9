"""nk_upsample_* through the C ABI (`capi`) against tests/upsample_oracle.py, BIT FOR BIT: y, dx from `_assign` (over a NaN-filled
destination) and dx from `+=` into a non-zero one, for every shape of the oracle's list (the smallest that reach the nearest x2,
vector and generic classes, in = 1, out = 1, down-sampling, 1 to 3 axes), both modes and both settings of align_corners.  Every
call runs twice from the same contents (determinism), between guard words, and once more with every pointer one float past a 16-byte
boundary - the generic class - which must give the bits of the aligned call (class agreement).  Few test ids, many cases: each test
walks its cases, runs every one of them and names the ones that failed."""
import ctypes
import functools

import numpy as np
import pytest

import upsample_oracle as U

pytestmark = pytest.mark.gpu

GUARD = np.float32(-12345.5)
LEAD, TAIL = 4, 5
CASES = [(shape, size, mode, align) for shape, size in U.SHAPES for mode, align in U.variants()]


def _each(cases, check, *args):
    """run `check` on every case; one failure does not hide the next, and the message names each"""
    failed = []
    for case in cases:
        try:
            check(*args, case)
        except AssertionError as e:
            failed.append("%r: %s" % (case, str(e)[:300]))
    assert not failed, "\n".join(failed)


def _rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _reference(shape, size, mode, align):
    """(x, g, d0, y, total, d0 + total): computed once, shared, never written"""
    x, g, d0 = _rnd(shape, 11), _rnd(shape[:2] + size, 12), _rnd(shape, 13)
    y, total = U.forward(x, size, mode, align), U.backward(g, shape, mode, align)
    out = (x, g, d0, y, total, d0 + total)
    for a in out:
        a.setflags(write=False)
    return out


class Buffers:
    """device arrays with guard floats on both sides; `off` = 1 moves every tensor one float past a 16-byte boundary"""

    def __init__(self, dev, off):
        self.dev, self.lead = dev, LEAD + off

    def f32(self, a):
        a = np.asarray(a, np.float32)
        host = np.full(self.lead + a.size + TAIL, GUARD, np.float32)
        host[self.lead:self.lead + a.size] = a.ravel()
        buf = self.dev.array(host)
        return buf, buf.view_offset(self.lead), a.shape

    def write(self, t, a):
        h = t[0].numpy()
        h[self.lead:-TAIL] = np.asarray(a, np.float32).ravel()
        t[0].upload(h)

    def read(self, t):
        buf, _, shape = t
        h = buf.numpy()
        assert (h[:self.lead] == GUARD).all() and (h[-TAIL:] == GUARD).all(), "a guard word was overwritten"
        return h[self.lead:-TAIL].reshape(shape).copy()


def _twice(fn, bufs, out):
    start = bufs.read(out)
    fn()
    first = bufs.read(out)
    bufs.write(out, start)
    fn()
    assert bufs.read(out).tobytes() == first.tobytes(), "the second run differs from the first"
    return first


def _three_passes(dev, shape, size, mode, align, off, x, g, d0):
    from neuronika_amd import capi as c
    B = Buffers(dev, off)
    X, G = B.f32(x), B.f32(g)
    Y, DA, DP = B.f32(np.full(shape[:2] + size, np.nan)), B.f32(np.full(shape, np.nan)), B.f32(d0)
    y = _twice(lambda: c.upsample_fwd(dev, X[1], shape, Y[1], size, mode, align), B, Y)
    da = _twice(lambda: c.upsample_bwd(dev, DA[1], shape, G[1], size, mode, align, assign=True), B, DA)
    dp = _twice(lambda: c.upsample_bwd(dev, DP[1], shape, G[1], size, mode, align), B, DP)
    assert B.read(X).tobytes() == np.asarray(x).tobytes() and B.read(G).tobytes() == np.asarray(g).tobytes()   # inputs and their guards
    return y, da, dp


def _check_bits(dev, case):
    shape, size, mode, align = case
    x, g, d0, y_want, total, plus = _reference(*case)
    y, da, dp = _three_passes(dev, shape, size, mode, align, 0, x, g, d0)
    assert y.tobytes() == y_want.tobytes(), np.abs(y - y_want).max()
    assert da.tobytes() == total.tobytes(), np.abs(da - total).max()
    assert dp.tobytes() == plus.tobytes(), np.abs(dp - plus).max()
    y1, da1, dp1 = _three_passes(dev, shape, size, mode, align, 1, x, g, d0)             # the generic class
    assert y1.tobytes() == y.tobytes() and da1.tobytes() == da.tobytes() and dp1.tobytes() == dp.tobytes()
    dev.sync()


ALONE = [((2, 3, 4, 4), (8, 8), "nearest", False), ((2, 3, 4, 4), (8, 8), "linear", False), ((2, 3, 5), (8,), "linear", True)]


def _check_a_sample_alone_gets_the_bits_it_gets_in_the_batch(dev, case):
    from neuronika_amd import capi as c
    shape, size, mode, align = case
    x, g, _, y_want, total, _ = _reference(*case)
    one = (1,) + shape[1:]
    X, G = dev.array(np.ascontiguousarray(x[1:])), dev.array(np.ascontiguousarray(g[1:]))
    Y, DX = dev.full(one[:2] + size, np.nan), dev.full(one, np.nan)
    c.upsample_fwd(dev, X, one, Y, size, mode, align)
    c.upsample_bwd(dev, DX, one, G, size, mode, align, assign=True)
    assert Y.numpy().tobytes() == y_want[1:].tobytes() and DX.numpy().tobytes() == total[1:].tobytes()


def _check_nearest_copies_nan_inf_and_minus_zero_bit_for_bit(dev, case):
    from neuronika_amd import capi as c
    shape, size = case
    x = _rnd(shape, 21)
    flat = x.ravel().view(np.uint32)
    flat[0::7] = 0x7FC01234                                                  # a NaN with a payload
    flat[1::7] = 0xFF800000                                                  # -inf
    flat[2::7] = 0x80000000                                                  # -0.0
    flat[3::7] = 0x7F800000                                                  # +inf
    Y = dev.full(shape[:2] + size, 7.0)
    c.upsample_fwd(dev, dev.array(x), shape, Y, size, "nearest")
    assert Y.numpy().tobytes() == U.forward(x, size, "nearest").tobytes()


NON_FINITE = [((1, 2, 6, 8), (9, 20), "linear", False), ((1, 2, 3, 4, 4), (6, 8, 8), "linear", True), ((2, 3, 5), (8,), "linear", False)]


def _check_a_non_finite_input_under_linear_matches_the_oracle(dev, case):
    """the oracle does the same operations, so NaN stands where its NaN stands and every other value has its bits (the payload and
    sign of a NaN the arithmetic makes are the processor's own: not compared)"""
    from neuronika_amd import capi as c
    shape, size, mode, align = case
    x, g = _rnd(shape, 31), _rnd(shape[:2] + size, 32)
    plane, oplane = int(np.prod(shape[2:])), int(np.prod(size))
    x.ravel()[[1, plane - 2, plane + plane // 2]] = [np.inf, -np.inf, np.nan]     # apart, so that infinities survive beside the NaNs
    g.ravel()[[2, oplane + oplane // 2]] = [np.inf, np.nan]
    Y, DX = dev.full(shape[:2] + size, 7.0), dev.full(shape, 7.0)
    c.upsample_fwd(dev, dev.array(x), shape, Y, size, mode, align)
    c.upsample_bwd(dev, DX, shape, dev.array(g), size, mode, align, assign=True)
    with np.errstate(invalid="ignore"):
        wants = U.forward(x, size, mode, align), U.backward(g, shape, mode, align)
    for got, want in zip((Y.numpy(), DX.numpy()), wants):
        assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        keep = ~np.isnan(want)
        assert got[keep].tobytes() == want[keep].tobytes()


def _check_no_planes_writes_nothing(dev, shape):
    from neuronika_amd import capi as c
    size = (8,) * (len(shape) - 2)
    X, Y, DX = dev.full((8,), 3.0), dev.full((8,), 3.0), dev.full((8,), 3.0)
    for mode in ("nearest", "linear"):
        c.upsample_fwd(dev, X, shape, Y, size, mode)
        for assign in (False, True):
            c.upsample_bwd(dev, DX, shape, X, size, mode, assign=assign)
    dev.sync()
    assert (Y.numpy() == 3.0).all() and (DX.numpy() == 3.0).all()


# id -> (x_shape, out_size, mode, align_corners, nd or None for len(x_shape) - 2)
REJECTED = {
    "nd-0": ((2, 3), (), 0, 0),
    "nd-4": ((2, 3, 4, 4, 4, 4), (8, 8, 8, 8), 0, 0),
    "unknown-mode": ((2, 3, 4, 4), (8, 8), 2, 0),
    "negative-mode": ((2, 3, 4, 4), (8, 8), -1, 0),
    "align-corners-with-nearest": ((2, 3, 4, 4), (8, 8), 0, 1),
    "negative-N": ((-1, 3, 4), (8,), 0, 0),
    "negative-C": ((2, -3, 4), (8,), 1, 0),
    "in-0": ((2, 3, 0, 4), (8, 8), 1, 0),
    "out-0": ((2, 3, 4, 4), (8, 0), 1, 1),
    "out-negative": ((2, 3, 4, 4), (-8, 8), 0, 0),
    "input-plane-beyond-31-bits": ((1, 1, 65536, 32768), (4, 4), 0, 0),
    "output-plane-beyond-31-bits": ((1, 1, 4, 4), (65536, 32768), 1, 0),
}


def _check_rejected_arguments_leave_the_destinations_untouched(dev, name):
    from neuronika_amd import capi as c
    shape, size, mode, align = REJECTED[name]
    X, Y, DX = dev.full((64,), 3.0), dev.full((64,), 3.0), dev.full((64,), 3.0)
    for call in (lambda: c.upsample_fwd(dev, X, shape, Y, size, mode, align), lambda: c.upsample_bwd(dev, DX, shape, X, size, mode, align),
                 lambda: c.upsample_bwd(dev, DX, shape, X, size, mode, align, assign=True)):
        try:
            call()
        except c.NeuronikaHipError as e:
            assert e.code == 1                                               # NK_ERR_INVALID
        else:
            raise AssertionError("accepted")
    dev.sync()
    assert (Y.numpy() == 3.0).all() and (DX.numpy() == 3.0).all() and (X.numpy() == 3.0).all()


def _check_out_size_and_the_scales_it_refuses():
    from neuronika_amd import capi as c
    for shape, scale in (((1, 2, 6, 8), 1.5), ((1, 2, 6, 8), (2, 2.5)), ((3, 4, 7), 0.5), ((1, 1, 2, 3, 5), (2.5, 1.4, 1.5)), ((1, 1, 5), 2)):
        assert c.upsample_out_size(shape, scale) == U.out_size(shape, scale), (shape, scale)
    for shape, scale in (((1, 2, 6, 8), float("nan")), ((1, 2, 6, 8), float("inf")), ((1, 2, 6, 8), 0.0), ((1, 2, 6, 8), (2.0, -1.0)),
                         ((1, 2, 6, 8), 0.1), ((1, 2, 0, 8), 2.0), ((-1, 2, 6, 8), 2.0), ((1, 2, 65536, 65536), 2.0), ((1, 2), 2.0)):
        try:
            c.upsample_out_size(shape, scale)
        except c.NeuronikaHipError as e:
            assert e.code == 1, (shape, scale)
        else:
            raise AssertionError("accepted: %r %r" % (shape, scale))


CAPTURED = [((2, 3, 4, 4), (8, 8), "nearest", False), ((1, 2, 6, 8), (9, 20), "linear", False), ((1, 2, 3, 4, 4), (6, 8, 8), "linear", True)]


def _check_forward_and_backward_captured_into_a_graph_replay_the_eager_bits(dev, case):
    from neuronika_amd import capi as c
    shape, size, mode, align = case
    x, g, d0, y_want, total, plus = _reference(*case)
    X, G = dev.array(x), dev.array(g)
    Y, DA, DP = dev.full(shape[:2] + size, np.nan), dev.full(shape, np.nan), dev.array(d0)

    def step():
        c.upsample_fwd(dev, X, shape, Y, size, mode, align)
        c.upsample_bwd(dev, DA, shape, G, size, mode, align, assign=True)
        c.upsample_bwd(dev, DP, shape, G, size, mode, align)

    step()                                                                   # one eager call first
    dev.sync()
    assert Y.numpy().tobytes() == y_want.tobytes() and DP.numpy().tobytes() == plus.tobytes()
    Y.fill(7.0); DA.fill(7.0); DP.upload(np.asarray(d0))
    gh = ctypes.c_void_p()
    dev.sync()
    c.check(c.lib.nk_graph_begin(dev.h))
    try:
        step()
    finally:
        c.check(c.lib.nk_graph_end(dev.h, ctypes.byref(gh)))
    dev.sync()
    assert (Y.numpy() == 7.0).all() and (DA.numpy() == 7.0).all()            # recorded, not run
    c.check(c.lib.nk_graph_launch(gh)); dev.sync()
    got = Y.numpy(), DA.numpy(), DP.numpy()
    c.check(c.lib.nk_graph_destroy(gh))
    assert got[0].tobytes() == y_want.tobytes() and got[1].tobytes() == total.tobytes() and got[2].tobytes() == plus.tobytes()


def test_bits_equal_the_oracle_in_every_class_and_every_call_repeats(dev):
    """every shape, mode and align_corners: y, dx `=` and dx `+=` equal the oracle bit for bit, twice, between guards, aligned (the
    nearest x2 and vector classes where the shape allows) and one float off (generic) with the same bits; a sample alone gets the bits
    it gets in the batch; forward and backward captured into a graph after one eager call replay the eager bits"""
    _each(CASES, _check_bits, dev)
    _each(ALONE, _check_a_sample_alone_gets_the_bits_it_gets_in_the_batch, dev)
    _each(CAPTURED, _check_forward_and_backward_captured_into_a_graph_replay_the_eager_bits, dev)


def test_special_values_empty_tensors_and_refusals(dev):
    """nearest copies a NaN with its payload, the infinities and -0.0 bit for bit; a non-finite input under linear matches the oracle;
    N * C == 0 writes nothing; every NK_ERR_INVALID case returns before any launch with its destination untouched; nk_upsample_out_size
    is floor(in * scale) in f64 and refuses the scales and geometries outside the contract"""
    _each([((2, 3, 4, 4), (8, 8)), ((1, 2, 6, 8), (9, 20)), ((1, 2, 5, 7), (10, 14))], _check_nearest_copies_nan_inf_and_minus_zero_bit_for_bit, dev)
    _each(NON_FINITE, _check_a_non_finite_input_under_linear_matches_the_oracle, dev)
    _each([(0, 3, 4, 4), (2, 0, 4, 4), (0, 0, 5)], _check_no_planes_writes_nothing, dev)
    _each(list(REJECTED), _check_rejected_arguments_leave_the_destinations_untouched, dev)
    _check_out_size_and_the_scales_it_refuses()
