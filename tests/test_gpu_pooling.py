"""nk_max_pool_* / nk_avg_pool_* through the C ABI (`capi`) against tests/pooling_oracle.py, every kernel class and every
specialised instantiation under its own test id: windowed (2/2/0, 3/2/0, 3/2/1, 3/1/0, 3/1/1, a tall window, one row, ragged out_W),
plane (L = 49, 64, 100, 130, 3136, above a block's reach ragged and not), generic (per-axis k / s / p, nd = 1 and 3, widths not
divisible by 4) and all of them again with every pointer one float past a 16-byte boundary.  Max forward: y and idx EQUAL the oracle.
Max backward: exact on integer-valued g; otherwise, like the average passes, err_gpu <= max(2 * err_cpu32, 1e-6 * scale) against
the f64 oracle (margins recorded as `pooling:*`).  `+=` into a non-zero dx, `_assign` into a NaN-filled one, every call twice."""
import zlib

import numpy as np
import pytest

import pooling_oracle as P

pytestmark = pytest.mark.gpu

# id -> (x_shape, kernel, stride, padding)
CASES = {
    "windowed-k2s2p0": ((3, 5, 16, 24), (2, 2), (2, 2), (0, 0)),
    "windowed-k3s2p0-scalar-stores": ((2, 3, 17, 20), (3, 3), (2, 2), (0, 0)),
    "windowed-k3s2p1": ((2, 4, 18, 24), (3, 3), (2, 2), (1, 1)),
    "windowed-k3s2p1-ragged-out-width": ((2, 3, 10, 20), (3, 3), (2, 2), (1, 1)),
    "windowed-k3s1p1": ((2, 3, 9, 16), (3, 3), (1, 1), (1, 1)),
    "windowed-k3s1p0": ((2, 3, 9, 16), (3, 3), (1, 1), (0, 0)),
    "windowed-1d-k3s2p1": ((3, 4, 40), (3,), (2,), (1,)),
    "windowed-1d-k2s2p0": ((3, 4, 64), (2,), (2,), (0,)),
    "windowed-tall-k5x3s3x2p2x1": ((2, 2, 15, 16), (5, 3), (3, 2), (2, 1)),
    "windowed-3d-depth-one-k3s2p1": ((2, 3, 1, 12, 16), (1, 3, 3), (1, 2, 2), (0, 1, 1)),
    "windowed-many-planes-k3s2p1": ((8, 64, 28, 28), (3, 3), (2, 2), (1, 1)),
    "generic-2d-k5x4s3x2p2x2": ((2, 3, 13, 10), (5, 4), (3, 2), (2, 2)),
    "generic-width-11-k3s2p1": ((2, 3, 9, 11), (3, 3), (2, 2), (1, 1)),
    "generic-width-7-k2s2p0-floor-drops-a-column": ((2, 3, 7, 7), (2, 2), (2, 2), (0, 0)),
    "generic-1d-k4s3p2": ((2, 3, 19), (4,), (3,), (2,)),
    "generic-3d-k3x2x3s2x1x2p1x1x0": ((2, 2, 5, 7, 9), (3, 2, 3), (2, 1, 2), (1, 1, 0)),
    "generic-3d-k2s2p0": ((1, 2, 6, 8, 8), (2, 2, 2), (2, 2, 2), (0, 0, 0)),
    "generic-k1s1p0": ((2, 2, 5, 6), (1, 1), (1, 1), (0, 0)),
    "plane-L49": ((4, 37, 7, 7), (7, 7), (7, 7), (0, 0)),
    "plane-L64": ((4, 33, 8, 8), (8, 8), (8, 8), (0, 0)),
    "plane-L100": ((2, 3, 10, 10), (10, 10), (10, 10), (0, 0)),
    "plane-L130": ((2, 3, 10, 13), (10, 13), (10, 13), (0, 0)),
    "plane-L3136": ((2, 5, 56, 56), (56, 56), (56, 56), (0, 0)),
    "plane-L16637-ragged-beyond-a-wave": ((1, 3, 131, 127), (131, 127), (131, 127), (0, 0)),
    "plane-L17408-beyond-a-wave": ((1, 2, 136, 128), (136, 128), (136, 128), (0, 0)),
    "plane-1d-L50": ((3, 4, 50), (50,), (50,), (0,)),
    "plane-3d-L64": ((2, 3, 4, 4, 4), (4, 4, 4), (4, 4, 4), (0, 0, 0)),
    "plane-L1-one-element": ((3, 5, 1, 1), (1, 1), (1, 1), (0, 0)),
}
OFFSET_CASES = ["windowed-k2s2p0", "windowed-k3s2p1", "windowed-k3s1p1", "generic-2d-k5x4s3x2p2x2", "plane-L49", "plane-L64", "plane-L3136",
                "plane-L17408-beyond-a-wave"]
GUARD = np.float32(-12345.5)
LEAD, TAIL = 4, 5


def _check(got, want, want32, what, scale):
    from conftest import record_margin
    err_gpu, err_cpu = float(np.abs(got - want).max()), float(np.abs(want32.astype(np.float64) - want).max())
    record_margin("pooling:" + what, err_gpu, err_cpu, 1e-6 * scale)
    assert err_gpu <= max(2 * err_cpu, 1e-6 * scale), (what, err_gpu, err_cpu, scale)


class Buffers:
    """device arrays with guard floats on both sides; `off` = 1 moves every tensor one float past a 16-byte boundary"""

    def __init__(self, dev, off):
        self.dev, self.lead, self.held = dev, LEAD + off, []

    def f32(self, a):
        a = np.asarray(a, np.float32)
        host = np.full(self.lead + a.size + TAIL, GUARD, np.float32)
        host[self.lead:self.lead + a.size] = a.ravel()
        buf = self.dev.array(host)
        self.held.append(buf)
        return buf, buf.view_offset(self.lead), a.shape

    def i32(self, a):
        a = np.asarray(a, np.int32)
        host = np.full(self.lead + a.size + TAIL, -77, np.int32)
        host[self.lead:self.lead + a.size] = a.ravel()
        buf = self.dev.int_array(host)
        self.held.append(buf)
        return buf, buf.view_offset(self.lead), a.shape

    def write(self, t, a):
        h = t[0].numpy()
        h[self.lead:-TAIL] = a.ravel()
        t[0].upload(h)

    def read(self, t):
        buf, _, shape = t
        h = buf.numpy()
        guard = GUARD if h.dtype == np.float32 else -77
        assert (h[:self.lead] == guard).all() and (h[-TAIL:] == guard).all(), "a guard word was overwritten"
        return h[self.lead:-TAIL].reshape(shape).copy()


def _twice(fn, bufs, outs):
    """run the call twice from the same starting contents: the outputs must be bit-equal"""
    start = [bufs.read(t) for t in outs]
    fn()
    first = [bufs.read(t) for t in outs]
    for t, s in zip(outs, start):
        bufs.write(t, s)
    fn()
    second = [bufs.read(t) for t in outs]
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes(), "the second run differs from the first"
    return first


def _run(dev, name, off):
    from neuronika_amd import capi as c
    shape, k, s, p = CASES[name]
    tag = name + ("/offset" if off else "")
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    x = rng.standard_normal(shape).astype(np.float32)
    x.ravel()[rng.integers(0, x.size, x.size // 5)] = np.float32(0.5)     # ties
    oshape = P.out_shape(shape, k, s, p)
    assert c.pool_out_shape(shape, k, s, p) == oshape
    B = Buffers(dev, off)
    X = B.f32(x)

    # ---- max forward: exact
    y_want, i_want = P.max_pool_fwd(x, k, s, p)
    Y, I = B.f32(np.full(oshape, np.nan)), B.i32(np.full(oshape, -5))
    y, i = _twice(lambda: c.max_pool_fwd(dev, X[1], shape, Y[1], I[1], k, s, p), B, [Y, I])
    np.testing.assert_array_equal(y, y_want)
    np.testing.assert_array_equal(i, i_want)
    Y2 = B.f32(np.full(oshape, np.nan))
    c.max_pool_fwd(dev, X[1], shape, Y2[1], None, k, s, p)                 # idx = NULL
    np.testing.assert_array_equal(B.read(Y2), y_want)

    # ---- max backward: exact on integers (+= into integers, assign over NaN), the rule on real g
    gi = rng.integers(-4, 5, oshape).astype(np.float32)
    d0 = rng.integers(-3, 4, shape).astype(np.float32)
    DX, GI = B.f32(d0), B.f32(gi)
    (dx,) = _twice(lambda: c.max_pool_bwd(dev, DX[1], shape, GI[1], I[1], k, s, p), B, [DX])
    np.testing.assert_array_equal(dx, d0 + P.max_pool_bwd(gi, i_want, shape))
    DXA = B.f32(np.full(shape, np.nan))
    (dxa,) = _twice(lambda: c.max_pool_bwd(dev, DXA[1], shape, GI[1], I[1], k, s, p, assign=True), B, [DXA])
    np.testing.assert_array_equal(dxa, P.max_pool_bwd(gi, i_want, shape))
    g = rng.standard_normal(oshape).astype(np.float32)
    Gd = B.f32(g)
    DXR = B.f32(np.full(shape, np.nan))
    c.max_pool_bwd(dev, DXR[1], shape, Gd[1], I[1], k, s, p, assign=True)
    want64, want32 = P.max_pool_bwd(g.astype(np.float64), i_want, shape), P.max_pool_bwd(g, i_want, shape)
    _check(B.read(DXR), want64, want32, "max dx " + tag, max(1.0, float(np.abs(want64).max())))

    # ---- average, both divisors
    for cip in (True, False):
        t2 = tag + ("/include_pad" if cip else "/exclude_pad")
        a64, a32 = P.avg_pool_fwd(x.astype(np.float64), k, s, p, cip), P.avg_pool_fwd(x, k, s, p, cip)
        YA = B.f32(np.full(oshape, np.nan))
        (ya,) = _twice(lambda: c.avg_pool_fwd(dev, X[1], shape, YA[1], k, s, p, cip), B, [YA])
        _check(ya, a64, a32, "avg y " + t2, float(np.abs(x).max()))
        b64, b32 = P.avg_pool_bwd(g.astype(np.float64), shape, k, s, p, cip), P.avg_pool_bwd(g, shape, k, s, p, cip)
        d1 = rng.standard_normal(shape).astype(np.float32)
        DA = B.f32(d1)
        (da,) = _twice(lambda: c.avg_pool_bwd(dev, DA[1], shape, Gd[1], k, s, p, cip), B, [DA])
        scale = max(1.0, float(np.abs(b64).max()) + float(np.abs(d1).max()))
        _check(da, d1 + b64, (d1 + b32).astype(np.float32), "avg dx += " + t2, scale)
        DB = B.f32(np.full(shape, np.nan))
        (db,) = _twice(lambda: c.avg_pool_bwd(dev, DB[1], shape, Gd[1], k, s, p, cip, assign=True), B, [DB])
        _check(db, b64, b32, "avg dx = " + t2, max(1.0, float(np.abs(b64).max())))
    dev.sync()


@pytest.mark.parametrize("name", list(CASES))
def test_class(dev, name):
    _run(dev, name, 0)


@pytest.mark.parametrize("name", OFFSET_CASES)
def test_pointers_offset_by_one_float(dev, name):
    """one float past a 16-byte boundary: no kernel with 16-byte accesses may be chosen; guard words on both sides of every tensor"""
    _run(dev, name, 1)


@pytest.mark.parametrize("name", ["windowed-k3s2p1", "windowed-k2s2p0", "windowed-k3s1p1", "windowed-k3s2p0-scalar-stores",
                                  "generic-2d-k5x4s3x2p2x2", "generic-3d-k3x2x3s2x1x2p1x1x0", "plane-L49", "plane-L64", "plane-L3136",
                                  "plane-L16637-ragged-beyond-a-wave"])
def test_nan_inf_and_all_minus_inf_windows(dev, name):
    from neuronika_amd import capi as c
    shape, k, s, p = CASES[name]
    rng = np.random.default_rng(11)
    x = rng.standard_normal(shape).astype(np.float32)
    plane = x.reshape(shape[0] * shape[1], -1)
    r = rng.random(plane.shape)
    plane[r < 0.10] = np.nan
    plane[(r >= 0.10) & (r < 0.25)] = -np.inf
    plane[(r >= 0.25) & (r < 0.30)] = np.inf
    plane[0, :] = -np.inf                                                  # a plane of nothing but -inf
    if plane.shape[0] > 1:
        plane[1, :] = rng.standard_normal(plane.shape[1])
        plane[1, plane.shape[1] // 2:] = np.nan                            # the first NaN of many
    if plane.shape[0] > 2:
        plane[2, :] = rng.standard_normal(plane.shape[1])                  # a finite plane stays finite
    y_want, i_want = P.max_pool_fwd(x, k, s, p)
    oshape = y_want.shape
    X, Y, I = dev.array(x), dev.full(oshape, 7.0), dev.int_zeros(oshape)
    c.max_pool_fwd(dev, X, shape, Y, I, k, s, p)
    np.testing.assert_array_equal(Y.numpy(), y_want)
    np.testing.assert_array_equal(I.numpy(), i_want)
    assert (y_want.reshape(plane.shape[0], -1)[0] == -np.inf).all()
    g = rng.integers(-4, 5, oshape).astype(np.float32)
    DX = dev.full(shape, np.nan)
    c.max_pool_bwd(dev, DX, shape, dev.array(g), I, k, s, p, assign=True)
    np.testing.assert_array_equal(DX.numpy(), P.max_pool_bwd(g, i_want, shape))
    # the average of a window that holds a non-finite value is non-finite there and nowhere else
    ya = dev.full(oshape, 7.0)
    c.avg_pool_fwd(dev, X, shape, ya, k, s, p, True)
    with np.errstate(invalid="ignore"):
        want = P.avg_pool_fwd(x, k, s, p, True)
    got = ya.numpy()
    np.testing.assert_array_equal(np.isfinite(got), np.isfinite(want))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))


@pytest.mark.parametrize("shape", [(0, 3, 8, 8), (2, 0, 8, 8), (0, 0, 7)])
def test_no_planes_writes_nothing(dev, shape):
    from neuronika_amd import capi as c
    nd = len(shape) - 2
    k, s, p = (2,) * nd, (2,) * nd, (0,) * nd
    assert c.pool_out_shape(shape, k, s, p) == P.out_shape(shape, k, s, p)
    X, Y, I, DX = dev.full((8,), 3.0), dev.full((8,), 3.0), dev.int_array(np.full(8, 3)), dev.full((8,), 3.0)
    c.max_pool_fwd(dev, X, shape, Y, I, k, s, p)
    c.avg_pool_fwd(dev, X, shape, Y, k, s, p)
    for assign in (False, True):
        c.max_pool_bwd(dev, DX, shape, Y, I, k, s, p, assign=assign)
        c.avg_pool_bwd(dev, DX, shape, Y, k, s, p, assign=assign)
    assert (Y.numpy() == 3.0).all() and (I.numpy() == 3).all() and (DX.numpy() == 3.0).all()


REJECTED = {
    "window-0": ((2, 3, 8, 8), (0, 2), (2, 2), (0, 0)),
    "stride-0": ((2, 3, 8, 8), (2, 2), (0, 2), (0, 0)),
    "padding-above-half-the-window": ((2, 3, 8, 8), (2, 2), (2, 2), (2, 0)),
    "padding-negative": ((2, 3, 8, 8), (3, 3), (2, 2), (-1, 0)),
    "window-beyond-the-padded-extent": ((2, 3, 2, 8), (5, 3), (1, 1), (1, 1)),
    "extent-0": ((2, 3, 0, 8), (2, 2), (2, 2), (1, 1)),
    "nd-0": ((2, 3), (), (), ()),
    "nd-4": ((2, 3, 4, 4, 4, 4), (1,) * 4, (1,) * 4, (0,) * 4),
    "negative-N": ((-1, 3, 8), (2,), (2,), (0,)),
    "plane-beyond-31-bits": ((1, 1, 65536, 65536), (1, 1), (1, 1), (0, 0)),
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_rejected_arguments_leave_the_outputs_untouched(dev, name):
    from neuronika_amd import capi as c
    shape, k, s, p = REJECTED[name]
    X, Y, I, DX = dev.full((64,), 3.0), dev.full((64,), 3.0), dev.int_array(np.full(64, 3)), dev.full((64,), 3.0)
    calls = [lambda: c.pool_out_shape(shape, k, s, p), lambda: c.max_pool_fwd(dev, X, shape, Y, I, k, s, p),
             lambda: c.avg_pool_fwd(dev, X, shape, Y, k, s, p), lambda: c.max_pool_bwd(dev, DX, shape, Y, I, k, s, p),
             lambda: c.max_pool_bwd(dev, DX, shape, Y, I, k, s, p, assign=True), lambda: c.avg_pool_bwd(dev, DX, shape, Y, k, s, p),
             lambda: c.avg_pool_bwd(dev, DX, shape, Y, k, s, p, assign=True)]
    for call in calls:
        with pytest.raises(c.NeuronikaHipError) as e:
            call()
        assert e.value.code == 1                                           # NK_ERR_INVALID
    dev.sync()
    assert (Y.numpy() == 3.0).all() and (I.numpy() == 3).all() and (DX.numpy() == 3.0).all()


def test_null_pointers_are_rejected(dev):
    from neuronika_amd import capi as c
    shape, k, s, p = (2, 3, 8, 8), (2, 2), (2, 2), (0, 0)
    X, Y, I = dev.full((384,), 1.0), dev.full((96,), 3.0), dev.int_zeros((96,))
    for call in (lambda: c.max_pool_fwd(dev, None, shape, Y, I, k, s, p), lambda: c.max_pool_fwd(dev, X, shape, None, I, k, s, p),
                 lambda: c.max_pool_bwd(dev, X, shape, Y, None, k, s, p), lambda: c.avg_pool_bwd(dev, None, shape, Y, k, s, p)):
        with pytest.raises(c.NeuronikaHipError):
            call()
    assert (Y.numpy() == 3.0).all()
