"""nk_quant_mx_* (csrc/nk_quant_mx.h) against tests/mx_oracle.py.  K = 32 is a tail-only slab, 160 one slab and a tail, 384 an odd
number of slabs, 736 a tail where the skinny kernel's eight waves split K; N = 1, 17, 289 is less than a fragment, two fragments and a
second block of 256 weight rows; M = 1, 5, 16 is the skinny class, 17, 33, 129 the wide class at MT = 2, 4, 8 with a second block row.
exact_data is lossless in both formats and every sum of its products is an integer multiple of 2^-4 below 2^24 units, so any summation
order is exact and the device must equal the f64 product EXACTLY; every (row, block) carries its own scale and x is not symmetric in
k, so a wrong lane-k mapping, nibble order or scale byte shows."""
import ctypes
import functools

import numpy as np
import pytest

import mx_oracle as O
from test_gpu_quant_linear import _each, rows_of, same_bits, strided

pytestmark = pytest.mark.gpu

KS, NS, MS, NAN = (32, 160, 384, 736), (1, 17, 289), (1, 5, 16, 17, 33, 129), float("nan")


@functools.lru_cache(maxsize=None)
def exact_data(K):
    """x (129, K): integers in [-8, 8] times 2^j per block, j in [-1, 1], a +-8 in every block; W (289, K): E2M1 values times 2^j per
    block, j in [-2, 2], a +-4 or +-6 in every block; integer bias.  |product| <= 8 * 2 * 6 * 4 = 384, K * 384 * 2^4 < 2^24."""
    rng = np.random.default_rng(K)
    def blocks(rows, grid, top, jmax):
        v = rng.choice(grid, (rows, K // 32, 32))
        at = rng.integers(0, 32, (rows, K // 32))
        np.put_along_axis(v, at[:, :, None], rng.choice(top, (rows, K // 32, 1)), axis=2)
        v *= rng.choice([-1.0, 1.0], v.shape) * 2.0 ** rng.integers(-jmax, jmax + 1, (rows, K // 32, 1))
        return v.reshape(rows, K).astype(np.float32)
    out = (blocks(129, np.arange(9.0), [8.0], 1), blocks(289, O.FP4, [4.0, 6.0], 2), rng.integers(-8, 9, 289).astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def random_data(K):   # normal data, log-normal scales per row and per block; x row 3 is zero, x[5, 7] huge
    rng = np.random.default_rng(1000 + K)
    def scaled(rows):
        return (rng.standard_normal((rows, K // 32, 32)) * np.exp(rng.normal(0, 2, (rows, 1, 1)) + rng.normal(0, 1, (rows, K // 32, 1)))).reshape(rows, K).astype(np.float32)
    x, W = scaled(129), scaled(289)
    x[3] = 0
    x[5, 7] = 3e30
    out = (x, W, rng.standard_normal(289).astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(kind, K, with_bias=True):
    """(packed bytes, scale bytes, f64 product (129, 289), sum of magnitudes): computed once, shared, never written"""
    x, W, bias = (exact_data if kind == "exact" else random_data)(K)
    b, e = O.pack(W)
    return (b, e) + O.forward64(x, b, e, bias if with_bias else None)


def as_words(a):   # a uint8 array as the f32 words the library passes around
    flat = np.ascontiguousarray(a, np.uint8).ravel()
    return np.concatenate([flat, np.zeros(-flat.size % 4, np.uint8)]).view(np.float32)


def device_weight(dev, kind, K, N):
    b, e = reference(kind, K)[:2]
    return dev.array(as_words(b[:N])), dev.array(as_words(e[:N]))


def mx(dev, capi, x, qw, sw, bias, M, N, K, ldx=None, ldy=None, xoff=0, yoff=0):
    """y (M, N) of one call: x out of a NaN-filled matrix of row stride ldx, y into a NaN-filled one whose other elements must stay NaN"""
    ldx, ldy = ldx or K, ldy or N
    xo, xv = strided(dev, np.ascontiguousarray(x[:M]), ldx, xoff, fill=np.float32(NAN))
    y = dev.full((yoff + M * ldy + 4,), NAN)
    capi.quant_mx_linear_fwd(dev, xv, ldx, qw, sw, bias, y.view_offset(yoff), ldy, M, N, K)
    out = y.numpy()
    assert np.isnan(out).sum() == out.size - M * N, "wrote outside its (M, N) block or left a NaN in it"
    return rows_of(out, M, N, ldy, yoff)


@pytest.mark.parametrize("R,K", ((1, 32), (17, 160), (33, 384)))
def test_pack_unpack_and_rows_are_the_oracle(dev, R, K):
    from neuronika_amd import capi
    a = np.array(random_data(K)[0][:R])
    if R > 1:
        a[1, :32] = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0] * 4       # every E2M1 tie and the saturating 7 (absmax 7: e = 127)
    for ld, off in ((K, 0), (K + 3, 1)):            # 16-byte loads; scalar loads out of a wider matrix aligned to 4 bytes only
        ao, av = strided(dev, a, ld, off)
        for fn, (code, e) in ((capi.quant_mx_pack, O.pack(a)), (capi.quant_mx_rows, O.quantise_rows(a))):
            q, s = dev.full((code.size // 4 + 4,), NAN), dev.full((e.size // 4 + 5,), NAN)
            fn(dev, av, ld, q, s, R, K)
            gq, gs = q.numpy().view(np.uint8), s.numpy().view(np.uint8)
            assert np.array_equal(gq[:code.size], code.ravel()) and np.array_equal(gs[:e.size], e.ravel()), (fn.__name__, ld)
    b, e = O.pack(a)
    assert b.size == 4 * capi.quant_mx_words(R, K) and (e.size + 3) // 4 == capi.quant_mx_scales(R, K)
    qw, sw = dev.array(as_words(b)), dev.array(as_words(e))
    for ld, off in ((K, 0), (K + 5, 3)):
        out = dev.full((off + R * ld + 4,), NAN)
        capi.quant_mx_unpack(dev, qw, sw, out.view_offset(off), ld, R, K)
        got = out.numpy()
        assert same_bits(rows_of(got, R, K, ld, off), O.unpack(b, e)) and np.isnan(got).sum() == got.size - R * K, "w^ differs (ldw %d)" % ld


def _exact_case(dev, capi, K, case):
    N, M = case
    x, _, bias = exact_data(K)
    qw, sw = device_weight(dev, "exact", K, N)
    got = mx(dev, capi, x, qw, sw, dev.array(bias[:N]), M, N, K)
    assert np.array_equal(got.astype(np.float64), reference("exact", K)[2][:M, :N]), "with a bias"
    got = mx(dev, capi, x, qw, sw, None, M, N, K, ldy=N + 3, yoff=1)                 # scalar stores into a wider, unaligned y
    assert np.array_equal(got.astype(np.float64), reference("exact", K, False)[2][:M, :N]), "without a bias, ldy = N + 3"


@pytest.mark.parametrize("K", KS)
def test_integer_data_gives_the_f64_product_exactly(dev, K):
    from neuronika_amd import capi
    _each([(N, M) for N in NS for M in MS], _exact_case, dev, capi, K)


@pytest.mark.parametrize("K", (160, 736))
def test_random_data_within_the_f32_summation_bound(dev, K):
    """|y - f64| <= 2 (K + 2) 2^-24 (sum_k |x^ w^| + |bias|): an f32 sum of K terms in any order, rounded or truncated"""
    from neuronika_amd import capi
    x, _, bias = random_data(K)
    _, _, want, mags = reference("random", K)
    worst = 0.0
    for N in (17, 289):
        qw, sw = device_weight(dev, "random", K, N)
        for M in (5, 16, 33, 129):
            err = np.abs(mx(dev, capi, x, qw, sw, dev.array(bias[:N]), M, N, K).astype(np.float64) - want[:M, :N])
            worst = max(worst, float((err / np.maximum(mags[:M, :N], 1e-300)).max()) * 2.0 ** 24)
            assert (err <= 2 * (K + 2) * 2.0 ** -24 * mags[:M, :N]).all(), (N, M, worst)
    print("K = %d: largest |y - f64| / (2^-24 sum|x^ w^|) = %.3f" % (K, worst))


@pytest.mark.parametrize("small,large", ((5, 16), (33, 129)))
def test_bits_do_not_depend_on_M_strides_or_alignment(dev, small, large):
    from neuronika_amd import capi
    K, N = 736, 289
    x, _, bias = random_data(K)
    qw, sw = device_weight(dev, "random", K, N)
    db = dev.array(bias)
    base = mx(dev, capi, x, qw, sw, db, large, N, K)
    assert same_bits(mx(dev, capi, x, qw, sw, db, small, N, K), base[:small]), "rows of the M = %d call differ from M = %d" % (large, small)
    assert same_bits(mx(dev, capi, x, qw, sw, db, large, N, K, ldx=K + 7, xoff=1, ldy=N + 2, yoff=3), base), "ldx / ldy / alignment change the bits"


@pytest.mark.parametrize("M", (5, 33))
def test_captured_replay_gives_the_eager_bits(dev, M):
    from neuronika_amd import capi
    K, N = 736, 289
    x, _, bias = random_data(K)
    qw, sw = device_weight(dev, "random", K, N)
    X, db, y = dev.array(np.ascontiguousarray(x[:M])), dev.array(bias), dev.full((M * N,), NAN)
    capi.quant_mx_linear_fwd(dev, X, K, qw, sw, db, y, N, M, N, K)   # warms the workspace
    eager = y.numpy()
    gh = ctypes.c_void_p(); dev.sync()
    capi.check(capi.lib.nk_graph_begin(dev.h))
    try:
        capi.quant_mx_linear_fwd(dev, X, K, qw, sw, db, y, N, M, N, K)
    finally:
        capi.check(capi.lib.nk_graph_end(dev.h, ctypes.byref(gh)))
    for _ in range(3):
        y.fill(NAN)
        capi.check(capi.lib.nk_graph_launch(gh)); dev.sync()
        assert same_bits(y.numpy(), eager), "a replay differs from the eager call"
    capi.check(capi.lib.nk_graph_destroy(gh))


@pytest.mark.parametrize("M", (5, 33))
def test_mx_linear_through_the_tape(dev, M):
    import neuronika_amd
    from neuronika_amd import capi
    nk = neuronika_amd.tape; tdev = nk.Device(0)
    lin = nk.nn.Linear(tdev, 160, 67, 11)
    layer = nk.nn.MxLinear(lin)
    x = np.ascontiguousarray(random_data(160)[0][:M])
    y = layer.forward(nk.from_ndarray(tdev, x)); y.forward()
    b, e = O.pack(lin.weight.data())
    assert same_bits(layer.dequantize().data(), O.unpack(b, e)), "dequantize() is not unpack"
    want = mx(dev, capi, x, dev.array(as_words(b)), dev.array(as_words(e)), dev.array(lin.bias.data()), M, 67, 160)
    assert same_bits(y.data(), want), "the layer is not the C entry"
