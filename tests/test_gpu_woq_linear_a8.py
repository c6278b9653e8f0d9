"""nk_quant_a8_linear_fwd (csrc/nk_quant_a8.h) against tests/quant_a8_oracle.py: every assertion is exact bit equality.  With g = group,
K = g is less than a stage (for group 0, 32: half a slab), 3 g a partial stage / a half-slab tail, 2048 + g crosses the F boundary of
group 0; N = 1, 5, 67, 130 is less than a fragment, not a multiple of 4 or 16, more than a wave's 32 rows, and 261 a second block of
256 weight rows; M = 1, 16, 17, 40, 129 takes the MT = 1, 2, 4, 8 kernels, their M tails and a second M tile.  Rows of x differ in
magnitude by e^(+-6); row 3 is zero, row 5 the half-way values of quant_oracle.tie_row.  The file stands beside
tests/test_gpu_woq_linear_mma.py, the other many-row path of the quantised layer."""
import ctypes
import functools

import numpy as np
import pytest

import quant_a8_oracle as A
import quant_oracle as Q
from test_gpu_quant_linear import _each, device_format, reference, rows_of, same_bits, strided

pytestmark = pytest.mark.gpu

FORMATS = [(bits, group) for bits in (8, 4) for group in (64, 128, 0)]
NS, MS, NAN = (1, 5, 67, 130, 261), (1, 16, 17, 40, 129), float("nan")


def ks(group):
    g = group or 32
    return (g, 3 * g, 2048 + g)


@functools.lru_cache(maxsize=None)
def x129(K):
    rng = np.random.default_rng(129 + K)
    x = (rng.standard_normal((129, K)) * np.exp(rng.uniform(-6, 6, (129, 1)))).astype(np.float32)
    x[3] = 0
    x[5] = Q.tie_row(K)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def expected(bits, group, K, N, with_bias=True):
    _, b, s, _, bias, _ = reference(bits, group, K, N)
    y = A.forward(x129(K), b, s, bias if with_bias else None, bits, group)
    y.setflags(write=False)
    return y


def a8(dev, capi, x, qw, sc, bias, M, N, K, bits, group, ldx=None, ldy=None, xoff=0):
    """y (M, N) of one call: x out of a NaN-filled matrix of row stride ldx, y into a NaN-filled one whose other elements must stay NaN"""
    ldx, ldy = ldx or K, ldy or N
    xo, xv = strided(dev, np.ascontiguousarray(x[:M]), ldx, xoff, fill=np.float32(NAN))
    y = dev.full((M * ldy + 4,), NAN)
    capi.quant_a8_linear_fwd(dev, xv, ldx, qw, sc, bias, y, ldy, M, N, K, bits, group)
    out = y.numpy()
    assert np.isnan(out).sum() == out.size - M * N, "wrote outside its (M, N) block or left a NaN in it"
    return rows_of(out, M, N, ldy)


def _case(dev, capi, bits, group, case):
    K, N = case
    (qw, sc), db = device_format(dev, capi, bits, group, K, N), dev.array(reference(bits, group, K, N)[4])
    for M in MS:
        assert same_bits(a8(dev, capi, x129(K), qw, sc, db, M, N, K, bits, group), expected(bits, group, K, N)[:M]), "M = %d differs" % M


@pytest.mark.parametrize("bits,group", FORMATS)
def test_bits_of_the_oracle(dev, bits, group):
    """every (K, N, M) runs; the failures of a format are named together"""
    from neuronika_amd import capi
    _each([(K, N) for K in ks(group) for N in NS], _case, dev, capi, bits, group)


@pytest.mark.parametrize("bits,group", FORMATS)
def test_strides_alignment_and_no_bias(dev, bits, group):
    from neuronika_amd import capi
    K, N, M = ks(group)[2], 67, 40
    (qw, sc), db = device_format(dev, capi, bits, group, K, N), dev.array(reference(bits, group, K, N)[4])
    want = expected(bits, group, K, N)[:M]
    # 16-byte loads and 16-byte stores (ldy % 4 == 0) / scalar loads out of an unaligned x and scalar stores
    for ldx, xoff, ldy in ((K + 8, 0, N + 5), (K + 7, 1, N + 6), (K, 0, N + 1)):
        assert same_bits(a8(dev, capi, x129(K), qw, sc, db, M, N, K, bits, group, ldx=ldx, ldy=ldy, xoff=xoff), want), "ldx %d, ldy %d differs" % (ldx, ldy)
    assert same_bits(a8(dev, capi, x129(K), qw, sc, None, M, N, K, bits, group), expected(bits, group, K, N, False)[:M]), "without a bias"


def test_refused_calls_write_nothing(dev):
    from neuronika_amd import capi
    N, K, M = 5, 192, 2
    x, sc, bias, qw = dev.full((M * K,), 1.0), dev.full((N * 6,), 1.0), dev.full((N,), 1.0), dev.full((N * K // 4 + 4,), 0.0)
    y = dev.full((M * N + 4,), NAN)
    for args in ((x, K, qw, sc, bias, y, N, M, N, K, 8, 32),                 # group 32
                 (x, 48, qw, sc, bias, y, N, M, N, 48, 8, 0),                # K = 48
                 (x, K, qw, sc, bias, y, N, M, N, K, 8, 128),                # group 128 does not divide K = 192
                 (x, K, qw, sc, bias, y, N, M, N, K, 3, 64),                 # bits = 3
                 (x, K, qw, sc, bias, y, N, M, N, K, 8, 16),                 # group = 16
                 (x, K, None, sc, bias, y, N, M, N, K, 8, 64),               # null qw
                 (x, K, qw, sc, bias, y, N - 1, M, N, K, 8, 64),             # ldy < N
                 (x, K - 1, qw, sc, bias, y, N, M, N, K, 8, 64),             # ldx < K
                 (x, K, qw.view_offset(1), sc, bias, y, N, M, N, K, 8, 64),  # qw misaligned by 4 bytes
                 (x, K, qw, sc, bias, y, N, -1, N, K, 8, 64),                # M < 0
                 (x, K, qw, sc, bias, y, N, M, 0, K, 8, 64)):                # N = 0
        with pytest.raises(capi.NeuronikaHipError) as e:
            capi.quant_a8_linear_fwd(dev, *args)
        assert e.value.code == 1 and np.isnan(y.numpy()).all(), args[-5:]
    capi.quant_a8_linear_fwd(dev, x, K, qw, sc, bias, y, N, 0, N, K, 8, 64)   # M = 0: an empty success
    assert np.isnan(y.numpy()).all()


@pytest.mark.parametrize("bits", (8, 4))
def test_captured_replay_gives_the_eager_bits(dev, bits):
    from neuronika_amd import capi
    group, N, M = 128, 67, 40
    K = ks(group)[2]
    (qw, sc), db = device_format(dev, capi, bits, group, K, N), dev.array(reference(bits, group, K, N)[4])
    X, y = dev.array(np.ascontiguousarray(x129(K)[:M])), dev.full((M * N,), NAN)
    capi.quant_a8_linear_fwd(dev, X, K, qw, sc, db, y, N, M, N, K, bits, group)   # warms the workspace
    eager = y.numpy()
    assert same_bits(eager.reshape(M, N), expected(bits, group, K, N)[:M])
    gh = ctypes.c_void_p(); dev.sync()
    capi.check(capi.lib.nk_graph_begin(dev.h))
    try:
        capi.quant_a8_linear_fwd(dev, X, K, qw, sc, db, y, N, M, N, K, bits, group)
    finally:
        capi.check(capi.lib.nk_graph_end(dev.h, ctypes.byref(gh)))
    for _ in range(3):
        y.fill(NAN)
        capi.check(capi.lib.nk_graph_launch(gh)); dev.sync()
        assert same_bits(y.numpy(), eager), "a replay differs from the eager call"
    capi.check(capi.lib.nk_graph_destroy(gh))


@pytest.mark.parametrize("bits", (8, 4))
def test_quant_linear_through_the_tape(bits):
    import neuronika_amd
    nk = neuronika_amd.tape; tdev = nk.Device(0)
    lin = nk.nn.Linear(tdev, 256, 67, 11)
    x = np.ascontiguousarray(x129(256)[:17])
    run = lambda layer: (lambda y: (y.forward(), y.data())[1])(layer.forward(nk.from_ndarray(tdev, x)))
    ql = nk.nn.QuantLinear(lin, bits, 128, 8)
    assert ql.act_bits == 8 and nk.nn.QuantLinear(lin, bits, 128).act_bits == 0
    b, s = Q.pack(lin.weight.data(), bits, 128)
    assert same_bits(run(ql), A.forward(x, b, s, lin.bias.data(), bits, 128)), "act_bits = 8 is not the oracle"
    assert same_bits(run(nk.nn.QuantLinear(lin, bits, 128, 0)), run(nk.nn.QuantLinear(lin, bits, 128))), "act_bits = 0 is not the layer as it was"
