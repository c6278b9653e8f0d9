"""The fused-dequant MFMA kernel of nk_quant_linear_fwd (csrc/nk_quant_linear_mma.h), forced with quant_rows(0) + quant_mma(U): parity
against the f64 product over the dequantised weights under the contraction policy of the rows check, the bit contract, the dispatch,
a captured replay, and nn::QuantLinear through the tape.  With g = group (32 for group 0), K = g is less than one slab, 3g a partial
slab, 2048 + g two slices (for g = 32 the second is half an int8 slab, a quarter of an int4 slab; the format refuses 2048 + 32 for group
128, whose tail slice is the shortest it accepts) and 4096 + g three; N = 1, 5, 67, 130 is less than a fragment, not a multiple of 16,
more than one block; M = 1, 9, 16, 17, 40, 129 takes every tile count, every M tail and the second pass."""
import ctypes
import functools

import numpy as np
import pytest

import quant_oracle as Q
from test_gpu_quant_linear import FORMATS, _each, device_format, fwd, reference, rows_of, same_bits, strided
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu

NS, MS, NAN = (1, 5, 67, 130), (1, 9, 16, 17, 40, 129), float("nan")


def ks(group):
    g = group or 32
    return (g, 3 * g, 2048 + g, 4096 + g)


@functools.lru_cache(maxsize=None)
def x129(K):
    return np.random.default_rng(129 + K).standard_normal((129, K)).astype(np.float32)


@pytest.fixture
def forced(dev):
    dev.quant_rows(0); dev.quant_mma(1 << 20)   # the MFMA kernel for every M
    try:
        yield dev
    finally:
        dev.quant_rows(None); dev.quant_mma(None)


def _parity_case(dev, capi, bits, group, case):
    K, N = case
    x, (_, b, s, wq, bias, _) = x129(K), reference(bits, group, K, N)
    (qw, sc), db = device_format(dev, capi, bits, group, K, N), dev.array(bias)
    ref64, cpu32 = Q.forward64(x, b, s, bias, bits, group), Q.forward32(x, b, s, bias, bits, group)

    def rows(M):
        got = fwd(dev, capi, x, qw, sc, db, M, N, K, bits, group)
        assert_contraction("quant_linear:mma:b%dg%d" % (bits, group), got, ref64[:M], K, amax=np.abs(x[:M]).max(), bmax=np.abs(wq).max(),
                           cpu32=cpu32[:M], epilogue=True)
    _each(MS, rows)


@pytest.mark.parametrize("bits,group", FORMATS)
def test_parity_against_the_f64_product(forced, bits, group):
    """every (K, N, M) runs; the failures are named together"""
    from neuronika_amd import capi
    _each([(K, N) for K in ks(group) for N in NS], _parity_case, forced, capi, bits, group)


@pytest.mark.parametrize("bits,group", FORMATS)
def test_bit_contract(forced, bits, group):
    from neuronika_amd import capi
    dev = forced
    K, N, n0, n1 = ks(group)[2], 67, 5, 23
    s, bias = reference(bits, group, K, N)[2], reference(bits, group, K, N)[4]
    x, db = x129(K), dev.array(bias)
    qw, sc = device_format(dev, capi, bits, group, K, N)
    alone = np.concatenate([fwd(dev, capi, x[m:m + 1], qw, sc, db, 1, N, K, bits, group) for m in range(129)])
    assert same_bits(fwd(dev, capi, x, qw, sc, db, 40, N, K, bits, group), alone[:40]), "a row of M = 40 differs from its M = 1 call"
    assert same_bits(fwd(dev, capi, x, qw, sc, db, 129, N, K, bits, group), alone), "a row of M = 129 (two passes) differs from its M = 1 call"
    part = fwd(dev, capi, x, qw.view_offset(n0 * K * bits // 32), sc.view_offset(n0 * s.shape[1]), db.view_offset(n0), 40, n1 - n0, K, bits, group)
    assert same_bits(part, alone[:40, n0:n1]), "weight rows %d .. %d alone differ from the full call" % (n0, n1)
    nb1 = fwd(dev, capi, x, qw, sc, None, 1, N, K, bits, group)
    assert same_bits(fwd(dev, capi, x, qw, sc, None, 17, N, K, bits, group)[:1], nb1), "without a bias, M = 17 differs from M = 1"
    # strides: x out of a wider NaN-filled matrix (16-byte and scalar loads), y into a wider NaN-filled one
    M, ldy = 17, N + 5
    for ldx, xoff in ((K + 8, 0), (K + 7, 1)):
        xo, xv = strided(dev, np.ascontiguousarray(x[:M]), ldx, xoff, fill=np.float32(NAN))
        y = dev.full((M * ldy + 4,), NAN)
        capi.quant_linear_fwd(dev, xv, ldx, qw, sc, db, y, ldy, M, N, K, bits, group)
        assert same_bits(rows_of(y.numpy(), M, N, ldy), alone[:M]), "strided call differs (ldx %d)" % ldx
        assert np.isnan(y.numpy()).sum() == y.numpy().size - M * N, "wrote outside its (M, N) block (ldx %d)" % ldx


@pytest.mark.parametrize("bits", (8, 4))
def test_dispatch_and_captured_replay(dev, bits):
    from neuronika_amd import capi
    group, N, K = 128, 1024, 1024
    bias, M = reference(bits, group, K, N)[4], capi.quant_linear_rows_rule(bits) + 1
    x, db = x129(K), dev.array(bias)
    qw, sc = device_format(dev, capi, bits, group, K, N)
    wd, X, Y = dev.zeros((N, K)), dev.array(x[:M]), dev.zeros((M, N))
    capi.quant_linear_unpack(dev, qw, sc, wd, K, N, K, bits, group)
    capi.linear_fwd(dev, X, wd, db, Y); gemm = Y.numpy()
    try:
        by_rule = fwd(dev, capi, x, qw, sc, db, M, N, K, bits, group)
        dev.quant_mma(M)
        mma = fwd(dev, capi, x, qw, sc, db, M, N, K, bits, group)
        assert same_bits(by_rule, mma if capi.quant_linear_mma_rule(bits) >= M else gemm), "the rule took another path at M = L + 1"
        dev.quant_mma(0)
        assert same_bits(fwd(dev, capi, x, qw, sc, db, M, N, K, bits, group), gemm), "knob 0 is not nk_linear_fwd over the unpacked weights"
        # a warmed call with more than one slice, captured: every replay gives the eager bits
        K2, N2 = ks(group)[2], 67
        qw2, sc2 = device_format(dev, capi, bits, group, K2, N2)
        db2, X2, y = dev.array(reference(bits, group, K2, N2)[4]), dev.array(x129(K2)[:M]), dev.full((M * N2,), NAN)
        dev.quant_mma(M)
        capi.quant_linear_fwd(dev, X2, K2, qw2, sc2, db2, y, N2, M, N2, K2, bits, group)
        eager = y.numpy()
        gh = ctypes.c_void_p(); dev.sync()
        capi.check(capi.lib.nk_graph_begin(dev.h))
        try:
            capi.quant_linear_fwd(dev, X2, K2, qw2, sc2, db2, y, N2, M, N2, K2, bits, group)
        finally:
            capi.check(capi.lib.nk_graph_end(dev.h, ctypes.byref(gh)))
        for _ in range(3):
            y.fill(NAN)
            capi.check(capi.lib.nk_graph_launch(gh)); dev.sync()
            assert same_bits(y.numpy(), eager), "a replay differs from the eager call"
        capi.check(capi.lib.nk_graph_destroy(gh))
    finally:
        dev.quant_mma(None)


@pytest.mark.parametrize("bits", (8, 4))
def test_quant_linear_through_the_tape(bits):
    import neuronika_amd
    from neuronika_amd import capi
    nk = neuronika_amd.tape; tdev = nk.Device(0)
    cdev, lin = capi.Device(handle=tdev.raw()), nk.nn.Linear(tdev, 1024, 1024, 11)
    ql = nk.nn.QuantLinear(lin, bits, 128)
    dq, bias, x = ql.dequantize().data(), lin.bias.data(), x129(1024)[:12]
    cdev.quant_rows(0); cdev.quant_mma(128)
    try:
        y = ql.forward(nk.from_ndarray(tdev, np.ascontiguousarray(x)))
        y.forward(); got = y.data()
    finally:
        cdev.quant_rows(None); cdev.quant_mma(None)
    ref64 = x.astype(np.float64) @ dq.astype(np.float64).T + bias.astype(np.float64)
    assert_contraction("quant_linear:mma:b%dg128" % bits, got, ref64, 1024, amax=np.abs(x).max(), bmax=np.abs(dq).max(),
                       cpu32=(x @ dq.T + bias).astype(np.float32), epilogue=True)
