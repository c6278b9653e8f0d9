"""nk_quant_linear_* through the C ABI (`capi`) against tests/quant_oracle.py.  pack and unpack agree with the oracle BIT FOR BIT;
the rows kernels pass the project's contraction policy against the f64 product over the dequantised weights and keep their bit
contract (a row's bits do not depend on M, N, the pass, the row range the call is pointed at or the strides); the many-row path is
nk_linear_fwd over the unpacked weights bit for bit; refused calls write nothing.

With g = group (32 for group 0) the K walk is g (one partial wave, some lanes without a load), 3g, 1024 + g (one full wave stride of
int8 plus a tail) and 4096 + g (several strides); the N walk is 1, 5, 67, 130 (less than a block of 16 weight rows, not a multiple of
a wave's 4, more than one block).  ONE test id, many cases: the test at the end of the file runs every `check_*` of this file and
then those of tests/test_gpu_tape_quant.py (the same layers through the tape), each check walks its cases, and the failures are named
together."""
import functools

import numpy as np
import pytest

import quant_oracle as Q
from tolerance import assert_contraction

pytestmark = pytest.mark.gpu

BITS, GROUPS, NS, MS = (8, 4), (32, 128, 0), (1, 5, 67, 130), (1, 2, 3, 5, 8)
GUARD = np.float32(-12345.5)


def ks(group):
    g = group or 32
    return (g, 3 * g, 1024 + g, 4096 + g)


FORMATS = [(bits, group) for bits in BITS for group in GROUPS]
CASES = [(bits, group, K, N) for bits, group in FORMATS for K in ks(group) for N in NS]


def _each(cases, check, *args):
    failed = []
    for case in cases:
        try:
            check(*args, case)
        except AssertionError as e:
            failed.append("%r: %s" % (case, str(e)[:300]))
    assert not failed, "\n".join(failed)


@functools.lru_cache(maxsize=None)
def weights(N, K, group):
    """seeded normal data with, in the first (row, group) slots, the tie row, an all-zero group and a group whose absmax is a negative
    element (as far as the shape has room for them)"""
    g = Q.group_len(K, group)
    W = np.random.default_rng(1000 * N + K).standard_normal((N, K)).astype(np.float32)
    W[0, :g] = Q.tie_row(g)
    slots = [(n, j) for n in range(N) for j in range(K // g)][1:3]
    if len(slots) > 0:
        n, j = slots[0]
        W[n, j * g:(j + 1) * g] = 0
    if len(slots) > 1:
        n, j = slots[1]
        W[n, j * g + 3] = -7.5
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def reference(bits, group, K, N):
    """(W, bytes, scales, w^, bias, x (8, K)): computed once, shared, never written"""
    W = weights(N, K, group)
    b, s = Q.pack(W, bits, group)
    rng = np.random.default_rng(7 * N + K + bits)
    out = (W, b, s, Q.unpack(b, s, bits, group, K), rng.standard_normal(N).astype(np.float32), rng.standard_normal((8, K)).astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


def strided(dev, a, ld, off=0, fill=GUARD):
    """a (R, C) host matrix as rows of stride ld on the device, `off` floats into the allocation -> (owner, view)"""
    R, C = a.shape
    host = np.full(off + R * ld + 4, fill, np.float32)
    for r in range(R):
        host[off + r * ld: off + r * ld + C] = a[r]
    buf = dev.array(host)
    return buf, buf.view_offset(off)


def rows_of(buf_np, R, C, ld, off=0):
    return np.stack([buf_np[off + r * ld: off + r * ld + C] for r in range(R)])


def device_format(dev, capi, bits, group, K, N):
    """the oracle's packed weight and scales uploaded -> (qw, scales)"""
    _, b, s, _, _, _ = reference(bits, group, K, N)
    assert b.size == 4 * capi.quant_linear_words(N, K, bits) and s.size == capi.quant_linear_scales(N, K, group)
    return dev.array(np.ascontiguousarray(b).view(np.float32).ravel()), dev.array(s.ravel())


def fwd(dev, capi, x, qw, sc, bias, M, N, K, bits, group, ldx=None, ldy=None, xoff=0):
    """y (M, N) of one call; x host (M, K), uploaded at stride ldx; y lands in a NaN-filled (M, ldy) buffer whose other columns must stay NaN"""
    ldx, ldy = ldx or K, ldy or N
    xo, xv = strided(dev, np.ascontiguousarray(x[:M]), ldx, xoff)
    y = dev.full((M * ldy + 4,), float("nan"))
    capi.quant_linear_fwd(dev, xv, ldx, qw, sc, bias, y, ldy, M, N, K, bits, group)
    out = y.numpy()
    got = rows_of(out, M, N, ldy)
    rest = np.ones(out.size, bool)
    for m in range(M):
        rest[m * ldy: m * ldy + N] = False
    assert np.isnan(out[rest]).all(), "wrote outside its (M, N) block"
    return got


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. pack, 2. unpack -----------------------------------------------------------------------------------------------------------
def _pack_case(dev, capi, case):
    bits, group, K, N = case
    W, b, s, _, _, _ = reference(bits, group, K, N)
    words = capi.quant_linear_words(N, K, bits)
    for ldw, off in ((K, 0), (K + 3, 1)):   # 16-byte loads; scalar loads out of a wider, unaligned matrix
        wo, wv = strided(dev, W, ldw, off)
        qw, sc = dev.full((words + 4,), float(GUARD)), dev.full((s.size + 4,), float(GUARD))
        capi.quant_linear_pack(dev, wv, ldw, qw, sc, N, K, bits, group)
        gq, gs = qw.numpy(), sc.numpy()
        assert (gq[words:] == GUARD).all() and (gs[s.size:] == GUARD).all(), "wrote past its output"
        assert np.array_equal(gq[:words].view(np.uint8).reshape(b.shape), b), "packed bytes differ (ldw %d)" % ldw
        assert same_bits(gs[:s.size].reshape(s.shape), s), "scales differ (ldw %d)" % ldw


def check_pack_matches_the_oracle_bit_for_bit(dev):
    from neuronika_amd import capi
    _each(CASES, _pack_case, dev, capi)


def _unpack_case(dev, capi, case):
    bits, group, K, N = case
    _, _, _, wq, _, _ = reference(bits, group, K, N)
    qw, sc = device_format(dev, capi, bits, group, K, N)
    for ldw, off in ((K, 0), (K + 4, 0), (K + 5, 3)):
        out = dev.full((off + N * ldw + 4,), float(GUARD))
        capi.quant_linear_unpack(dev, qw, sc, out.view_offset(off), ldw, N, K, bits, group)
        got = out.numpy()
        assert same_bits(rows_of(got, N, K, ldw, off), wq), "w^ differs (ldw %d)" % ldw
        rest = np.ones(got.size, bool)
        for n in range(N):
            rest[off + n * ldw: off + n * ldw + K] = False
        assert (got[rest] == GUARD).all(), "wrote beyond a row's K columns (ldw %d)" % ldw


def check_unpack_matches_the_oracle_bit_for_bit(dev):
    from neuronika_amd import capi
    _each(CASES, _unpack_case, dev, capi)


# ---- 3. rows path parity ------------------------------------------------------------------------------------------------------------
def _rows_case(dev, capi, case):
    bits, group, K, N = case
    _, b, s, wq, bias, x = reference(bits, group, K, N)
    qw, sc = device_format(dev, capi, bits, group, K, N)
    db = dev.array(bias)
    ref64, cpu32 = Q.forward64(x, b, s, bias, bits, group), Q.forward32(x, b, s, bias, bits, group)
    for M in MS:
        got = fwd(dev, capi, x, qw, sc, db, M, N, K, bits, group)
        assert_contraction("quant_linear:rows:b%dg%d" % (bits, group), got, ref64[:M], K, amax=np.abs(x[:M]).max(), bmax=np.abs(wq).max(),
                           cpu32=cpu32[:M], epilogue=True)


def check_rows_path_against_the_f64_product(dev):
    from neuronika_amd import capi
    dev.quant_rows(8)   # the rows kernels whatever the measured rule says
    try:
        _each(CASES, _rows_case, dev, capi)
    finally:
        dev.quant_rows(None)


# ---- 4. bit contract ----------------------------------------------------------------------------------------------------------------
def _contract_case(dev, capi, case):
    bits, group = case
    K, N = 1024 + (group or 32), 67
    _, b, s, _, bias, x8 = reference(bits, group, K, N)
    x = np.concatenate([x8, x8[::-1] * np.float32(0.5), x8[:3] + np.float32(1)])   # 19 rows
    qw, sc = device_format(dev, capi, bits, group, K, N)
    db = dev.array(bias)
    dev.quant_rows(24)
    alone = np.concatenate([fwd(dev, capi, x[m:m + 1], qw, sc, db, 1, N, K, bits, group) for m in range(19)])
    assert same_bits(fwd(dev, capi, x, qw, sc, db, 8, N, K, bits, group), alone[:8]), "a row of M = 8 differs from its M = 1 call"
    assert same_bits(fwd(dev, capi, x, qw, sc, db, 19, N, K, bits, group), alone), "a row of M = 19 (three passes) differs from its M = 1 call"
    # the row range n0 .. n1 of the weights
    n0, n1 = 5, 23
    part = fwd(dev, capi, x, qw.view_offset(n0 * K * bits // 32), sc.view_offset(n0 * s.shape[1]), db.view_offset(n0), 8, n1 - n0, K, bits, group)
    assert same_bits(part, alone[:8, n0:n1]), "rows %d .. %d alone differ from the full call" % (n0, n1)
    # no bias: the sum alone, whatever the other arguments
    nb1 = fwd(dev, capi, x, qw, sc, None, 1, N, K, bits, group)
    assert same_bits(fwd(dev, capi, x, qw, sc, None, 5, N, K, bits, group)[:1], nb1)
    # strides: x out of a wider matrix (16-byte and scalar loads), y into a wider NaN-filled one
    for ldx, xoff in ((K + 8, 0), (K + 7, 1)):
        assert same_bits(fwd(dev, capi, x, qw, sc, db, 5, N, K, bits, group, ldx=ldx, ldy=N + 5, xoff=xoff), alone[:5]), "strided call differs (ldx %d)" % ldx


def check_rows_path_bit_contract(dev):
    from neuronika_amd import capi
    try:
        _each(FORMATS, _contract_case, dev, capi)
    finally:
        dev.quant_rows(None)


# ---- 5. many-row path ---------------------------------------------------------------------------------------------------------------
def _many_case(dev, capi, case):
    bits, group = case
    K, N = 1024 + (group or 32), 67
    _, b, s, wq, bias, x8 = reference(bits, group, K, N)
    L = capi.quant_linear_rows_rule(bits)
    assert L >= 1
    M = L + 1
    x = np.random.default_rng(5).standard_normal((M, K)).astype(np.float32)
    qw, sc = device_format(dev, capi, bits, group, K, N)
    db = dev.array(bias)
    wd = dev.zeros((N, K))
    capi.quant_linear_unpack(dev, qw, sc, wd, K, N, K, bits, group)

    def gemm(xs):
        X, Y = dev.array(xs), dev.zeros((xs.shape[0], N))
        capi.linear_fwd(dev, X, wd, db, Y)
        return Y.numpy()

    by_rule_rows = fwd(dev, capi, x, qw, sc, db, 3, N, K, bits, group)
    assert same_bits(fwd(dev, capi, x, qw, sc, db, M, N, K, bits, group), gemm(x)), "M = L + 1 is not nk_linear_fwd over the unpacked weights"
    dev.quant_rows(0)
    assert same_bits(fwd(dev, capi, x, qw, sc, db, 3, N, K, bits, group), gemm(x[:3])), "knob 0, M = 3 is not nk_linear_fwd over the unpacked weights"
    assert_contraction("quant_linear:many:b%dg%d" % (bits, group), gemm(x[:3]), Q.forward64(x[:3], b, s, bias, bits, group), K,
                       amax=np.abs(x[:3]).max(), bmax=np.abs(wq).max(), cpu32=Q.forward32(x[:3], b, s, bias, bits, group), epilogue=True)
    dev.quant_rows(8)
    forced_rows = fwd(dev, capi, x, qw, sc, db, 3, N, K, bits, group)
    dev.quant_rows(-1)
    assert same_bits(fwd(dev, capi, x, qw, sc, db, 3, N, K, bits, group), by_rule_rows), "knob -1 did not restore the rule"
    if L >= 3:
        assert same_bits(by_rule_rows, forced_rows)
    assert same_bits(fwd(dev, capi, x, qw, sc, db, M, N, K, bits, group), gemm(x)), "knob -1 did not restore the rule at M = L + 1"


def check_many_row_path_is_linear_fwd_over_the_unpacked_weights(dev):
    from neuronika_amd import capi
    try:
        _each(FORMATS, _many_case, dev, capi)
    finally:
        dev.quant_rows(None)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def check_refused_calls_write_nothing(dev):
    from neuronika_amd import capi
    N, K, M = 5, 96, 2
    x, sc, bias = dev.full((M * K,), 1.0), dev.full((N * 3,), 1.0), dev.full((N,), 1.0)
    qw = dev.full((N * K // 4 + 4,), 0.0)
    y = dev.full((M * N + 4,), float(GUARD))
    W = dev.full((N * K,), float(GUARD))

    def refused(fn, *args):
        try:
            fn(dev, *args)
        except capi.NeuronikaHipError as e:
            assert e.code == 1, e
        else:
            raise AssertionError("accepted: %r" % (args[-5:],))
        assert (y.numpy() == GUARD).all() and (W.numpy() == GUARD).all(), "a refused call wrote"

    f = capi.quant_linear_fwd
    refused(f, x, 48, qw, sc, bias, y, N, M, N, 48, 8, 0)      # K = 48
    refused(f, x, K, qw, sc, bias, y, N, M, N, K, 8, 64)       # group 64 does not divide K = 96
    refused(f, x, K, qw, sc, bias, y, N, M, N, K, 3, 32)       # bits = 3
    refused(f, x, K, qw, sc, bias, y, N, M, N, K, 8, 16)       # group = 16
    refused(f, x, K, None, sc, bias, y, N, M, N, K, 8, 32)     # null qw
    refused(f, x, K, qw, sc, bias, y, N - 1, M, N, K, 8, 32)   # ldy < N
    refused(f, x, K - 1, qw, sc, bias, y, N, M, N, K, 8, 32)   # ldx < K
    refused(f, x, K, qw.view_offset(1), sc, bias, y, N, M, N, K, 8, 32)   # qw misaligned by 4 bytes
    refused(f, x, K, qw, sc, bias, y, N, -1, N, K, 8, 32)      # M < 0
    refused(f, x, K, qw, sc, bias, y, N, M, 0, K, 8, 32)       # N = 0
    u = capi.quant_linear_unpack
    refused(u, qw, sc, W, K - 1, N, K, 8, 32)                  # ldw < K
    refused(u, qw.view_offset(1), sc, W, K, N, K, 4, 32)
    refused(u, qw, sc, W, 48, N, 48, 8, 0)
    refused(u, qw, None, W, K, N, K, 8, 32)
    capi.quant_linear_fwd(dev, x, K, qw, sc, bias, y, N, 0, N, K, 8, 32)   # M = 0: an empty success
    assert (y.numpy() == GUARD).all()
    # pack refuses the same way and leaves qw and the scales alone
    qg, sg = dev.full((N * K // 4 + 4,), float(GUARD)), dev.full((N * 3,), float(GUARD))
    for args in ((x, 48, qg, sg, 2, 48, 8, 0), (x, K, qg, sg, 2, K, 5, 0), (x, K, qg, sg, 2, K, 4, 64), (x, K - 1, qg, sg, 2, K, 4, 32),
                 (x, K, qg.view_offset(1), sg, 2, K, 4, 32), (None, K, qg, sg, 2, K, 4, 32)):
        try:
            capi.quant_linear_pack(dev, *args)
        except capi.NeuronikaHipError as e:
            assert e.code == 1, e
        else:
            raise AssertionError("pack accepted %r" % (args[-5:],))
        assert (qg.numpy() == GUARD).all() and (sg.numpy() == GUARD).all()


# ---- the one test id ---------------------------------------------------------------------------------------------------------------
CHECKS = (check_pack_matches_the_oracle_bit_for_bit, check_unpack_matches_the_oracle_bit_for_bit, check_rows_path_against_the_f64_product,
          check_rows_path_bit_contract, check_many_row_path_is_linear_fwd_over_the_unpacked_weights, check_refused_calls_write_nothing)


def test_quant_linear_through_the_c_abi_and_the_tape(dev):
    """every check of this file, then every check of tests/test_gpu_tape_quant.py; a failed assertion does not hide the next check (any
    other exception ends the test at once)"""
    import test_gpu_tape_quant as T
    failed = []
    for name, check in [(f.__name__, lambda f=f: f(dev)) for f in CHECKS] + T.checks():
        try:
            check()
        except AssertionError as e:
            failed.append("%s: %s" % (name, str(e)[:800]))
    assert not failed, "\n".join(failed)
