"""The over-window route of the aligned 128 x 128 GEMM.  The four kernels sgemm_kernel<TA, TB, true, 2, 2, 1, EPX> (NN, NT, TN) hold the
buffer-addressed block program alone, so a launch whose operand windows pass the limit (NK_TUNE_GEMM_WINDOW lowers it for small
matrices) runs the GUARDED instantiation of the same layout, tile and epilogue, sgemm_kernel<TA, TB, false, 2, 2, 1, EPX>: its loader's
16-byte `interior` path, the one-k-tile look-ahead loop, the same MFMA feeding order.  Every launch form that can get there -
split-K, several tiles per block, a strided two-level batch, beta = 1 on views - must give the bits of the buffer-addressed launch
(and, where the launch is unsplit, of oracle/device_order_sgemm.c), and the counter nk_gemm_buffer_launches says which route ran.
k-pair blocks are decided first and keep their aligned pointer kernel under any window."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYOUTS = [pytest.param(0, 0, id="nn"), pytest.param(0, 1, id="nt"), pytest.param(1, 0, id="tn")]
LOOKAHEAD_FROM_1 = "2,2,1,1,8,1"   # NK_TUNE_GEMM_FORCE: 128 x 128 tiles, unsplit, one tile per block, look-ahead loop from one k-tile on
PLAIN = "2,2,1"                    # ... with the look-ahead threshold of the rules (NN 32, NT / TN 48 k-tiles)
LOW = 1 << 20                      # window limit in bytes that every operand of cases A1 - A4 passes


def capi():
    from neuronika_amd import capi as c
    return c


def rnd(seed, shape):
    return np.asarray(np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(2) - np.float32(1), dtype=np.float32)


def model(opa, opb):
    from oracle.build_c import sgemm_device_order
    return sgemm_device_order(opa, opb, 0)


def place(dev, mat, ld, first):
    """`mat` (rows x cols) as a view: leading dimension `ld`, first element `first` floats into an allocation that its last element
    ends; the rest of the allocation holds NaN, so a load from outside the view shows"""
    rows, cols = mat.shape
    assert ld >= cols
    host = np.full(first + (rows - 1) * ld + cols, np.nan, np.float32)
    host[first + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]] = mat
    return dev.array(host).view_offset(first)


def operands(seed, ta, tb, M, N, K):
    """stored A, stored B, op(A) (M x K), op(B) (K x N)"""
    a = rnd(seed, (K, M) if ta else (M, K))
    b = rnd(seed + 1, (N, K) if tb else (K, N))
    return a, b, np.ascontiguousarray(a.T if ta else a), np.ascontiguousarray(b.T if tb else b)


def window_bytes(kc, ld, K):
    """the window a 128-row tile spans in an operand (gemm_plan's rule)"""
    return (127 * ld + K) * 4 if kc else (K * ld + 128) * 4


def both_windows(dev, run, low=LOW):
    """run() -> output array, once under the low window limit and once under the rule: ({window: output}, {window: buffer launches})"""
    outs, took = {}, {}
    for window in (low, None):
        dev.gemm_window(window)
        before = dev.gemm_buffer_launches()
        outs[window] = run()
        took[window] = dev.gemm_buffer_launches() - before
    return outs, took


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_split_k(dev, ta, tb):
    """A1: split-K 4 of 256 x 256 x 2048, operands with ld = 4096: slabs of 16 k-tiles each, then the second pass.  Each slab is one
    chain in the device order, the second pass adds them in split order."""
    c = capi()
    M = N = 256
    K, ld = 2048, 4096
    a, b, opa, opb = operands(700, ta, tb, M, N, K)
    assert min(window_bytes(not ta, ld, K), window_bytes(bool(tb), ld, K)) > LOW
    try:
        dev.gemm_kpair(0)
        dev.gemm_force("2,2,4")
        A, B = place(dev, a, ld, 0), place(dev, b, ld, 0)

        def run():
            Cd = dev.full((M, N), np.nan)
            c.sgemm(dev, ta, tb, M, N, K, 1.0, A, ld, B, ld, 0.0, Cd, N)
            return Cd.numpy()
        outs, took = both_windows(dev, run)
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None); dev.gemm_window(None)
    assert took == {LOW: 0, None: 1}, took
    assert np.array_equal(outs[LOW], outs[None])
    want = np.zeros((M, N), np.float32)
    for s in range(4):
        want = want + model(opa[:, 512 * s:512 * (s + 1)], opb[512 * s:512 * (s + 1)])
    assert np.array_equal(outs[None], want)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_several_tiles_per_block(dev, ta, tb):
    """A2: two tiles per block (256 x 256 x 96: three k-tiles each, the next tile's first loads issued in front of the last MFMAs)"""
    c = capi()
    M = N = 256
    K, ld = 96, 4096
    a, b, opa, opb = operands(710, ta, tb, M, N, K)
    assert min(window_bytes(not ta, ld, K), window_bytes(bool(tb), ld, K)) > LOW
    try:
        dev.gemm_kpair(0)
        dev.gemm_force("2,2,1,2")
        A, B = place(dev, a, ld, 0), place(dev, b, ld, 0)

        def run():
            Cd = dev.full((M, N), np.nan)
            c.sgemm(dev, ta, tb, M, N, K, 1.0, A, ld, B, ld, 0.0, Cd, N)
            return Cd.numpy()
        outs, took = both_windows(dev, run)
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None); dev.gemm_window(None)
    assert took == {LOW: 0, None: 1}, took
    assert np.array_equal(outs[LOW], outs[None])
    assert np.array_equal(outs[None], model(opa, opb))


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_two_level_batch_with_strides(dev, ta, tb):
    """A3: 2 x 2 problems of 128 x 128 x 160 in one launch, ld = 4096 and strides that are not the matrices' sizes.  The default run is
    the buffer-addressed look-ahead loop (forced from one k-tile), the low-window run the guarded kernel's one-k-tile loop."""
    c = capi()
    M, N, K, bo, bi, ld = 128, 128, 32 * 5, 2, 2, 4096
    assert min(window_bytes(not ta, ld, K), window_bytes(bool(tb), ld, K)) > LOW
    ra, rb = (K if ta else M), (N if tb else K)                  # stored rows
    sAi, sAo = ra * ld + 12, 2 * (ra * ld + 12) + 16
    sBi, sBo = rb * ld + 20, 2 * (rb * ld + 20) + 4
    sCi, sCo = M * N, 2 * M * N
    ha = np.full(bo * sAo, np.nan, np.float32)
    hb = np.full(bo * sBo, np.nan, np.float32)
    want = np.empty((bo, bi, M, N), np.float32)
    for o in range(bo):
        for i in range(bi):
            a, b, opa, opb = operands(720 + 10 * o + i, ta, tb, M, N, K)
            ha[o * sAo + i * sAi + np.arange(ra)[:, None] * ld + np.arange(a.shape[1])[None, :]] = a
            hb[o * sBo + i * sBi + np.arange(rb)[:, None] * ld + np.arange(b.shape[1])[None, :]] = b
            want[o, i] = model(opa, opb)
    try:
        dev.gemm_kpair(0)
        dev.gemm_force(LOOKAHEAD_FROM_1)
        A, B = dev.array(ha), dev.array(hb)

        def run():
            Cd = dev.full((bo, bi, M, N), np.nan)
            c.sgemm_batched(dev, ta, tb, M, N, K, 1.0, A, ld, sAo, sAi, B, ld, sBo, sBi, 0.0, Cd, N, sCo, sCi, bo, bi)
            return Cd.numpy()
        outs, took = both_windows(dev, run)
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None); dev.gemm_window(None)
    assert took == {LOW: 0, None: 1}, took
    assert np.array_equal(outs[LOW], outs[None])
    assert np.array_equal(outs[None], want)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_kpair_blocks_keep_their_kernel(dev, ta, tb):
    """A4: k-pair blocks (512 threads) are chosen before the window is looked at and hold the pointer loader: the same kernel, the same
    bits and no buffer-addressed launch under either limit"""
    c = capi()
    M = N = 256
    K, ld = 2048, 4096
    a, b, _, _ = operands(730, ta, tb, M, N, K)
    try:
        dev.gemm_kpair(1)
        dev.gemm_force(PLAIN)
        A, B = place(dev, a, ld, 0), place(dev, b, ld, 0)

        def run():
            Cd = dev.full((M, N), np.nan)
            c.sgemm(dev, ta, tb, M, N, K, 1.0, A, ld, B, ld, 0.0, Cd, N)
            return Cd.numpy()
        outs, took = both_windows(dev, run)
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None); dev.gemm_window(None)
    assert took == {LOW: 0, None: 0}, took
    assert not np.isnan(outs[None]).any()
    assert np.array_equal(outs[LOW], outs[None])


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_views_offset_base_and_beta(dev, ta, tb):
    """B: beta = 1 on top of an old C; A, B and C are views 16 bytes into their allocations with leading dimensions above the extents
    (different for each).  The window limit of 64 KiB is below every operand's window here.  Reductions of 49, 5 and 3 k-tiles: on
    the default route both k-loops, on the over-window route the one-k-tile loop with two, one and no trips past the first pair."""
    c = capi()
    M, N, first, low = 256, 128, 4, 1 << 16
    try:
        dev.gemm_kpair(0)
        for force, K in ((PLAIN, 32 * 49), (LOOKAHEAD_FROM_1, 32 * 5), (PLAIN, 32 * 3)):
            dev.gemm_force(force)
            a, b, opa, opb = operands(740 + K, ta, tb, M, N, K)
            c0 = rnd(743, (M, N))
            lda, ldb, ldc = a.shape[1] + 68, b.shape[1] + 132, N + 36
            assert min(window_bytes(not ta, lda, K), window_bytes(bool(tb), ldb, K)) > low
            A, B = place(dev, a, lda, first), place(dev, b, ldb, first)

            def run():
                Cd = place(dev, c0, ldc, first)
                c.sgemm(dev, ta, tb, M, N, K, 1.0, A, lda, B, ldb, 1.0, Cd, ldc)
                return Cd.numpy()[(np.arange(M)[:, None] * ldc + np.arange(N)[None, :])]
            outs, took = both_windows(dev, run, low)
            assert took == {low: 0, None: 1}, (force, K, took)
            assert np.array_equal(outs[low], outs[None]), (force, K)
            assert np.array_equal(outs[None], c0 + model(opa, opb)), (force, K)   # fmaf(1, old, acc) == fl(old + acc)
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None); dev.gemm_window(None)
