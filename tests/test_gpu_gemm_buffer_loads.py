"""The buffer-addressed tile loads of the aligned 128 x 128 GEMM (sgemm_kernel's `p.buf` path, BufTileLoader: nk_gemm.hip, nk_mma.h) against
the device-order model of oracle/device_order_sgemm.c, BIT FOR BIT - the reference and the comparison of
tests/test_gpu_parity.py::test_sgemm_is_the_device_order_model_bit_for_bit.  A descriptor per operand based at the block's tile
origin, 32-bit byte offsets per lane, the k advance in a scalar: what can go wrong is an origin, an offset, the advance or
num_records, so the cases move each of them - every tail length of the look-ahead loop and the one-k-tile loop, operands that are
views (leading dimension above the extent, a base 16 / 4096 bytes into an allocation), beta = 1, the two fused epilogues, a two-level
batch with strides, the fallback to the 64-bit pointer kernels above the window limit, and an operand that ends where its
allocation ends.  Outputs are 128 x 128 and 256 x 128 (one and two blocks); every launch is checked to have taken the kernel the
case is about (nk_gemm_buffer_launches)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LAYOUTS = [pytest.param(0, 0, id="nn"), pytest.param(0, 1, id="nt"), pytest.param(1, 0, id="tn")]
LOOKAHEAD_FROM_1 = "2,2,1,1,8,1"   # NK_TUNE_GEMM_FORCE: 128 x 128 tiles, unsplit, one tile per block, look-ahead loop from one k-tile on
PLAIN = "2,2,1"                    # ... with the look-ahead threshold of the rules (NN 32, NT / TN 48 k-tiles)


def capi():
    from neuronika_amd import capi as c
    return c


def rnd(seed, shape):
    return np.asarray(np.random.default_rng(seed).random(shape, dtype=np.float32) * np.float32(2) - np.float32(1), dtype=np.float32)


def model(opa, opb):
    from oracle.build_c import sgemm_device_order
    return sgemm_device_order(opa, opb, 0)


def place(dev, mat, ld, first, total=None):
    """`mat` (rows x cols) as a view: leading dimension `ld`, first element `first` floats into an allocation of `total` floats
    (default: the view's last element ends it); the rest of the allocation holds NaN, so a load from outside the view shows"""
    rows, cols = mat.shape
    need = first + (rows - 1) * ld + cols
    total = need if total is None else total
    assert total >= need and ld >= cols
    host = np.full(total, np.nan, np.float32)
    idx = first + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
    host[idx] = mat
    return dev.array(host).view_offset(first)


def operands(seed, ta, tb, M, N, K):
    """stored A, stored B, op(A) (M x K), op(B) (K x N)"""
    a = rnd(seed, (K, M) if ta else (M, K))
    b = rnd(seed + 1, (N, K) if tb else (K, N))
    return a, b, np.ascontiguousarray(a.T if ta else a), np.ascontiguousarray(b.T if tb else b)


def launched(dev, fn):
    """runs fn(); how many of its GEMM launches took the buffer-addressed kernels"""
    before = dev.gemm_buffer_launches()
    fn()
    return dev.gemm_buffer_launches() - before


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_reduction_lengths(dev, ta, tb):
    """K = 32 nt: nt = 48, 49 leave the look-ahead loop with 2 and 3 tiles; with the threshold lowered nt = 1 .. 5 are its every
    prologue / tail combination; nt = 3 under the rules' threshold is the one-k-tile loop with the same loader"""
    c = capi()
    M, N = 256, 128
    try:
        dev.gemm_kpair(0)                                            # 256-thread blocks: two-block grids would take k-pair blocks by rule
        for force, nts in ((PLAIN, (48, 49, 3)), (LOOKAHEAD_FROM_1, (1, 2, 3, 4, 5))):
            dev.gemm_force(force)
            for nt in nts:
                K = 32 * nt
                a, b, opa, opb = operands(100 + nt, ta, tb, M, N, K)
                A, B, Cd = dev.array(a), dev.array(b), dev.full((M, N), np.nan)
                n = launched(dev, lambda: c.sgemm(dev, ta, tb, M, N, K, 1.0, A, a.shape[1], B, b.shape[1], 0.0, Cd, N))
                assert n == 1, (force, nt, "not the buffer-addressed kernel")
                assert np.array_equal(Cd.numpy(), model(opa, opb)), (force, nt)
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None)


@pytest.mark.parametrize("first", [4, 1024], ids=["base16B", "base4096B"])
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_views_offset_bases_and_beta(dev, ta, tb, first):
    """sub-matrix views: leading dimensions above the extents (different for A, B and C), bases 16 / 4096 bytes into their
    allocations, beta = 1 on top of an old C; both k-loops"""
    c = capi()
    M, N = 256, 128
    try:
        dev.gemm_kpair(0)                                            # 256-thread blocks: two-block grids would take k-pair blocks by rule
        for force, K in ((PLAIN, 32 * 49), (LOOKAHEAD_FROM_1, 32 * 5), (PLAIN, 32 * 3)):
            dev.gemm_force(force)
            a, b, opa, opb = operands(200 + K + first, ta, tb, M, N, K)
            c0 = rnd(203, (M, N))
            lda, ldb, ldc = a.shape[1] + 68, b.shape[1] + 132, N + 36
            A, B, Cd = place(dev, a, lda, first, first + a.shape[0] * lda + 64), place(dev, b, ldb, first), place(dev, c0, ldc, first)
            n = launched(dev, lambda: c.sgemm(dev, ta, tb, M, N, K, 1.0, A, lda, B, ldb, 1.0, Cd, ldc))
            assert n == 1, (force, K)
            got = Cd.numpy()[(np.arange(M)[:, None] * ldc + np.arange(N)[None, :])]
            assert np.array_equal(got, c0 + model(opa, opb)), (force, K)   # fmaf(1, old, acc) == fl(old + acc)
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None)


@pytest.mark.parametrize("form", ["bias_relu", "mask"])
def test_fused_epilogues(dev, form):
    """the two EPX instantiations: nk_linear_relu_fwd (NT: max(acc + bias, 0)) and nk_linear_bwd_input_relu (NN: beta C + (acc where
    the mask operand is positive, 0 * acc elsewhere)); both k-loops"""
    c = capi()
    n_, m_ = 256, 128
    try:
        dev.gemm_kpair(0)                                            # 256-thread blocks: two-block grids would take k-pair blocks by rule
        for force, K in ((PLAIN, 32 * 48), (LOOKAHEAD_FROM_1, 32 * 4)):
            dev.gemm_force(force)
            if form == "bias_relu":                                  # Y (n, o) = max(X (n, K) . W (o, K)^T + b, 0)
                x, w, bias = rnd(300 + K, (n_, K)), rnd(301 + K, (m_, K)), rnd(302, (m_,))
                X, W, Bv, Y = dev.array(x), dev.array(w), dev.array(bias), dev.full((n_, m_), np.nan)
                n = launched(dev, lambda: c.linear_relu_fwd(dev, X, W, Bv, Y))
                want = np.maximum(model(x, np.ascontiguousarray(w.T)) + bias[None, :], np.float32(0))
                got = Y.numpy()
            else:                                                    # dZ (n, m) += (G (n, K) . W (K, m)) where X > 0
                g, w, x, z0 = rnd(310 + K, (n_, K)), rnd(311 + K, (K, m_)), rnd(312, (n_, m_)), rnd(313, (n_, m_))
                G, W, X, Z = dev.array(g), dev.array(w), dev.array(x), dev.array(z0)
                n = launched(dev, lambda: c.linear_bwd_input_relu(dev, Z, G, W, X))
                acc = model(g, w)
                want = z0 + np.where(x > 0, acc, np.float32(0) * acc)
                got = Z.numpy()
            assert n == 1, (form, force)
            assert np.array_equal(got, want), (form, force)
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_two_level_batch_with_strides(dev, ta, tb):
    """2 x 2 problems of one launch, outer / inner strides that are not the matrices' sizes: every block bases its descriptors at
    ITS batch element's tile origin"""
    c = capi()
    M, N, K, bo, bi = 128, 128, 32 * 5, 2, 2
    try:
        dev.gemm_kpair(0)                                            # 256-thread blocks: two-block grids would take k-pair blocks by rule
        dev.gemm_force(LOOKAHEAD_FROM_1)
        ra, rb = (K if ta else M), (N if tb else K)                  # stored rows
        lda, ldb = (M if ta else K) + 4, (K if tb else N) + 8
        sAi, sAo = ra * lda + 12, 2 * (ra * lda + 12) + 16
        sBi, sBo = rb * ldb + 20, 2 * (rb * ldb + 20) + 4
        sCi, sCo = M * N, 2 * M * N
        ha = np.full(bo * sAo, np.nan, np.float32)
        hb = np.full(bo * sBo, np.nan, np.float32)
        want = np.empty((bo, bi, M, N), np.float32)
        for o in range(bo):
            for i in range(bi):
                a, b, opa, opb = operands(400 + 10 * o + i, ta, tb, M, N, K)
                ha[o * sAo + i * sAi + np.arange(ra)[:, None] * lda + np.arange(a.shape[1])[None, :]] = a
                hb[o * sBo + i * sBi + np.arange(rb)[:, None] * ldb + np.arange(b.shape[1])[None, :]] = b
                want[o, i] = model(opa, opb)
        A, B, Cd = dev.array(ha), dev.array(hb), dev.full((bo, bi, M, N), np.nan)
        n = launched(dev, lambda: c.sgemm_batched(dev, ta, tb, M, N, K, 1.0, A, lda, sAo, sAi, B, ldb, sBo, sBi, 0.0, Cd, N, sCo, sCi, bo, bi))
        assert n == 1
        assert np.array_equal(Cd.numpy(), want)
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None)


@pytest.mark.parametrize("case", ["nn", "nt", "tn", "nn_mask"])
def test_window_limit_takes_the_pointer_kernels(dev, case):
    """NK_TUNE_GEMM_WINDOW = 1 MiB: a 256 x 256 x 2048 product whose operands have leading dimension 4096 (windows of 2 - 32 MiB) must
    take the 64-bit pointer kernels - the four instantiations sgemm_kernel<.., true, 2, 2, 1, ..> of NN, NT, TN and masked NN -
    and give the bits the buffer-addressed launch gives with the knob at its default (and the model's)"""
    c = capi()
    M = N = 256
    K, ld = 2048, 4096
    ta, tb = {"nn": (0, 0), "nt": (0, 1), "tn": (1, 0), "nn_mask": (0, 0)}[case]
    outs, took = {}, {}
    try:
        dev.gemm_kpair(0)                                            # 256-thread blocks: two-block grids would take k-pair blocks by rule
        dev.gemm_force(PLAIN)
        if case == "nn_mask":                                        # the entry point fixes ld = extent: (127 * 2048 + 2048) * 4 > 1 MiB
            g, w, x = rnd(500, (M, K)), rnd(501, (K, N)), rnd(502, (M, N))
            G, W, X = dev.array(g), dev.array(w), dev.array(x)
            acc = model(g, w)
            want = np.where(x > 0, acc, np.float32(0) * acc)
        else:
            a, b, opa, opb = operands(510, ta, tb, M, N, K)
            A, B = place(dev, a, ld, 0), place(dev, b, ld, 0)
            want = model(opa, opb)
        for window in (1 << 20, None):
            dev.gemm_window(window)
            Cd = dev.full((M, N), np.nan)
            if case == "nn_mask":
                took[window] = launched(dev, lambda: c.linear_bwd_input_relu(dev, Cd, G, W, X, assign=True))
            else:
                took[window] = launched(dev, lambda: c.sgemm(dev, ta, tb, M, N, K, 1.0, A, ld, B, ld, 0.0, Cd, N))
            outs[window] = Cd.numpy()
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None)
        dev.gemm_window(None)
    assert took == {1 << 20: 0, None: 1}, took
    assert np.array_equal(outs[1 << 20], outs[None])
    assert np.array_equal(outs[None], want)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_operands_that_end_with_their_allocation(dev, ta, tb):
    """both operands are views (ld above the extent) whose LAST element is the last float of the allocation: the last tile's window
    ends exactly there.  Exact results, and the descriptor of every tile has num_records == the bytes from the tile's origin to
    the end of the window it may read - for the last tile, to the end of the allocation (the operand's real extent) - never more"""
    c = capi()
    M, N, K = 256, 128, 32 * 5
    a, b, opa, opb = operands(600, ta, tb, M, N, K)
    lda, ldb = a.shape[1] + 32, b.shape[1] + 64
    first = 4
    A, B = place(dev, a, lda, first), place(dev, b, ldb, first)       # total = first + (rows - 1) * ld + cols
    try:
        dev.gemm_kpair(0)                                            # 256-thread blocks: two-block grids would take k-pair blocks by rule
        dev.gemm_force(LOOKAHEAD_FROM_1)
        Cd = dev.full((M, N), np.nan)
        n = launched(dev, lambda: c.sgemm(dev, ta, tb, M, N, K, 1.0, A, lda, B, ldb, 0.0, Cd, N))
    finally:
        dev.gemm_force(None); dev.gemm_kpair(None)
    assert n == 1
    assert np.array_equal(Cd.numpy(), model(opa, opb))
    for kc, ld, rows, alloc in ((not ta, lda, M, A.size), (bool(tb), ldb, N, B.size)):   # operand as the kernel sees it: `rows` x K
        for row0 in range(0, rows, 128):
            origin = row0 * ld if kc else row0                       # floats from the view's base
            rec = c.gemm_buffer_records(kc, 128, ld, row0, rows, 0, K)
            window = ((127 * ld + K) if kc else ((K - 1) * ld + 128)) * 4
            assert rec == window and origin * 4 + rec <= alloc * 4, (kc, row0, rec)
            if row0 + 128 == rows:
                assert origin * 4 + rec == alloc * 4, (kc, row0, rec, "the last tile's descriptor ends with the allocation")
    # a tile that would reach past the operand's rows is clipped to the extent; an empty reduction reads nothing
    assert c.gemm_buffer_records(True, 128, 200, 64, 128, 0, 96) == (63 * 200 + 96) * 4
    assert c.gemm_buffer_records(False, 128, 200, 64, 128, 0, 96) == (95 * 200 + 64) * 4
    assert c.gemm_buffer_records(True, 128, 200, 0, 128, 96, 96) == 0
