// Quantised Linear with int8 activations (ours; contract at nk_quant_a8_linear_fwd in include/neuronika_hip.h): W8A8 / W4A8 on the int8
// matrix instruction.  Included ONCE, by nk_norm.hip, after the header of the quantised layer, whose ql_* device helpers and ql_check
// it reuses.  Two kernels, one entry; nothing here is reached from the weight-only forward, whose paths and bits stay as they are.
//   quant_a8_rows_kernel<SPLIT>   a block per row of x: the row's absmax (block maximum), sx = fl32(absmax / 127), then ONE rounding
//                           pass, 16 consecutive k per thread (from the cache the first pass filled) -> one 16-byte store of int8.  The
//                           image (M rows of K bytes, then sx[M]) lives in the device workspace and is private to this path.
//                           SPLIT (int4 weights): inside every 8 consecutive k the bytes are stored as k 0 2 4 6 | 1 3 5 7, the order in
//                           which a word of weight nibbles separates into its low and high nibbles.
//   quant_a8_gemm_kernel<BITS, MT>   grid (ceil(N / 256), ceil(M / 16 MT)), 512 threads, no K split.
//     instruction  v_mfma_i32_16x16x64_i8, A = weights (16 rows x 64 k), B = xq (64 k x 16 rows of x), D = int32.  Lane l = 16 g + r
//                  supplies 16 bytes of A row r and 16 bytes of B column r - the same 16 k of the 64-k slab in both, so any k order
//                  that the two operands share gives the same integer - and holds D[weight rows 4 g .. 4 g + 3][x row r].
//     weights      global memory -> registers, never LDS, never another type in memory.  int8: lane (r, g) loads the 16 bytes
//                  k 16 g .. 16 g + 15 of the slab of weight row r; the chunk IS the operand.  int4: 8-BYTE chunks of the 64-k slab
//                  (so that one instruction never mixes two scale groups, group 64 included): the 16 nibbles k 16 g .. 16 g + 15; a
//                  mask and a shift separate even and odd k, and ((u | 0x80808080) - 0x08080808) ^ 0x80808080 turns the stored q + 8
//                  into two's-complement bytes without a borrow between bytes.  QA_ST = 4 slabs per fragment are in flight; a chunk is
//                  replaced as soon as its operand is built.
//     xq           through LDS: the block stages a (16 MT) x 256-byte tile (QA_ST slabs) per barrier by cooperative 16-byte loads,
//                  double-buffered - the next tile travels to registers while this tile's MFMAs run, and is written to the other
//                  buffer before the one barrier of the stage.  Row stride 272 bytes = 17 slots of 16 bytes (odd), so the sixteen rows
//                  of a fragment read start on different banks.  LDS: 2 * 128 * 272 = 69632 bytes at MT = 8.
//     wave tile    a wave owns QA_NF = 2 weight fragments (32 rows; 8 waves: 256 weight rows a block) x MT in {1, 2, 4, 8} fragments
//                  of x.  Every 16-byte LDS fragment read (1 KiB a wave) feeds two MFMAs: 512 LDS bytes per MFMA of 16384 MACs.
//     registers    per (weight fragment, x fragment) pair 4 int32 span sums + 4 f32 running sums: 2 * MT * 8 = 128 at MT = 8; weights
//                  in flight 2 * 4 chunks = 32 (int8) / 16 (int4); the staged tile MT / 2 chunks = 16; scales 8; operands 12.  About
//                  200 of the 256 a 512-thread block may hold; the compiler takes 246 (int8) / 230 (int4) at MT = 8, no scratch.
//     spans        group 64 / 128: one group (1 / 2 slabs); group 0: F = 2048 k (32 slabs), the last span shorter.  At a span's end the
//                  lane converts its int32 sums (round-to-nearest-even; exact below 2^24, i.e. for groups 64 / 128), multiplies by the
//                  scales of its four weight rows and adds into the f32 sums - separate f32 operations, no fma - and fetches the next
//                  span's scales, which arrive under that span's MFMAs.
//     tails        weight rows past N, x rows past M and k past K (K % 64 == 32) are SELECTED to zero in both operands: never
//                  loaded, never stored.  Epilogue: fl32(acc * sx[m]), then + bias[n]; 16-byte stores where y allows, into the (M, N)
//                  block only.  No atomics, no inline assembly, no host synchronisation; the workspace's growth refuses capture.
//     bits         y[m][n] is a function of x[m, :], weight row n with its scales, bias[n] and (bits, group, K): integer sums are
//                  exact in any order, and the f32 chain is span-ascending for every tile shape.

namespace {

constexpr int QA_NF = 2;                             // weight fragments per wave
constexpr int QA_WAVES = 8;                          // waves per block
constexpr int QA_NT = QA_WAVES * 64;
constexpr int QA_NTILE = QA_WAVES * QA_NF * 16;      // weight rows per block
constexpr int QA_ST = 4;                             // slabs per stage = slabs in flight per fragment
constexpr int QA_LDR = QA_ST * 64 + 16;              // LDS row stride, bytes
constexpr int QA_F = 2048;                           // k per span for group 0

typedef int qa_v4i __attribute__((ext_vector_type(4)));

// The contract is written per scalar f32 operation: the GEMM kernel (and the lambdas inside it) is compiled without the packed f32
// instructions, which its span-end arithmetic would otherwise be paired into (the row quantiser has no f32 pair to pack).  Device pass
// only: the host knows no such feature.  A function with another feature set is not inlined into the kernel unless it is
// __forceinline__, so the kernel builds its vectors and its barrier from the helpers below, not from the HIP header's functions.
#if defined(__HIP_DEVICE_COMPILE__)
#define QA_SCALAR_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define QA_SCALAR_F32
#endif

__device__ __forceinline__ float qa_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

template <bool SPLIT>
__global__ __launch_bounds__(256) void quant_a8_rows_kernel(const float* __restrict__ x, long long ldx, unsigned char* __restrict__ xq,
                                                            float* __restrict__ sx, int M, int K, int xvec) {
    __shared__ float red[4];
    for (long long m = blockIdx.x; m < M; m += gridDim.x) {
        const float* row = x + m * ldx;
        float a = 0.f;
        for (int k = threadIdx.x * 4; k < K; k += 1024) a = fmaxf(a, ql_absmax4(ql_load4(row + k, xvec != 0)));
        a = nk_block_max<256>(a, red);
        const float s = ql_div(a, 127.f);
        if (threadIdx.x == 0) sx[m] = s;
        for (int k = threadIdx.x * 16; k < K; k += 4096) {  // K % 16 == 0: a chunk lies wholly below K
            unsigned w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = ql_quant4<8>(ql_load4(row + k + 4 * j, xvec != 0), s);
            if (SPLIT) {
#pragma unroll
                for (int j = 0; j < 4; j += 2) {
                    const unsigned lo = w[j], hi = w[j + 1];
                    w[j] = (lo & 0xffu) | ((lo >> 8) & 0xff00u) | ((hi & 0xffu) << 16) | ((hi << 8) & 0xff000000u);
                    w[j + 1] = ((lo >> 8) & 0xffu) | ((lo >> 16) & 0xff00u) | ((hi << 8) & 0xff0000u) | (hi & 0xff000000u);
                }
            }
            *reinterpret_cast<uint4*>(xq + m * K + k) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

// what a lane loads of a weight row per slab, and the A operand it becomes
template <int BITS> struct qa_chunk { typedef uint4 type; };
template <> struct qa_chunk<4> { typedef uint2 type; };

__device__ __forceinline__ uint4 qa_u4(unsigned a, unsigned b, unsigned c, unsigned d) {
    uint4 v;
    v.x = a; v.y = b; v.z = c; v.w = d;
    return v;
}
__device__ __forceinline__ void qa_barrier() {  // what __syncthreads() is made of
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ uint4 qa_zero(const uint4*) { return qa_u4(0u, 0u, 0u, 0u); }
__device__ __forceinline__ uint2 qa_zero(const uint2*) {  // nibbles q + 8 of q = 0
    uint2 v;
    v.x = 0x88888888u; v.y = 0x88888888u;
    return v;
}
__device__ __forceinline__ qa_v4i qa_operand(const uint4& c) { return qa_v4i{(int)c.x, (int)c.y, (int)c.z, (int)c.w}; }
__device__ __forceinline__ int qa_bytes(unsigned u) { return (int)(((u | 0x80808080u) - 0x08080808u) ^ 0x80808080u); }
__device__ __forceinline__ qa_v4i qa_operand(const uint2& c) {
    return qa_v4i{qa_bytes(c.x & 0x0f0f0f0fu), qa_bytes((c.x >> 4) & 0x0f0f0f0fu), qa_bytes(c.y & 0x0f0f0f0fu), qa_bytes((c.y >> 4) & 0x0f0f0f0fu)};
}

template <int BITS, int MT>
__global__ QA_SCALAR_F32 __launch_bounds__(QA_NT) void quant_a8_gemm_kernel(const unsigned char* __restrict__ xq, const float* __restrict__ sx,
                                                              const unsigned char* __restrict__ qw, const float* __restrict__ scales,
                                                              const float* __restrict__ bias, float* __restrict__ y, long long ldy, int M,
                                                              int N, int K, int gshift, int span, int yvec) {
    typedef typename qa_chunk<BITS>::type chunk_t;
    constexpr int WB = BITS * 2;                                // bytes of a weight row a lane loads per slab
    constexpr int XR = 16 * MT;                                 // rows of the xq tile
    constexpr int NST = (XR * 16 + QA_NT - 1) / QA_NT;          // 16-byte chunks a thread stages per tile
    __shared__ __attribute__((aligned(16))) unsigned char xs[2][XR * QA_LDR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const long long m0 = (long long)blockIdx.y * XR;
    const long long nbase = (long long)blockIdx.x * QA_NTILE + wave * (QA_NF * 16);
    const int nsl = (K + 63) / 64;                              // slabs
    const int nstage = (nsl + QA_ST - 1) / QA_ST;
    const int spr = gshift < 31 ? K >> gshift : 1;              // scales per weight row
    const unsigned char* wrow[QA_NF];
    bool wrow_on[QA_NF];
#pragma unroll
    for (int f = 0; f < QA_NF; ++f) {
        wrow_on[f] = nbase + 16 * f + r < N;
        wrow[f] = qw + (wrow_on[f] ? nbase + 16 * f + r : 0) * ((long long)K * BITS / 8) + g * WB;
    }

    auto chunk_load = [&](int slab, int f) QA_SCALAR_F32 -> chunk_t {
        return wrow_on[f] && slab * 64 + 16 * g < K ? *reinterpret_cast<const chunk_t*>(wrow[f] + (long long)slab * (4 * WB))
                                                     : qa_zero((const chunk_t*)nullptr);
    };
    // chunk `idx` of a tile is row idx / 16, bytes 16 (idx % 16) of the stage's 256
    auto stage_load = [&](int stage, uint4 (&st)[NST]) QA_SCALAR_F32 {
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int idx = tid + j * QA_NT;
            const long long m = m0 + (idx >> 4);
            const int k = stage * (QA_ST * 64) + 16 * (idx & 15);
            st[j] = (NST * QA_NT == XR * 16 || idx < XR * 16) && m < M && k < K ? *reinterpret_cast<const uint4*>(xq + m * K + k)
                                                                               : qa_u4(0u, 0u, 0u, 0u);
        }
    };
    auto stage_store = [&](int buf, const uint4 (&st)[NST]) QA_SCALAR_F32 {
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int idx = tid + j * QA_NT;
            if (NST * QA_NT == XR * 16 || idx < XR * 16) *reinterpret_cast<uint4*>(&xs[buf][(idx >> 4) * QA_LDR + 16 * (idx & 15)]) = st[j];
        }
    };
    // the scales of span j for the lane's weight rows 4 g .. 4 g + 3 of each fragment
    auto scales_load = [&](int j, float (&sc)[QA_NF][4]) QA_SCALAR_F32 {
        const int at = gshift < 31 ? j : 0;
#pragma unroll
        for (int f = 0; f < QA_NF; ++f)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long n = nbase + 16 * f + 4 * g + i;
                sc[f][i] = n < N && at < spr ? scales[n * spr + at] : 0.f;
            }
    };

    qa_v4i isum[QA_NF][MT];
    float acc[QA_NF][MT][4];
#pragma unroll
    for (int f = 0; f < QA_NF; ++f)
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            isum[f][t] = qa_v4i{0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[f][t][i] = 0.f;
        }
    chunk_t raw[QA_ST][QA_NF];
#pragma unroll
    for (int u = 0; u < QA_ST; ++u)
#pragma unroll
        for (int f = 0; f < QA_NF; ++f) raw[u][f] = chunk_load(u, f);
    float sc[QA_NF][4];
    scales_load(0, sc);
    {
        uint4 st[NST];
        stage_load(0, st);
        stage_store(0, st);
    }
    qa_barrier();

    for (int s = 0; s < nstage; ++s) {
        uint4 st[NST];
        stage_load(s + 1, st);  // past K: zeros, no load
#pragma unroll
        for (int u = 0; u < QA_ST; ++u) {
            const int slab = s * QA_ST + u;
            if (slab < nsl) {  // the whole block
                qa_v4i a[QA_NF];
#pragma unroll
                for (int f = 0; f < QA_NF; ++f) {
                    a[f] = qa_operand(raw[u][f]);
                    raw[u][f] = chunk_load(slab + QA_ST, f);
                }
                const unsigned char* xb = &xs[s & 1][r * QA_LDR + 64 * u + 16 * g];
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    const qa_v4i b = *reinterpret_cast<const qa_v4i*>(xb + t * 16 * QA_LDR);
#pragma unroll
                    for (int f = 0; f < QA_NF; ++f) isum[f][t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[f], b, isum[f][t], 0, 0, 0);
                }
                if (((slab + 1) & (span - 1)) == 0 || slab == nsl - 1) {  // a span ends: the whole block
#pragma unroll
                    for (int f = 0; f < QA_NF; ++f)
#pragma unroll
                        for (int t = 0; t < MT; ++t) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) acc[f][t][i] = qa_add(acc[f][t][i], ql_mul((float)isum[f][t][i], sc[f][i]));
                            isum[f][t] = qa_v4i{0, 0, 0, 0};
                        }
                    if (slab + 1 < nsl) scales_load((slab + 1) / span, sc);
                }
            }
        }
        stage_store((s + 1) & 1, st);
        qa_barrier();
    }

    // lane (c = r, g) holds x row m0 + 16 t + c against weight rows nbase + 16 f + 4 g .. + 3
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const long long m = m0 + 16 * t + r;
        if (m >= M) continue;
        const float sxm = sx[m];
#pragma unroll
        for (int f = 0; f < QA_NF; ++f) {
            const long long n0 = nbase + 16 * f + 4 * g;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = ql_mul(acc[f][t][i], sxm);
                if (bias && n0 + i < N) v[i] = qa_add(v[i], bias[n0 + i]);
            }
            if (yvec && n0 + 3 < N) {
                float4 o;
                o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
                *reinterpret_cast<float4*>(y + m * ldy + n0) = o;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (n0 + i < N) y[m * ldy + n0 + i] = v[i];
            }
        }
    }
}

template <int BITS>
void qa_launch(nk_device* dev, const unsigned char* xq, const float* sx, const float* qw, const float* scales, const float* bias, float* y,
               long long ldy, int M, int N, int K, int group) {
    const int mt = M <= 16 ? 1 : M <= 32 ? 2 : M <= 64 ? 4 : 8;
    const dim3 grid((unsigned)((N + QA_NTILE - 1) / QA_NTILE), (unsigned)((M + 16 * mt - 1) / (16 * mt)));
    const int span = group ? group / 64 : QA_F / 64;
    const int yvec = al16(y) && ldy % 4 == 0;
#define NK_QA(MT)                                                                                                                       \
    hipLaunchKernelGGL((quant_a8_gemm_kernel<BITS, MT>), grid, dim3(QA_NT), 0, dev->compute, xq, sx, reinterpret_cast<const unsigned char*>(qw), \
                       scales, bias, y, ldy, M, N, K, ql_gshift(group), span, yvec)
    if (mt == 1) NK_QA(1);
    else if (mt == 2) NK_QA(2);
    else if (mt == 4) NK_QA(4);
    else NK_QA(8);
#undef NK_QA
}
#undef QA_SCALAR_F32

}  // namespace

extern "C" int nk_quant_a8_linear_fwd(nk_device* dev, const float* x, int ldx, const float* qw, const float* scales, const float* bias, float* y,
                                      int ldy, int M, int N, int K, int bits, int group) {
    NK_USE(dev);
    if (int rc = ql_check("nk_quant_a8_linear_fwd", N, K, bits, group)) return rc;
    NK_CHECK(group != 32, "nk_quant_a8_linear_fwd: group = 32 (one 64-k instruction would straddle two scales: 64, 128 or 0)");
    NK_CHECK(K <= (1 << 30), "nk_quant_a8_linear_fwd: K = %d is beyond this path (2^30)", K);
    NK_CHECK(M >= 0, "nk_quant_a8_linear_fwd: M = %d", M);
    NK_CHECK(x && qw && scales && y, "null pointer in nk_quant_a8_linear_fwd (only bias may be NULL)");
    NK_CHECK(ldx >= K && ldy >= N, "nk_quant_a8_linear_fwd: ldx = %d < K = %d or ldy = %d < N = %d", ldx, K, ldy, N);
    NK_CHECK(al16(qw), "nk_quant_a8_linear_fwd: qw must be 16-byte aligned");
    NK_CHECK((M + 127) / 128 <= 65535, "nk_quant_a8_linear_fwd: M = %d is beyond one launch", M);
    if (M == 0) return NK_OK;
    void* ws = nullptr;
    if (int rc = nk_workspace(dev, (size_t)M * (size_t)K + (size_t)M * sizeof(float), &ws)) return rc;
    unsigned char* xq = reinterpret_cast<unsigned char*>(ws);
    float* sx = reinterpret_cast<float*>(xq + (size_t)M * (size_t)K);  // M * K is a multiple of 32
    const int xvec = al16(x) && ldx % 4 == 0;
    const dim3 qgrid((unsigned)(M < (1 << 20) ? M : (1 << 20)));
    if (bits == 4) hipLaunchKernelGGL(quant_a8_rows_kernel<true>, qgrid, dim3(256), 0, dev->compute, x, (long long)ldx, xq, sx, M, K, xvec);
    else hipLaunchKernelGGL(quant_a8_rows_kernel<false>, qgrid, dim3(256), 0, dev->compute, x, (long long)ldx, xq, sx, M, K, xvec);
    NK_LAUNCH_CHECK();
    if (int rc = nk_prof_start(dev, NK_KERNEL_QUANT_A8, 2.0 * M * N * (double)K)) return rc;
    if (bits == 8) qa_launch<8>(dev, xq, sx, qw, scales, bias, y, ldy, M, N, K, group);
    else qa_launch<4>(dev, xq, sx, qw, scales, bias, y, ldy, M, N, K, group);
    NK_LAUNCH_CHECK();
    return nk_prof_stop(dev);
}
