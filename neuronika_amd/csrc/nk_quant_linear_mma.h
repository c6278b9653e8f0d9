// Weight-only quantised Linear, the fused-dequant MFMA kernel (ours): y[m][n] = bias[n] + sum_k x[m][k] * w^[n][k] for up to 128 rows
// of x per pass over the weights, each weight converted ONCE in registers and fed to the matrix unit for all rows.  The weight never
// exists as f32 outside registers.  Included ONCE, by nk_norm.hip, after the header of the quantised layer, whose ql_* helpers and
// nk_quant_linear_fwd it serves (ql_mma_fwd below is the one entry).
//   quant_linear_mma_kernel<BITS, MT>   grid (ceil(N / 128), S), 512 threads.  A wave owns QM_NR = 16 weight rows, the QM_WAVES = 8
//                           waves of a block 128, and MT in {1, 2, 4, 8} accumulator tiles of 16 rows of x (16 MT rows a pass).
//     instruction  v_mfma_f32_16x16x4_f32 with A = weights (16 rows x 4 k), B = x (4 k x 16 rows of x).  Lane l = 16 g + r supplies
//                  A[row r][k-slot g] and B[k-slot g][x row r], and holds D[weight rows 4 g .. 4 g + 3][x row r].
//     k order      A slab is QM_SLAB = 64 (int8) / 128 (int4) consecutive k = four 16-byte chunks of a weight row.  Lane (r, g) loads
//                  chunk g of the slab of weight row r straight from global memory into registers: the slab's k g E .. g E + E - 1
//                  with E = 16 / 32.  MFMA step j of the slab multiplies element j of every lane's chunk, so lane (c, g) of B needs x
//                  row c at the same E consecutive k: a contiguous fragment, read from LDS sixteen bytes at a time.  No transpose,
//                  no shuffle.  The A operand is ql_mul(float(q), s) = w^, the format's value, so a group of 32 inside a slab is no
//                  special case.
//     x            the block stages the slab's (16 MT) x QM_SLAB tile of x in LDS by 16-byte cooperative loads (scalar loads of the
//                  same values when x or ldx break the alignment), double-buffered: the next slab's tile travels to registers while
//                  this slab's MFMAs run and is written to the other buffer before the one barrier of the slab.  Row stride
//                  QM_SLAB + 4 floats: an odd number of 16-byte slots, so the sixteen rows of a fragment read land on different banks.
//     weights      never touch LDS.  QM_U chunks per lane are in flight (with their scales); a chunk is replaced as soon as it is used.
//     tails        weight rows past N, x rows past M and k past K are SELECTED to zero: never loaded, never multiplied by zero.
//                  Nothing outside x[0..M) x [0..K), the N weight rows and the (M, N) block of y is touched.
//     K split      blockIdx.y = slice of QM_SLICE = 2048 k (the project's chain bound), S = ceil(K / 2048), the last may be shorter.
//                  S == 1: y = sum + bias.  S > 1: the slice's sum goes to the device workspace (S * M * N floats) and
//                  quant_linear_mma_sum_kernel adds the partials in ascending slice order, then the bias.  The matrix unit's
//                  sums are plain f32 adds in a fixed order; nothing is allocated per call, so a warmed call is capturable.
//     bits         the chain of y[m][n] is: slices ascending; inside a slice slabs ascending, steps ascending, the instruction's own
//                  4-way sum over the k-slots of a step.  It holds x[m, :], weight row n with its scales, bias[n] and (bits, group, K)
//                  and nothing else: not M, N, MT, the pass, the tile slot, ldx / ldy or the alignment of x.  These are NOT the rows
//                  kernels' bits (per-unit scaling, lane butterfly) and NOT the GEMM's over the unpacked weights (other k order).
// Dispatch (nk_quant_linear_fwd): after the rows path, M <= U(bits) (QM_RULE_*) when N * K >= QL_MMA_MIN_WEIGHTS; NK_TUNE_QUANT_MMA
// overrides both.  Measured: DESIGN.md "Weight-only quantised Linear: the MFMA kernel".

namespace {

constexpr int QM_NR = 16;       // weight rows per wave: one A fragment
constexpr int QM_WAVES = 8;     // waves per block
constexpr int QM_NT = QM_WAVES * 64;
constexpr int QM_U = 4;         // weight chunks (slabs) in flight per lane
constexpr int QM_SLICE = 2048;  // k per slice
constexpr int QM_ROWS = 128;    // rows of x per pass (MT = 8)
constexpr int QM_RULE_8 = 512, QM_RULE_4 = 256;     // U(bits): this kernel up to that M by rule (measured: DESIGN.md)
constexpr long long QL_MMA_MIN_WEIGHTS = 1LL << 20;  // ... for layers of at least that many weights

typedef float qm_v4f __attribute__((ext_vector_type(4)));

// the chunk that dequantises to +0 whatever the scale: the select for weight rows past N and k past K
template <int BITS>
__device__ __forceinline__ uint4 qm_zero_chunk() {
    return BITS == 8 ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(0x88888888u, 0x88888888u, 0x88888888u, 0x88888888u);
}

template <int BITS, int MT>
__global__ __launch_bounds__(QM_NT) void quant_linear_mma_kernel(const float* __restrict__ x, long long ldx, const uint4* __restrict__ qw,
                                                                  const float* __restrict__ scales, const float* __restrict__ bias,
                                                                  float* __restrict__ y, long long ldy, float* __restrict__ part,
                                                                  long long part_stride, int rows, int N, int K, int gshift, int xvec) {
    constexpr int E = 128 / BITS;        // elements per chunk
    constexpr int SLAB = 4 * E;          // k per slab
    constexpr int LDT = SLAB + 4;        // LDS row stride, floats
    constexpr int XR = 16 * MT;          // rows of the x tile
    constexpr int QPR = SLAB / 4;        // float4s per tile row
    constexpr int NST = (XR * QPR + QM_NT - 1) / QM_NT;  // float4s a thread stages per slab
    __shared__ __attribute__((aligned(16))) float xs[2][XR * LDT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int k0 = blockIdx.y * QM_SLICE;
    const int kend = k0 + QM_SLICE < K ? k0 + QM_SLICE : K;
    const int nsl = (kend - k0 + SLAB - 1) / SLAB;  // slabs of this slice
    const long long nbase = ((long long)blockIdx.x * QM_WAVES + wave) * QM_NR;
    const int nch = K / E;                          // chunks per weight row
    const int spr = gshift < 31 ? K >> gshift : 1;  // scales per weight row
    const bool wrow_on = nbase + r < N;
    const uint4* wrow = qw + (wrow_on ? nbase + r : 0) * nch;
    const float* srow = scales + (wrow_on ? nbase + r : 0) * spr;

    // the x tile: float4 `idx` of the tile is row idx / QPR, k 4 (idx % QPR)
    auto stage_load = [&](int slab, float4 (&st)[NST]) {
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int idx = tid + j * QM_NT;
            const int row = idx / QPR, k = k0 + slab * SLAB + 4 * (idx % QPR);
            st[j] = (NST * QM_NT == XR * QPR || idx < XR * QPR) && row < rows && k < kend ? ql_load4(x + row * ldx + k, xvec != 0)
                                                                                          : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stage_store = [&](int buf, const float4 (&st)[NST]) {
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int idx = tid + j * QM_NT;
            if (NST * QM_NT == XR * QPR || idx < XR * QPR) *reinterpret_cast<float4*>(&xs[buf][(idx / QPR) * LDT + 4 * (idx % QPR)]) = st[j];
        }
    };
    // chunk g of slab `slab` of the lane's weight row, and its scale
    auto chunk_load = [&](int slab, uint4& raw, float& s) {
        const int k = k0 + slab * SLAB + g * E;
        const bool on = wrow_on && slab < nsl && k < kend;
        raw = on ? wrow[k / E] : qm_zero_chunk<BITS>();
        s = on ? srow[k >> gshift] : 0.f;
    };

    qm_v4f acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = qm_v4f{0.f, 0.f, 0.f, 0.f};
    uint4 raw[QM_U];
    float sc[QM_U];
#pragma unroll
    for (int u = 0; u < QM_U; ++u) chunk_load(u, raw[u], sc[u]);
    {
        float4 st[NST];
        stage_load(0, st);
        stage_store(0, st);
    }
    __syncthreads();

    for (int s0 = 0; s0 < nsl; s0 += QM_U) {
#pragma unroll
        for (int u = 0; u < QM_U; ++u) {
            const int slab = s0 + u;
            if (slab < nsl) {  // the whole block
                const uint4 cur = raw[u];
                const float s = sc[u];
                float4 st[NST];
                stage_load(slab + 1, st);  // past the slice: zeros, no load
                chunk_load(slab + QM_U, raw[u], sc[u]);
                const float* xb = &xs[u & 1][r * LDT + g * E];
#pragma unroll
                for (int qd = 0; qd < E / 4; ++qd) {
                    float a[4];
                    ql_quad<BITS>(cur, qd / 4, qd % 4, a);
#pragma unroll
                    for (int i = 0; i < 4; ++i) a[i] = ql_mul(a[i], s);
                    float4 b[MT];
#pragma unroll
                    for (int t = 0; t < MT; ++t) b[t] = *reinterpret_cast<const float4*>(xb + t * 16 * LDT + 4 * qd);
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[t].x, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[t].y, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[t].z, acc[t], 0, 0, 0);
                        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[t].w, acc[t], 0, 0, 0);
                    }
                }
                stage_store((u + 1) & 1, st);
                __syncthreads();
            }
        }
    }

    // lane (c = r, g) holds x row 16 t + c against weight rows nbase + 4 g .. + 3
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = 16 * t + r;
        if (m >= rows) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long n = nbase + 4 * g + i;
            if (n >= N) continue;
            if (part) part[blockIdx.y * part_stride + (long long)m * N + n] = acc[t][i];
            else y[m * ldy + n] = bias ? acc[t][i] + bias[n] : acc[t][i];
        }
    }
}

// y[m][n] = ((p_0 + p_1) + ... + p_{S-1}) + bias[n] over the S slice sums of the workspace
__global__ __launch_bounds__(256) void quant_linear_mma_sum_kernel(const float* __restrict__ part, long long part_stride, int S,
                                                                  const float* __restrict__ bias, float* __restrict__ y, long long ldy, int M, int N) {
    const long long total = (long long)M * N;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long m = t / N;
        const int n = (int)(t - m * N);
        float s = part[t];
        for (int i = 1; i < S; ++i) s += part[i * part_stride + t];
        y[m * ldy + n] = bias ? s + bias[n] : s;
    }
}

template <int BITS>
void qm_launch(nk_device* dev, int rows, const float* x, long long ldx, const uint4* qw, const float* scales, const float* bias, float* y,
               long long ldy, float* part, long long part_stride, int N, int K, int gshift, int xvec) {
    const dim3 grid((unsigned)((N + QM_WAVES * QM_NR - 1) / (QM_WAVES * QM_NR)), (unsigned)((K + QM_SLICE - 1) / QM_SLICE));
#define NK_QM(MT)                                                                                                                         \
    hipLaunchKernelGGL((quant_linear_mma_kernel<BITS, MT>), grid, dim3(QM_NT), 0, dev->compute, x, ldx, qw, scales, bias, y, ldy, part, \
                       part_stride, rows, N, K, gshift, xvec)
    if (rows <= 16) NK_QM(1);
    else if (rows <= 32) NK_QM(2);
    else if (rows <= 64) NK_QM(4);
    else NK_QM(8);
#undef NK_QM
}

int ql_mma_limit(const nk_device* dev, int N, int K, int bits) {
    if ((K + QM_SLICE - 1) / QM_SLICE > 65535) return 0;  // more slices than a grid's y extent: unpack + GEMM
    if (dev->tune_quant_mma >= 0) return dev->tune_quant_mma;
    return (long long)N * K >= QL_MMA_MIN_WEIGHTS ? nk_quant_linear_mma_rule(bits) : 0;
}

// the arguments are nk_quant_linear_fwd's, checked there; M > 0
int ql_mma_fwd(nk_device* dev, const float* x, int ldx, const float* qw, const float* scales, const float* bias, float* y, int ldy, int M,
               int N, int K, int bits, int group) {
    const int S = (K + QM_SLICE - 1) / QM_SLICE;
    const long long part_stride = (long long)M * N;
    float* part = nullptr;
    if (S > 1) {
        void* p = nullptr;
        if (int rc = nk_workspace(dev, (size_t)S * (size_t)part_stride * sizeof(float), &p)) return rc;
        part = (float*)p;
    }
    const int xvec = al16(x) && ldx % 4 == 0;
    for (int m0 = 0; m0 < M; m0 += QM_ROWS) {
        const int rows = M - m0 < QM_ROWS ? M - m0 : QM_ROWS;
        const float* xp = x + (long long)m0 * ldx;
        float* yp = y + (long long)m0 * ldy;
        float* pp = part ? part + (long long)m0 * N : nullptr;
        if (bits == 8) qm_launch<8>(dev, rows, xp, ldx, reinterpret_cast<const uint4*>(qw), scales, bias, yp, ldy, pp, part_stride, N, K, ql_gshift(group), xvec);
        else qm_launch<4>(dev, rows, xp, ldx, reinterpret_cast<const uint4*>(qw), scales, bias, yp, ldy, pp, part_stride, N, K, ql_gshift(group), xvec);
        NK_LAUNCH_CHECK();
    }
    if (part) {
        hipLaunchKernelGGL(quant_linear_mma_sum_kernel, dim3(nk_stream_grid((size_t)part_stride, 256)), dim3(256), 0, dev->compute, part, part_stride, S,
                           bias, y, (long long)ldy, M, N);
        NK_LAUNCH_CHECK();
    }
    return NK_OK;
}

}  // namespace

extern "C" int nk_quant_linear_mma_rule(int bits) { return bits == 8 ? QM_RULE_8 : bits == 4 ? QM_RULE_4 : 0; }
