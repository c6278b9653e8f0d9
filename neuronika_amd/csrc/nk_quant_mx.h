// Microscaling Linear (ours; format and contract at nk_quant_mx_* in include/neuronika_hip.h): MXFP4 weights, MXFP8 (E4M3) rows of x,
// multiplied on gfx950's block-scaled matrix instruction.  Included ONCE, by nk_norm.hip, after nk_quant_a8.h; it reuses ql_load4,
// ql_mul and ql_store_quads of the quantised layer and touches none of its paths.
//   quant_mx_kernel<FP4>    pack (FP4) and row quantiser (!FP4), one streaming body: a wave owns 256 consecutive elements of one row
//                           (a float4 per lane, 16-byte loads where the source allows), a 32-block is 8 neighbouring lanes, its
//                           absmax an xor-shuffle maximum over them - taken on the f32 BITS without their sign, which order as
//                           the magnitudes do.  The block's E8M0 byte is the absmax's exponent field minus emax (2 / 8), clamped to
//                           [0, 254]; 127 for a zero block.  Every element is scaled by the exact power of two 2^(127 - e), rounded
//                           with ONE rintf at the spacing of its binade (mx_encode) and saturated; the codes of 8 (fp4) / 4 (fp8)
//                           lanes leave in one 16-byte store.  The forward runs the !FP4 form into the device workspace, whose
//                           scale rows are padded to a multiple of 16 bytes so that the GEMM kernels load them aligned.
//   quant_mx_unpack_kernel  a 16-byte chunk IS one 32-block: a thread decodes it against its one scale byte -> 8 float4 stores.
//   quant_mx_gemm_kernel<MT>   M > 16.  Grid (ceil(N / 256), ceil(M / 16 MT)), 512 threads, no K split, MT in {2, 4, 8}.
//     instruction  v_mfma_scale_f32_16x16x128_f8f6f4, A = weights as fp4 (cbsz 4), B = the x image as fp8 (blgp 0).  A slab is 128 k.
//                  Lane l = 16 g + r supplies, for weight row r, k 32 g .. 32 g + 31 of the slab (16 bytes, even k in the low
//                  nibble); for x row r, k 16 g .. 16 g + 15 in its first four registers and k 64 + 16 g .. 64 + 16 g + 15 in the
//                  last four (the 8-bit operand is laid out as two 64-k halves; read off the device with one-hot rows of x); and
//                  the E8M0 byte of block 4 slab + g of either row in the low byte of its scale operands (op_sel 0): the
//                  instruction scales k 32 j .. 32 j + 31 of a row by the byte of lane 16 j + r.  The lane holds
//                  D[weight rows 4 g .. 4 g + 3][x row r].  The scales are applied inside the instruction: the k-loop holds loads
//                  and matrix instructions only.
//     weights      global memory -> registers, never LDS: the lane's 16-byte load is the operand.  MX_ST = 4 slabs per fragment
//                  and their scale bytes are in flight; a chunk is replaced as soon as it has been used.
//     x image      through LDS, double-buffered: a stage is MX_ST slabs = 512 bytes of each of the 16 MT rows plus the 16 scale
//                  bytes of every row, staged by cooperative 16-byte loads while the previous stage's MFMAs run; one barrier a
//                  stage.  Row stride 528 bytes = 33 slots of 16 bytes.  A lane reads its two 16-byte halves (64 bytes apart) one
//                  by one; a read instruction is served 16 lanes at a time (64 banks of 4 bytes = 16 slots), and the 16 lanes of one g sit at
//                  slot (33 r + const) mod 16 = (r + const) mod 16: sixteen different slots, no conflict.  The two halves are two
//                  instructions and cannot collide.  Scale bytes: the four g of a row share a dword (broadcast), the sixteen rows
//                  are 16 bytes apart (four banks each): conflict-free.  LDS at MT = 8: 2 * 128 * (528 + 16) = 139264 bytes.
//     accumulator  one float4 per (weight fragment, x fragment), chained through the C operand from slab 0 to the last slab.
//     tails        k past K (K % 128 in {32, 64, 96}), weight rows past N and x rows past M are SELECTED to zero elements with scale
//                  byte 127: never loaded, never stored.  Epilogue: + bias[n]; 16-byte stores where y allows.
//   quant_mx_skinny_kernel<NF>   M <= 16 (decode).  One x fragment; a block of 8 waves owns 16 NF weight rows (NF = 2 from N = 8192
//                  rows, so a 4096-wide layer launches 256 blocks); wave w takes slabs w, w + 8, ... - MX_SKU = 4 of them in flight,
//                  weights and x image both straight from global memory (the image is shared by all blocks and stays in the
//                  cache).  The eight partial float4s meet in LDS (8 KiB per fragment) and are added in ascending wave order, then
//                  the bias.  The kernel is bound by reading 0.53 bytes per weight.
//   bits           Within one kernel class y[m][n] is a function of x[m, :], row n of qw / sw, bias[n] and K only: not of M, N, MT,
//                  NF, the tile a row lands in, ldx / ldy or the alignment of x.  The classes differ from each other: the wide
//                  kernel chains all slabs in one accumulator, the skinny kernel adds eight interleaved chains.
//   No atomics, no inline assembly, no host synchronisation; the workspace's growth refuses capture, a warmed call is capturable.
//   Resources (-Rpass-analysis=kernel-resource-usage, gfx950; no kernel uses scratch):
//                  quant_mx_gemm_kernel<2 / 4 / 8>   121 / 152 / 213 VGPRs, 34816 / 69632 / 139264 bytes of LDS
//                  quant_mx_skinny_kernel<1 / 2>     84 / 112 VGPRs, 8192 / 16384 bytes of LDS
//                  quant_mx_kernel<fp4 / fp8>        15 / 17 VGPRs, no LDS
//                  quant_mx_unpack_kernel            33 VGPRs, no LDS

namespace {

constexpr int MX_NF = 2;                             // weight fragments per wave (wide kernel)
constexpr int MX_WAVES = 8;                          // waves per block, both GEMM kernels
constexpr int MX_NT = MX_WAVES * 64;
constexpr int MX_NTILE = MX_WAVES * MX_NF * 16;      // weight rows per block (wide kernel)
constexpr int MX_ST = 4;                             // slabs per stage = weight slabs in flight per fragment
constexpr int MX_LDR = MX_ST * 128 + 16;             // LDS row stride of the x image, bytes
constexpr int MX_SKU = 4;                            // slabs in flight per wave (skinny kernel)
constexpr int MX_SK_WIDE_N = 8192;                   // skinny kernel: 32 weight rows a block from this N

typedef int mx_v8i __attribute__((ext_vector_type(8)));
typedef float mx_v4f __attribute__((ext_vector_type(4)));

// ---- format ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned mx_absbits4(const float4& v) {
    const unsigned a = __float_as_uint(v.x) & 0x7fffffffu, b = __float_as_uint(v.y) & 0x7fffffffu;
    const unsigned c = __float_as_uint(v.z) & 0x7fffffffu, d = __float_as_uint(v.w) & 0x7fffffffu;
    return max(max(a, b), max(c, d));
}
// E8M0 byte of a block from the bits of its absmax: exponent field - emax, clamped; 127 for a zero block
template <int EMAX>
__device__ __forceinline__ unsigned mx_scale_byte(unsigned absbits) {
    const int e = (int)(absbits >> 23) - EMAX;
    return absbits == 0u ? 127u : (unsigned)min(max(e, 0), 254);
}
// The code of w * up (up = 2^(127 - e), exact) in a sign / exponent (bias BIAS) / MB-bit mantissa format without infinities: E2M1
// <1, 1> saturating at 6, E4M3 <3, 7> saturating at 448.  E is the binade of |v| (the lowest one for subnormals), 2^(E - MB) its
// spacing; rintf rounds half to even.  A zero code carries no sign; a NaN leaves as the maximum.
template <int MB, int BIAS>
__device__ __forceinline__ unsigned mx_encode(float w, float up) {
    constexpr float MAXV = MB == 1 ? 6.f : 448.f;
    const float v = ql_mul(fabsf(w), up);
    const int E = max((int)(__float_as_uint(v) >> 23) - 127, 1 - BIAS);
    const float r = fminf(ql_mul(rintf(ql_mul(v, __uint_as_float((unsigned)(127 + MB - E) << 23))), __uint_as_float((unsigned)(127 - MB + E) << 23)), MAXV);
    const unsigned mag = r >= __uint_as_float((unsigned)(128 - BIAS) << 23) ? (__float_as_uint(r) >> (23 - MB)) - ((unsigned)(127 - BIAS) << MB)
                                                                           : (unsigned)ql_mul(r, (float)(1 << (BIAS - 1 + MB)));
    return mag ? mag | ((__float_as_uint(w) >> 31) << (MB == 1 ? 3 : 7)) : 0u;
}
// the value of an E2M1 nibble: 0, 0.5, 1, 1.5, 2, 3, 4, 6 with the sign in bit 3
__device__ __forceinline__ float mx_e2m1(unsigned nib) {
    const unsigned m = nib & 7u;
    const unsigned mag = m < 2u ? (m ? 0x3f000000u : 0u) : (((m >> 1) + 126u) << 23) | ((m & 1u) << 22);
    return __uint_as_float(mag | ((nib & 8u) << 28));
}

template <bool FP4>
__global__ __launch_bounds__(256) void quant_mx_kernel(const float* __restrict__ W, long long ldw, unsigned char* __restrict__ q,
                                                       unsigned char* __restrict__ s, long long lds, long long N, int K, int wvec) {
    const int lane = threadIdx.x & 63;
    const int cpr = (K + 255) / 256;  // wave spans per row
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= N * cpr) return;  // the whole wave
    const long long n = wid / cpr;
    const int k = (int)(wid - n * cpr) * 256 + lane * 4;
    const bool on = k < K;  // a 32-block lies wholly below K or wholly beyond it
    const float4 v = on ? ql_load4(W + n * ldw + k, wvec != 0) : make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned a = mx_absbits4(v);
    for (int off = 1; off < 8; off <<= 1) a = max(a, (unsigned)__shfl_xor((int)a, off, 64));
    const unsigned e = mx_scale_byte<FP4 ? 2 : 8>(a);
    if (on && (lane & 7) == 0) s[n * lds + (k >> 5)] = (unsigned char)e;
    const float up = __uint_as_float((254u - e) << 23);
    const float el[4] = {v.x, v.y, v.z, v.w};
    unsigned word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) word |= FP4 ? mx_encode<1, 1>(el[j], up) << (4 * j) : mx_encode<3, 7>(el[j], up) << (8 * j);
    if (FP4) ql_store_quads<4>(q + n * (K / 2), k, word, on);
    else ql_store_quads<8>(q + n * K, k, word, on);
}

__global__ __launch_bounds__(256) void quant_mx_unpack_kernel(const uint4* __restrict__ qw, const unsigned char* __restrict__ sw,
                                                              float* __restrict__ W, long long ldw, long long N, int K, int wvec) {
    const int nch = K / 32;
    const long long total = N * nch;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long n = t / nch;
        const uint4 raw = qw[t];
        const unsigned e = sw[t];
        const float sc = __uint_as_float(e ? e << 23 : 0x00400000u);  // 2^(e - 127); e = 0 is the subnormal 2^-127
        const unsigned w[4] = {raw.x, raw.y, raw.z, raw.w};
        float* o = W + n * ldw + (t - n * nch) * 32;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float f[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] = ql_mul(mx_e2m1((w[j] >> (4 * i)) & 15u), sc);
            if (wvec) {
                reinterpret_cast<float4*>(o + 8 * j)[0] = make_float4(f[0], f[1], f[2], f[3]);
                reinterpret_cast<float4*>(o + 8 * j)[1] = make_float4(f[4], f[5], f[6], f[7]);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) o[8 * j + i] = f[i];
            }
        }
    }
}

// ---- the matrix instruction ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 mx_u4(unsigned a, unsigned b, unsigned c, unsigned d) {
    uint4 v;
    v.x = a; v.y = b; v.z = c; v.w = d;
    return v;
}
// acc += (fp4 slab of 16 weight rows) x (fp8 slab of 16 x rows), the lane's scale bytes in the low byte of sa / sb
__device__ __forceinline__ mx_v4f mx_mfma(const uint4& a, int sa, const uint4& blo, const uint4& bhi, int sb, mx_v4f acc) {
    const mx_v8i av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};  // fp4: the low four registers are the operand
    const mx_v8i bv = {(int)blo.x, (int)blo.y, (int)blo.z, (int)blo.w, (int)bhi.x, (int)bhi.y, (int)bhi.z, (int)bhi.w};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, acc, 4, 0, 0, sa, 0, sb);
}
// lane (r, g) holds rows m0 + r of x against weight rows n0 .. n0 + 3 (n0 = fragment base + 4 g)
__device__ __forceinline__ void mx_store(const mx_v4f& acc, const float* __restrict__ bias, float* __restrict__ y, long long ldy, long long m,
                                         long long n0, int N, int yvec) {
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = bias && n0 + i < N ? acc[i] + bias[n0 + i] : acc[i];
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

template <int MT>
__global__ __launch_bounds__(MX_NT) void quant_mx_gemm_kernel(const unsigned char* __restrict__ xq, const unsigned char* __restrict__ sx, int sxld,
                                                              const unsigned char* __restrict__ qw, const unsigned char* __restrict__ sw,
                                                              const float* __restrict__ bias, float* __restrict__ y, long long ldy, int M, int N,
                                                              int K, int yvec) {
    constexpr int XR = 16 * MT;                        // rows of the x tile
    constexpr int NST = XR * (MX_ST * 8) / MX_NT;      // 16-byte chunks a thread stages per tile: 2 MT
    __shared__ __attribute__((aligned(16))) unsigned char xs[2][XR * MX_LDR];
    __shared__ __attribute__((aligned(16))) unsigned char xe[2][XR * 16];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const long long m0 = (long long)blockIdx.y * XR;
    const long long nbase = (long long)blockIdx.x * MX_NTILE + wave * (MX_NF * 16);
    const int nsl = (K + 127) / 128;                   // slabs
    const int nstage = (nsl + MX_ST - 1) / MX_ST;
    const int spr = K / 32;                            // scale bytes per row
    const unsigned char* wrow[MX_NF];
    const unsigned char* srow[MX_NF];
    bool wrow_on[MX_NF];
#pragma unroll
    for (int f = 0; f < MX_NF; ++f) {
        wrow_on[f] = nbase + 16 * f + r < N;
        const long long n = wrow_on[f] ? nbase + 16 * f + r : 0;
        wrow[f] = qw + n * (K / 2) + 16 * g;
        srow[f] = sw + n * spr + g;
    }

    auto weight_load = [&](int slab, int f, uint4& c, int& e) {
        const bool on = wrow_on[f] && slab * 128 + 32 * g < K;
        c = on ? *reinterpret_cast<const uint4*>(wrow[f] + (long long)slab * 64) : mx_u4(0u, 0u, 0u, 0u);
        e = on ? (int)srow[f][slab * 4] : 127;
    };
    // chunk `idx` of a tile is row idx / 32, bytes 16 (idx % 32) of the stage's 512; thread t < XR also carries row t's 16 scale bytes
    auto stage_load = [&](int stage, uint4 (&st)[NST], uint4& se) {
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int idx = tid + j * MX_NT;
            const long long m = m0 + (idx >> 5);
            const int k = stage * (MX_ST * 128) + 16 * (idx & 31);
            st[j] = m < M && k < K ? *reinterpret_cast<const uint4*>(xq + m * K + k) : mx_u4(0u, 0u, 0u, 0u);
        }
        if (tid < XR) {
            const long long m = m0 + tid;
            const int left = spr - stage * (MX_ST * 4);  // scale bytes of the row from this stage on
            se = m < M && left > 0 ? *reinterpret_cast<const uint4*>(sx + m * sxld + stage * (MX_ST * 4)) : mx_u4(0u, 0u, 0u, 0u);
            unsigned w[4] = {se.x, se.y, se.z, se.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int nv = m < M ? min(max(left - 4 * j, 0), 4) : 0;  // bytes of this dword that are scales of the row
                const unsigned keep = nv == 4 ? 0xffffffffu : (1u << (8 * nv)) - 1u;
                w[j] = (w[j] & keep) | (0x7f7f7f7fu & ~keep);
            }
            se = mx_u4(w[0], w[1], w[2], w[3]);
        }
    };
    auto stage_store = [&](int buf, const uint4 (&st)[NST], const uint4& se) {
#pragma unroll
        for (int j = 0; j < NST; ++j) {
            const int idx = tid + j * MX_NT;
            *reinterpret_cast<uint4*>(&xs[buf][(idx >> 5) * MX_LDR + 16 * (idx & 31)]) = st[j];
        }
        if (tid < XR) *reinterpret_cast<uint4*>(&xe[buf][tid * 16]) = se;
    };

    mx_v4f acc[MX_NF][MT];
#pragma unroll
    for (int f = 0; f < MX_NF; ++f)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[f][t] = mx_v4f{0.f, 0.f, 0.f, 0.f};
    uint4 raw[MX_ST][MX_NF];
    int wsc[MX_ST][MX_NF];
#pragma unroll
    for (int u = 0; u < MX_ST; ++u)
#pragma unroll
        for (int f = 0; f < MX_NF; ++f) weight_load(u, f, raw[u][f], wsc[u][f]);
    {
        uint4 st[NST], se;
        stage_load(0, st, se);
        stage_store(0, st, se);
    }
    __syncthreads();

    for (int s = 0; s < nstage; ++s) {
        uint4 st[NST], se;
        stage_load(s + 1, st, se);  // past K: zeros and 127s, no load
#pragma unroll
        for (int u = 0; u < MX_ST; ++u) {
            const int slab = s * MX_ST + u;
            if (slab < nsl) {  // the whole block
                uint4 a[MX_NF];
                int sa[MX_NF];
#pragma unroll
                for (int f = 0; f < MX_NF; ++f) {
                    a[f] = raw[u][f];
                    sa[f] = wsc[u][f];
                    weight_load(slab + MX_ST, f, raw[u][f], wsc[u][f]);
                }
                const unsigned char* xb = &xs[s & 1][r * MX_LDR + 128 * u + 16 * g];
                const unsigned char* eb = &xe[s & 1][r * 16 + 4 * u + g];
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    const uint4 blo = *reinterpret_cast<const uint4*>(xb + t * 16 * MX_LDR);
                    const uint4 bhi = *reinterpret_cast<const uint4*>(xb + t * 16 * MX_LDR + 64);
                    const int sb = eb[t * 256];
#pragma unroll
                    for (int f = 0; f < MX_NF; ++f) acc[f][t] = mx_mfma(a[f], sa[f], blo, bhi, sb, acc[f][t]);
                }
            }
        }
        stage_store((s + 1) & 1, st, se);
        __syncthreads();
    }

#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const long long m = m0 + 16 * t + r;
        if (m >= M) continue;
#pragma unroll
        for (int f = 0; f < MX_NF; ++f) mx_store(acc[f][t], bias, y, ldy, m, nbase + 16 * f + 4 * g, N, yvec);
    }
}

template <int NF>
__global__ __launch_bounds__(MX_NT) void quant_mx_skinny_kernel(const unsigned char* __restrict__ xq, const unsigned char* __restrict__ sx, int sxld,
                                                                const unsigned char* __restrict__ qw, const unsigned char* __restrict__ sw,
                                                                const float* __restrict__ bias, float* __restrict__ y, long long ldy, int M, int N,
                                                                int K, int yvec) {
    __shared__ mx_v4f part[MX_WAVES][NF][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const long long nbase = (long long)blockIdx.x * (16 * NF);
    const int nsl = (K + 127) / 128;
    const int spr = K / 32;
    const bool xon = r < M;
    const unsigned char* xrow = xq + (long long)(xon ? r : 0) * K + 16 * g;
    const unsigned char* erow = sx + (long long)(xon ? r : 0) * sxld + g;
    const unsigned char* wrow[NF];
    const unsigned char* srow[NF];
    bool wrow_on[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        wrow_on[f] = nbase + 16 * f + r < N;
        const long long n = wrow_on[f] ? nbase + 16 * f + r : 0;
        wrow[f] = qw + n * (K / 2) + 16 * g;
        srow[f] = sw + n * spr + g;
    }
    mx_v4f acc[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) acc[f] = mx_v4f{0.f, 0.f, 0.f, 0.f};

    for (int base = wave; base < nsl; base += MX_WAVES * MX_SKU) {  // the wave's slabs base, base + 8, ...: all loads, then the MFMAs
        uint4 a[MX_SKU][NF], blo[MX_SKU], bhi[MX_SKU];
        int sa[MX_SKU][NF], sb[MX_SKU];
#pragma unroll
        for (int u = 0; u < MX_SKU; ++u) {
            const int slab = base + MX_WAVES * u;
            const bool kon = slab * 128 + 32 * g < K;  // false for every slab past the last
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const bool on = kon && wrow_on[f];
                a[u][f] = on ? *reinterpret_cast<const uint4*>(wrow[f] + (long long)slab * 64) : mx_u4(0u, 0u, 0u, 0u);
                sa[u][f] = on ? (int)srow[f][slab * 4] : 127;
            }
            blo[u] = xon && slab * 128 + 16 * g < K ? *reinterpret_cast<const uint4*>(xrow + (long long)slab * 128) : mx_u4(0u, 0u, 0u, 0u);
            bhi[u] = xon && slab * 128 + 64 + 16 * g < K ? *reinterpret_cast<const uint4*>(xrow + (long long)slab * 128 + 64) : mx_u4(0u, 0u, 0u, 0u);
            sb[u] = xon && kon ? (int)erow[slab * 4] : 127;
        }
#pragma unroll
        for (int u = 0; u < MX_SKU; ++u)
            if (base + MX_WAVES * u < nsl) {  // the whole wave
#pragma unroll
                for (int f = 0; f < NF; ++f) acc[f] = mx_mfma(a[u][f], sa[u][f], blo[u], bhi[u], sb[u], acc[f]);
            }
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) part[wave][f][lane] = acc[f];
    __syncthreads();
    if (wave < NF && xon) {  // wave f adds fragment f's partial sums, wave 0 first
        mx_v4f sum = part[0][wave][lane];
#pragma unroll
        for (int w = 1; w < MX_WAVES; ++w) sum += part[w][wave][lane];
        mx_store(sum, bias, y, ldy, r, nbase + 16 * wave + 4 * g, N, yvec);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
bool mx_format(long long N, long long K) { return N > 0 && K > 0 && N <= 0x7fffffffLL && K <= (1LL << 30) && K % 32 == 0; }

int mx_check(const char* who, int N, int K) {
    NK_CHECK(N > 0 && K > 0, "%s: N = %d, K = %d", who, N, K);
    NK_CHECK(K % 32 == 0, "%s: K = %d must be a multiple of the MX block (32)", who, K);
    NK_CHECK(K <= (1 << 30), "%s: K = %d is beyond this path (2^30)", who, K);
    return NK_OK;
}

// rows of W (row stride ldw) -> codes q and scale bytes s (row stride lds bytes): the pack (fp4) and the row quantiser (fp8)
template <bool FP4>
int mx_quantise(nk_device* dev, const char* who, const float* W, long long ldw, unsigned char* q, unsigned char* s, long long lds, int N, int K) {
    const long long blocks = ((long long)N * ((K + 255) / 256) + 3) / 4;
    NK_CHECK(blocks <= 0x7fffffffLL, "%s: %d rows of K = %d are beyond one launch", who, N, K);
    const int wvec = al16(W) && ldw % 4 == 0;
    hipLaunchKernelGGL(quant_mx_kernel<FP4>, dim3((unsigned)blocks), dim3(256), 0, dev->compute, W, ldw, q, s, lds, (long long)N, K, wvec);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // namespace

extern "C" {

size_t nk_quant_mx_words(int N, int K) { return mx_format(N, K) ? (size_t)N * (size_t)K / 8 : 0; }
size_t nk_quant_mx_scales(int N, int K) { return mx_format(N, K) ? ((size_t)N * (size_t)(K / 32) + 3) / 4 : 0; }

int nk_quant_mx_pack(nk_device* dev, const float* W, int ldw, float* qw, float* sw, int N, int K) {
    NK_USE(dev);
    if (int rc = mx_check("nk_quant_mx_pack", N, K)) return rc;
    NK_CHECK(W && qw && sw, "null pointer in nk_quant_mx_pack");
    NK_CHECK(ldw >= K, "nk_quant_mx_pack: ldw = %d < K = %d", ldw, K);
    NK_CHECK(al16(qw), "nk_quant_mx_pack: qw must be 16-byte aligned");
    return mx_quantise<true>(dev, "nk_quant_mx_pack", W, ldw, reinterpret_cast<unsigned char*>(qw), reinterpret_cast<unsigned char*>(sw), K / 32, N, K);
}

int nk_quant_mx_unpack(nk_device* dev, const float* qw, const float* sw, float* W, int ldw, int N, int K) {
    NK_USE(dev);
    if (int rc = mx_check("nk_quant_mx_unpack", N, K)) return rc;
    NK_CHECK(W && qw && sw, "null pointer in nk_quant_mx_unpack");
    NK_CHECK(ldw >= K, "nk_quant_mx_unpack: ldw = %d < K = %d", ldw, K);
    NK_CHECK(al16(qw), "nk_quant_mx_unpack: qw must be 16-byte aligned");
    const int wvec = al16(W) && ldw % 4 == 0;
    hipLaunchKernelGGL(quant_mx_unpack_kernel, dim3(nk_stream_grid((size_t)N * (size_t)(K / 32), 256)), dim3(256), 0, dev->compute,
                       reinterpret_cast<const uint4*>(qw), reinterpret_cast<const unsigned char*>(sw), W, (long long)ldw, (long long)N, K, wvec);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int nk_quant_mx_rows(nk_device* dev, const float* x, int ldx, float* xq, float* sx, int M, int K) {
    NK_USE(dev);
    if (int rc = mx_check("nk_quant_mx_rows", M, K)) return rc;
    NK_CHECK(x && xq && sx, "null pointer in nk_quant_mx_rows");
    NK_CHECK(ldx >= K, "nk_quant_mx_rows: ldx = %d < K = %d", ldx, K);
    NK_CHECK(al16(xq), "nk_quant_mx_rows: xq must be 16-byte aligned");
    return mx_quantise<false>(dev, "nk_quant_mx_rows", x, ldx, reinterpret_cast<unsigned char*>(xq), reinterpret_cast<unsigned char*>(sx), K / 32, M, K);
}

int nk_quant_mx_linear_fwd(nk_device* dev, const float* x, int ldx, const float* qw, const float* sw, const float* bias, float* y, int ldy, int M,
                           int N, int K) {
    NK_USE(dev);
    if (int rc = mx_check("nk_quant_mx_linear_fwd", N, K)) return rc;
    NK_CHECK(M >= 0, "nk_quant_mx_linear_fwd: M = %d", M);
    NK_CHECK(x && qw && sw && y, "null pointer in nk_quant_mx_linear_fwd (only bias may be NULL)");
    NK_CHECK(ldx >= K && ldy >= N, "nk_quant_mx_linear_fwd: ldx = %d < K = %d or ldy = %d < N = %d", ldx, K, ldy, N);
    NK_CHECK(al16(qw), "nk_quant_mx_linear_fwd: qw must be 16-byte aligned");
    NK_CHECK((M + 127) / 128 <= 65535, "nk_quant_mx_linear_fwd: M = %d is beyond one launch", M);
    if (M == 0) return NK_OK;
    const int sxld = (K / 32 + 15) & ~15;  // scale bytes per row of the image, padded for 16-byte loads
    void* ws = nullptr;
    if (int rc = nk_workspace(dev, (size_t)M * (size_t)K + (size_t)M * (size_t)sxld, &ws)) return rc;
    unsigned char* xq = reinterpret_cast<unsigned char*>(ws);
    unsigned char* sx = xq + (size_t)M * (size_t)K;  // M * K is a multiple of 32
    if (int rc = mx_quantise<false>(dev, "nk_quant_mx_linear_fwd", x, ldx, xq, sx, sxld, M, K)) return rc;
    if (int rc = nk_prof_start(dev, NK_KERNEL_QUANT_MX, 2.0 * M * N * (double)K)) return rc;
    const unsigned char* q = reinterpret_cast<const unsigned char*>(qw);
    const unsigned char* s = reinterpret_cast<const unsigned char*>(sw);
    const int yvec = al16(y) && ldy % 4 == 0;
#define NK_MX(KERNEL, GRID) hipLaunchKernelGGL(KERNEL, GRID, dim3(MX_NT), 0, dev->compute, xq, sx, sxld, q, s, bias, y, (long long)ldy, M, N, K, yvec)
    if (M <= 16) {
        if (N >= MX_SK_WIDE_N) NK_MX(quant_mx_skinny_kernel<2>, dim3((unsigned)((N + 31) / 32)));
        else NK_MX(quant_mx_skinny_kernel<1>, dim3((unsigned)((N + 15) / 16)));
    } else {
        const int mt = M <= 32 ? 2 : M <= 64 ? 4 : 8;
        const dim3 grid((unsigned)((N + MX_NTILE - 1) / MX_NTILE), (unsigned)((M + 16 * mt - 1) / (16 * mt)));
        if (mt == 2) NK_MX(quant_mx_gemm_kernel<2>, grid);
        else if (mt == 4) NK_MX(quant_mx_gemm_kernel<4>, grid);
        else NK_MX(quant_mx_gemm_kernel<8>, grid);
    }
#undef NK_MX
    NK_LAUNCH_CHECK();
    return nk_prof_stop(dev);
}

}  // extern "C"
