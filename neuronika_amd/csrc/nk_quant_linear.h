// Weight-only quantised Linear (ours; the reference has no such layer; format and semantics in include/neuronika_hip.h): int8 / int4
// weights with per-group f32 scales, f32 activations and accumulation.  Included ONCE, by nk_norm.hip.  Kernels and entry points of
// nk_quant_linear_*.
//   quant_pack_kernel       group in {32, 64, 128}: a wave owns 256 consecutive elements of one row (a float4 per lane), the absmax of a
//                           group is an xor-shuffle maximum over its group / 4 lanes, the quantised quads of 4 (int8) or 8 (int4) lanes
//                           are gathered by shuffles into one 16-byte store
//   quant_pack_row_kernel   group 0: a block per row, the absmax over the row first (block maximum), then the same quantise-and-store
//                           walk over the row, which the first pass left in the cache
//   quant_unpack_kernel     a 16-byte chunk (16 int8 / 32 int4 elements) per thread -> 4 / 8 float4 stores (scalar stores when W or
//                           ldw break the alignment)
//   quant_linear_rows_kernel<BITS, ROWS>   y[m][n] = bias[n] + sum_k x[m][k] * w^[n][k] for ROWS <= 8 rows of x in ONE pass over the
//                           weights.  A wave owns QL_NW = 4 weight rows, a block of four waves 16.  Row n is K * BITS / 128 chunks of 16
//                           bytes; lane l takes chunks l, l + 64, l + 128, ... - a function of (BITS, K) alone - straight from
//                           global memory into registers, QL_U chunks of each of the wave's rows issued before the first is used.  x
//                           is read through the caches (the four waves of a block walk the same columns together) and every fragment of
//                           it serves the wave's four weight rows.
//     the sum  A chunk is one (int8) or two (int4) UNITS of 16 consecutive k, each inside one scale group.  Per unit, per (m, n):
//                  p = fma(x[k+15], q[k+15], ... fma(x[k], q[k], 0))        ascending k, q = float(integer weight), exact
//                  acc = fma(s, p, acc)                                     s the group's scale
//              i.e. the scale is applied per unit: acc += s * sum_unit(x * float(q)).  A lane walks its units in ascending k; the 64
//              lane sums meet in the xor-shuffle butterfly of nk_wave_sum (offsets 32, 16, ... 1); y = sum + bias[n] (sum alone
//              without a bias).  No split of K beyond the lanes, no workspace, no atomics, nothing allocated: capturable.
//     bits     the chain of y[m][n] holds x[m, :], row n of the weights and scales, bias[n] and (bits, group, K) and nothing else:
//              not M, N, the other rows, ldx / ldy, the alignment of x (16-byte or scalar loads of the same values), ROWS or the
//              weight row's slot in its wave.  Rows past N re-read row N - 1 and are not stored.
//   many rows  quant_unpack into the device's operand scratch, then the f32 GEMM: nk_linear_fwd itself for contiguous x / y with a bias
//              (its bits exactly), else nk_sgemm with the strides followed by quant_bias_rows_kernel.
// The switch between the two is a function of (M, bits): rows path for M <= L(bits) (QL_RULE_*, measured: DESIGN.md), in
// ceil(M / 8) passes; NK_TUNE_QUANT_ROWS overrides L.

namespace {

constexpr int QL_NW = 4;     // weight rows per wave
constexpr int QL_WAVES = 4;  // waves per block
constexpr int QL_R = 8;      // rows of x per pass
constexpr int QL_U = 2;      // chunks per weight row in flight per lane
constexpr int QL_RULE_8 = 8, QL_RULE_4 = 8;  // L(bits): rows path up to this M

__device__ __forceinline__ float ql_div(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}
__device__ __forceinline__ float ql_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// The 16 integer weights of unit `u` of a 16-byte chunk, as floats (exact).  int8: two's-complement bytes, the chunk is one unit.
// int4: nibble q + 8, element k in byte k / 2, even k low; words (x, y) are unit 0, (z, w) unit 1.
template <int BITS>
__device__ __forceinline__ void ql_unit(const uint4& c, int u, float (&q)[16]) {
    if (BITS == 8) {
        const unsigned w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) q[4 * j + b] = (float)(int)(signed char)(w[j] >> (8 * b));
    } else {
        const unsigned w[2] = {u ? c.z : c.x, u ? c.w : c.y};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned lo = w[j] & 0x0f0f0f0fu, hi = (w[j] >> 4) & 0x0f0f0f0fu;  // even and odd elements, a byte each
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                q[8 * j + 2 * b] = (float)((lo >> (8 * b)) & 0xffu) - 8.f;
                q[8 * j + 2 * b + 1] = (float)((hi >> (8 * b)) & 0xffu) - 8.f;
            }
        }
    }
}

__device__ __forceinline__ float4 ql_load4(const float* __restrict__ p, bool vec) {
    return vec ? *reinterpret_cast<const float4*>(p) : make_float4(p[0], p[1], p[2], p[3]);
}

// the four integer weights k = 16 u + 4 j .. + 3 of a chunk (j = 0 .. 3), as floats: ql_unit's values, four at a time
template <int BITS>
__device__ __forceinline__ void ql_quad(const uint4& c, int u, int j, float (&q)[4]) {
    if (BITS == 8) {
        const unsigned w = j == 0 ? c.x : j == 1 ? c.y : j == 2 ? c.z : c.w;
#pragma unroll
        for (int b = 0; b < 4; ++b) q[b] = (float)(int)(signed char)(w >> (8 * b));
    } else {
        const unsigned w = u ? (j < 2 ? c.z : c.w) : (j < 2 ? c.x : c.y);
        const unsigned lo = w & 0x0f0f0f0fu, hi = (w >> 4) & 0x0f0f0f0fu;  // even and odd elements, a byte each
        const int b0 = (j & 1) * 2;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            q[2 * b] = (float)((lo >> (8 * (b0 + b))) & 0xffu) - 8.f;
            q[2 * b + 1] = (float)((hi >> (8 * (b0 + b))) & 0xffu) - 8.f;
        }
    }
}

// chunk c of the wave's QL_NW weight rows against ROWS rows of x: four k at a time, ascending, so that only a float4 of every x
// row and four weights of every weight row are live beside the sums
template <int BITS, int ROWS>
__device__ __forceinline__ void ql_chunk(float (&acc)[ROWS][QL_NW], const uint4 (&raw)[QL_NW], const float* const (&srow)[QL_NW],
                                         const float* __restrict__ x, long long ldx, int c, int gshift, bool xvec) {
    constexpr int EPC = 128 / BITS;
    const int k0 = c * EPC;
    float s[QL_NW];
#pragma unroll
    for (int w = 0; w < QL_NW; ++w) s[w] = srow[w][k0 >> gshift];
#pragma unroll
    for (int u = 0; u < EPC / 16; ++u) {
        float p[ROWS][QL_NW];
#pragma unroll
        for (int m = 0; m < ROWS; ++m)
#pragma unroll
            for (int w = 0; w < QL_NW; ++w) p[m][w] = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float q[QL_NW][4];
#pragma unroll
            for (int w = 0; w < QL_NW; ++w) ql_quad<BITS>(raw[w], u, j, q[w]);
#pragma unroll
            for (int m = 0; m < ROWS; ++m) {
                const float4 xv = ql_load4(x + m * ldx + k0 + 16 * u + 4 * j, xvec);
#pragma unroll
                for (int w = 0; w < QL_NW; ++w)
                    p[m][w] = fmaf(xv.w, q[w][3], fmaf(xv.z, q[w][2], fmaf(xv.y, q[w][1], fmaf(xv.x, q[w][0], p[m][w]))));
            }
        }
#pragma unroll
        for (int m = 0; m < ROWS; ++m)
#pragma unroll
            for (int w = 0; w < QL_NW; ++w) acc[m][w] = fmaf(s[w], p[m][w], acc[m][w]);
    }
}

template <int BITS, int ROWS>
__global__ __launch_bounds__(256) void quant_linear_rows_kernel(const float* __restrict__ x, long long ldx, const uint4* __restrict__ qw,
                                                                const float* __restrict__ scales, const float* __restrict__ bias,
                                                                float* __restrict__ y, long long ldy, int N, int K, int gshift, int xvec) {
    constexpr int EPC = 128 / BITS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n0 = ((long long)blockIdx.x * QL_WAVES + wave) * QL_NW;
    if (n0 >= N) return;  // the whole wave; the kernel has no barrier
    const int nch = K / EPC;                        // chunks per weight row
    const int spr = gshift < 31 ? K >> gshift : 1;  // scales per weight row
    const uint4* wrow[QL_NW];
    const float* srow[QL_NW];
#pragma unroll
    for (int w = 0; w < QL_NW; ++w) {
        const long long n = n0 + w < N ? n0 + w : N - 1;
        wrow[w] = qw + n * nch;
        srow[w] = scales + n * spr;
    }
    float acc[ROWS][QL_NW];
#pragma unroll
    for (int m = 0; m < ROWS; ++m)
#pragma unroll
        for (int w = 0; w < QL_NW; ++w) acc[m][w] = 0.f;
    int i = 0;
    for (; (i + QL_U) * 64 <= nch; i += QL_U) {  // every lane holds QL_U chunks of each row
        uint4 raw[QL_U][QL_NW];
#pragma unroll
        for (int u = 0; u < QL_U; ++u)
#pragma unroll
            for (int w = 0; w < QL_NW; ++w) raw[u][w] = wrow[w][(i + u) * 64 + lane];
#pragma unroll
        for (int u = 0; u < QL_U; ++u) ql_chunk<BITS, ROWS>(acc, raw[u], srow, x, ldx, (i + u) * 64 + lane, gshift, xvec != 0);
    }
    for (; i * 64 < nch; ++i) {
        const int c = i * 64 + lane;
        if (c < nch) {
            uint4 raw[QL_NW];
#pragma unroll
            for (int w = 0; w < QL_NW; ++w) raw[w] = wrow[w][c];
            ql_chunk<BITS, ROWS>(acc, raw, srow, x, ldx, c, gshift, xvec != 0);
        }
    }
#pragma unroll
    for (int m = 0; m < ROWS; ++m)
#pragma unroll
        for (int w = 0; w < QL_NW; ++w) {
            const float s = nk_wave_sum(acc[m][w]);
            if (lane == m * QL_NW + w && n0 + w < N) y[m * ldy + n0 + w] = bias ? s + bias[n0 + w] : s;
        }
}

// ---- pack ------------------------------------------------------------------------------------------------------------------------
// the quad's four integers: bytes (int8) or nibbles q + 8 (int4) from bit 0 up
template <int BITS>
__device__ __forceinline__ unsigned ql_quant4(const float4& v, float s) {
    constexpr float QM = BITS == 8 ? 127.f : 7.f;
    const float e[4] = {v.x, v.y, v.z, v.w};
    unsigned out = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float r = s == 0.f ? 0.f : rintf(ql_div(e[j], s));
        r = fminf(fmaxf(r, -QM), QM);  // a NaN leaves as -QM
        const int q = (int)r;
        out |= BITS == 8 ? (unsigned)(q & 0xff) << (8 * j) : (unsigned)(q + 8) << (4 * j);
    }
    return out;
}
// Every lane of the wave calls this: the quads of 4 (int8) or 8 (int4) neighbouring lanes leave in one 16-byte store by the first
// of them.  `k` is the quad's first element in the row, `row` the row's packed bytes; lanes with !on hold nothing.
template <int BITS>
__device__ __forceinline__ void ql_store_quads(unsigned char* __restrict__ row, int k, unsigned word, bool on) {
    const int lane = threadIdx.x & 63;
    if (BITS == 8) {
        const unsigned w1 = __shfl_down(word, 1, 64), w2 = __shfl_down(word, 2, 64), w3 = __shfl_down(word, 3, 64);
        if (on && (lane & 3) == 0) *reinterpret_cast<uint4*>(row + k) = make_uint4(word, w1, w2, w3);
    } else {
        const unsigned h = word | (__shfl_down(word, 1, 64) << 16);  // two quads, at the even lanes
        const unsigned w1 = __shfl_down(h, 2, 64), w2 = __shfl_down(h, 4, 64), w3 = __shfl_down(h, 6, 64);
        if (on && (lane & 7) == 0) *reinterpret_cast<uint4*>(row + k / 2) = make_uint4(h, w1, w2, w3);
    }
}
__device__ __forceinline__ float ql_absmax4(const float4& v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }

template <int BITS>
__global__ __launch_bounds__(256) void quant_pack_kernel(const float* __restrict__ W, long long ldw, unsigned char* __restrict__ qw,
                                                         float* __restrict__ scales, int N, int K, int group, int wvec) {
    const int lane = threadIdx.x & 63;
    const int cpr = (K + 255) / 256;  // wave spans per row
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long long)N * cpr) return;  // the whole wave
    const long long n = wid / cpr;
    const int k = (int)(wid - n * cpr) * 256 + lane * 4;
    const bool on = k < K;  // a group lies wholly below K or wholly beyond it
    const float4 v = on ? ql_load4(W + n * ldw + k, wvec != 0) : make_float4(0.f, 0.f, 0.f, 0.f);
    float a = ql_absmax4(v);
    for (int off = 1; off < group / 4; off <<= 1) a = fmaxf(a, __shfl_xor(a, off, 64));
    const float s = ql_div(a, BITS == 8 ? 127.f : 7.f);
    if (on && k % group == 0) scales[n * (K / group) + k / group] = s;
    ql_store_quads<BITS>(qw + n * ((long long)K * BITS / 8), k, ql_quant4<BITS>(v, s), on);
}

template <int BITS>
__global__ __launch_bounds__(256) void quant_pack_row_kernel(const float* __restrict__ W, long long ldw, unsigned char* __restrict__ qw,
                                                             float* __restrict__ scales, int N, int K, int wvec) {
    __shared__ float red[4];
    for (long long n = blockIdx.x; n < N; n += gridDim.x) {
        const float* w = W + n * ldw;
        float a = 0.f;
        for (int k = threadIdx.x * 4; k < K; k += 1024) a = fmaxf(a, ql_absmax4(ql_load4(w + k, wvec != 0)));
        a = nk_block_max<256>(a, red);
        const float s = ql_div(a, BITS == 8 ? 127.f : 7.f);
        if (threadIdx.x == 0) scales[n] = s;
        for (int base = 0; base < K; base += 1024) {
            const int k = base + threadIdx.x * 4;
            const bool on = k < K;
            const float4 v = on ? ql_load4(w + k, wvec != 0) : make_float4(0.f, 0.f, 0.f, 0.f);
            ql_store_quads<BITS>(qw + n * ((long long)K * BITS / 8), k, ql_quant4<BITS>(v, s), on);
        }
    }
}

// ---- unpack ----------------------------------------------------------------------------------------------------------------------
template <int BITS>
__global__ __launch_bounds__(256) void quant_unpack_kernel(const uint4* __restrict__ qw, const float* __restrict__ scales,
                                                           float* __restrict__ W, long long ldw, int N, int K, int gshift, int wvec) {
    constexpr int EPC = 128 / BITS;
    const int nch = K / EPC;
    const int spr = gshift < 31 ? K >> gshift : 1;
    const long long total = (long long)N * nch;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long n = t / nch;
        const int k0 = (int)(t - n * nch) * EPC;
        const uint4 raw = qw[t];
        const float s = scales[n * spr + (k0 >> gshift)];
        float* o = W + n * ldw + k0;
#pragma unroll
        for (int u = 0; u < EPC / 16; ++u) {
            float q[16];
            ql_unit<BITS>(raw, u, q);
#pragma unroll
            for (int j = 0; j < 16; ++j) q[j] = ql_mul(q[j], s);
            if (wvec) {
#pragma unroll
                for (int j = 0; j < 4; ++j) reinterpret_cast<float4*>(o + 16 * u)[j] = make_float4(q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3]);
            } else {
#pragma unroll
                for (int j = 0; j < 16; ++j) o[16 * u + j] = q[j];
            }
        }
    }
}

// y[m][n] += bias[n]: the many-row path when the GEMM had to follow ldx / ldy
__global__ __launch_bounds__(256) void quant_bias_rows_kernel(float* __restrict__ y, long long ldy, const float* __restrict__ bias, int M, int N) {
    const long long total = (long long)M * N;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long m = t / N;
        const int n = (int)(t - m * N);
        y[m * ldy + n] += bias[n];
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
bool ql_format(long long N, long long K, int bits, int group) {
    return N > 0 && K > 0 && N <= 0x7fffffffLL && K <= 0x7fffffffLL && (bits == 8 || bits == 4) && K % 32 == 0 &&
           (group == 0 || ((group == 32 || group == 64 || group == 128) && K % group == 0));
}
int ql_gshift(int group) { return group == 32 ? 5 : group == 64 ? 6 : group == 128 ? 7 : 31; }

int ql_check(const char* who, int N, int K, int bits, int group) {
    NK_CHECK(N > 0 && K > 0, "%s: N = %d, K = %d", who, N, K);
    NK_CHECK(bits == 8 || bits == 4, "%s: bits = %d (8 or 4)", who, bits);
    NK_CHECK(group == 0 || group == 32 || group == 64 || group == 128, "%s: group = %d (32, 64, 128, or 0 for one group per row)", who, group);
    NK_CHECK(K % 32 == 0 && (group == 0 || K % group == 0), "%s: K = %d must be a multiple of 32 and of the group (%d)", who, K, group);
    return NK_OK;
}

template <int BITS>
void ql_launch_rows(nk_device* dev, int rows, const float* x, long long ldx, const uint4* qw, const float* scales, const float* bias, float* y,
                    long long ldy, int N, int K, int gshift, int xvec) {
    const dim3 grid((unsigned)((N + QL_WAVES * QL_NW - 1) / (QL_WAVES * QL_NW)));
#define NK_QL_ROWS(R) \
    case R: hipLaunchKernelGGL((quant_linear_rows_kernel<BITS, R>), grid, dim3(256), 0, dev->compute, x, ldx, qw, scales, bias, y, ldy, N, K, gshift, xvec); break
    switch (rows) {
        NK_QL_ROWS(1); NK_QL_ROWS(2); NK_QL_ROWS(3); NK_QL_ROWS(4); NK_QL_ROWS(5); NK_QL_ROWS(6); NK_QL_ROWS(7); NK_QL_ROWS(8);
    }
#undef NK_QL_ROWS
}

int ql_unpack(nk_device* dev, const float* qw, const float* scales, float* W, long long ldw, int N, int K, int bits, int group) {
    const long long chunks = (long long)N * (K / (128 / bits));
    const int grid = nk_stream_grid((size_t)chunks, 256);
    const int wvec = al16(W) && ldw % 4 == 0;
    if (bits == 8)
        hipLaunchKernelGGL(quant_unpack_kernel<8>, dim3(grid), dim3(256), 0, dev->compute, reinterpret_cast<const uint4*>(qw), scales, W, ldw, N, K, ql_gshift(group), wvec);
    else
        hipLaunchKernelGGL(quant_unpack_kernel<4>, dim3(grid), dim3(256), 0, dev->compute, reinterpret_cast<const uint4*>(qw), scales, W, ldw, N, K, ql_gshift(group), wvec);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // namespace

extern "C" {

size_t nk_quant_linear_words(int N, int K, int bits) { return ql_format(N, K, bits, 0) ? (size_t)N * (size_t)K * (size_t)bits / 32 : 0; }
size_t nk_quant_linear_scales(int N, int K, int group) {
    return ql_format(N, K, 8, group) ? (size_t)N * (size_t)(group ? K / group : 1) : 0;
}
int nk_quant_linear_rows_rule(int bits) { return bits == 8 ? QL_RULE_8 : bits == 4 ? QL_RULE_4 : 0; }

int nk_quant_linear_pack(nk_device* dev, const float* W, int ldw, float* qw, float* scales, int N, int K, int bits, int group) {
    NK_USE(dev);
    if (int rc = ql_check("nk_quant_linear_pack", N, K, bits, group)) return rc;
    NK_CHECK(W && qw && scales, "null pointer in nk_quant_linear_pack");
    NK_CHECK(ldw >= K, "nk_quant_linear_pack: ldw = %d < K = %d", ldw, K);
    NK_CHECK(al16(qw), "nk_quant_linear_pack: qw must be 16-byte aligned");
    const int wvec = al16(W) && ldw % 4 == 0;
    unsigned char* q = reinterpret_cast<unsigned char*>(qw);
    if (group > 0) {
        const long long waves = (long long)N * ((K + 255) / 256);
        NK_CHECK((waves + 3) / 4 <= 0x7fffffffLL, "nk_quant_linear_pack: N = %d, K = %d is beyond one launch", N, K);
        const dim3 grid((unsigned)((waves + 3) / 4));
        if (bits == 8) hipLaunchKernelGGL(quant_pack_kernel<8>, grid, dim3(256), 0, dev->compute, W, (long long)ldw, q, scales, N, K, group, wvec);
        else hipLaunchKernelGGL(quant_pack_kernel<4>, grid, dim3(256), 0, dev->compute, W, (long long)ldw, q, scales, N, K, group, wvec);
    } else {
        const dim3 grid(row_grid(N, 1));
        if (bits == 8) hipLaunchKernelGGL(quant_pack_row_kernel<8>, grid, dim3(256), 0, dev->compute, W, (long long)ldw, q, scales, N, K, wvec);
        else hipLaunchKernelGGL(quant_pack_row_kernel<4>, grid, dim3(256), 0, dev->compute, W, (long long)ldw, q, scales, N, K, wvec);
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int nk_quant_linear_unpack(nk_device* dev, const float* qw, const float* scales, float* W, int ldw, int N, int K, int bits, int group) {
    NK_USE(dev);
    if (int rc = ql_check("nk_quant_linear_unpack", N, K, bits, group)) return rc;
    NK_CHECK(W && qw && scales, "null pointer in nk_quant_linear_unpack");
    NK_CHECK(ldw >= K, "nk_quant_linear_unpack: ldw = %d < K = %d", ldw, K);
    NK_CHECK(al16(qw), "nk_quant_linear_unpack: qw must be 16-byte aligned");
    return ql_unpack(dev, qw, scales, W, ldw, N, K, bits, group);
}

int nk_quant_linear_fwd(nk_device* dev, const float* x, int ldx, const float* qw, const float* scales, const float* bias, float* y, int ldy,
                        int M, int N, int K, int bits, int group) {
    NK_USE(dev);
    if (int rc = ql_check("nk_quant_linear_fwd", N, K, bits, group)) return rc;
    NK_CHECK(M >= 0, "nk_quant_linear_fwd: M = %d", M);
    NK_CHECK(x && qw && scales && y, "null pointer in nk_quant_linear_fwd (only bias may be NULL)");
    NK_CHECK(ldx >= K && ldy >= N, "nk_quant_linear_fwd: ldx = %d < K = %d or ldy = %d < N = %d", ldx, K, ldy, N);
    NK_CHECK(al16(qw), "nk_quant_linear_fwd: qw must be 16-byte aligned");
    if (M == 0) return NK_OK;
    const int L = dev->tune_quant_rows >= 0 ? dev->tune_quant_rows : nk_quant_linear_rows_rule(bits);
    if (M <= L) {
        const int xvec = al16(x) && ldx % 4 == 0;
        for (int m0 = 0; m0 < M; m0 += QL_R) {
            const int rows = M - m0 < QL_R ? M - m0 : QL_R;
            const float* xp = x + (long long)m0 * ldx;
            float* yp = y + (long long)m0 * ldy;
            if (bits == 8) ql_launch_rows<8>(dev, rows, xp, ldx, reinterpret_cast<const uint4*>(qw), scales, bias, yp, ldy, N, K, ql_gshift(group), xvec);
            else ql_launch_rows<4>(dev, rows, xp, ldx, reinterpret_cast<const uint4*>(qw), scales, bias, yp, ldy, N, K, ql_gshift(group), xvec);
            NK_LAUNCH_CHECK();
        }
        return NK_OK;
    }
    void* wd = nullptr;
    if (int rc = nk_operand_scratch(dev, (size_t)N * (size_t)K * sizeof(float), &wd)) return rc;
    if (int rc = ql_unpack(dev, qw, scales, (float*)wd, K, N, K, bits, group)) return rc;
    if (bias && ldx == K && ldy == N) return nk_linear_fwd(dev, x, (const float*)wd, bias, y, M, K, N);
    if (int rc = nk_sgemm(dev, 0, 1, M, N, K, 1.f, x, ldx, (const float*)wd, K, 0.f, y, ldy)) return rc;
    if (bias) {
        hipLaunchKernelGGL(quant_bias_rows_kernel, dim3(nk_stream_grid((size_t)M * N, 256)), dim3(256), 0, dev->compute, y, (long long)ldy, bias, M, N);
        NK_LAUNCH_CHECK();
    }
    return NK_OK;
}

}  // extern "C"
