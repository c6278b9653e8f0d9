// Incremental decoding (ours; semantics in include/neuronika_hip.h): the key / value cache of a causal attention layer and the
// single-query attention over it.  Included by nk_norm.hip, the row-kernel unit.  Memory-bound, no MFMA: one query row reads its
// n cached keys and values once, 2 n dh 4 bytes, straight into registers with 16-byte loads (no LDS staging: nothing is shared
// between waves, cdna_hip_programming.md "GEMV / M <= 16").
//   append    a transposing copy (B*T, H*dh) rows -> (B, H, cap, dh), K and V in one launch; 16-byte accesses where dh % 4 == 0 and
//             the strides / pointers allow it (T = float4), scalar otherwise (T = float).  Positions >= cap are dropped.
//   partial   one 256-thread block per (problem (b, t, h), chunk of ADEC_CHUNK keys).  The chunk size is a compile-time constant
//             of the dh instantiation - never a function of the CU count, B, H, T, cap or a tuning knob - so the summation order
//             of a problem depends on its own length alone.  A group of dh / 4 lanes owns a key: 16-byte loads, a partial dot of
//             four elements per lane, xor-shuffles inside the group.  A group owns keys g, g + G, g + 2G ... of the chunk (the
//             block reads G consecutive keys = 4 KiB per step), ADEC_KPG = 16 of them; the source issues all 16 key loads and
//             all 16 value loads before the first use - the intent; the compiler settles on 108 VGPRs, so it does not keep all
//             32 float4 live and orders some loads later.  The same group then owns the same keys' values.  The chunk's shift
//             is its exact maximum, so nothing is rescaled inside a chunk.  Keys >= n: the load is redirected to key n - 1 (never a read past the problem's own rows, never a value
//             of the uninitialised tail in a register) and the probability is SELECTED to 0, not multiplied.
//             A problem of one chunk writes O directly; otherwise (m, l, unnormalised o[dh]) go to the workspace.
//   combine   one thread per (problem, column): the problem's partials in chunk order, in the exp2 form of the fused core -
//             M = max m_c, O = sum_c o_c exp2(m_c - M), L = sum_c l_c exp2(m_c - M), O / L.  No atomics, no arrival order.
//   generic   any other dh (dh % 4 != 0 included): scalar accesses, a chunk of 256 keys, groups of lpk = the power of two >= dh
//             (64 at most) lanes per key; scores and probabilities through LDS, columns in blocks of lpk.
#pragma once
#include "nk_common.h"

namespace {

constexpr int ADEC_THREADS = 256;
constexpr int ADEC_KPG = 16;             // keys per lane group and chunk in the vector instantiations: 16 + 16 float4 loads per lane
constexpr int ADEC_CHUNK_GENERIC = 256;  // one key per thread in the generic kernel's softmax
constexpr float ADEC_LOG2E = 1.44269504088896341f;

// keys per chunk: part of the summation order, a constant of the library per head size
constexpr int adec_chunk_of(int dh) {
    return dh == 32 || dh == 64 || dh == 128 ? (ADEC_THREADS / (dh / 4)) * ADEC_KPG : ADEC_CHUNK_GENERIC;
}
bool adec_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Row b*T + t of K / V -> position start[b] + t of every head of sample b.  DV = dh in units of T, ldv = the row stride in units of T.
template <typename T>
__global__ void __launch_bounds__(256) kv_append_kernel(T* __restrict__ Kc, T* __restrict__ Vc, const T* __restrict__ K, const T* __restrict__ V,
                                                        long long ldv, const int* __restrict__ start, int Tn, int H, int DV, int cap,
                                                        long long total) {
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const int q = (int)(i % DV);
        const long long rh = i / DV;
        const int h = (int)(rh % H);
        const long long row = rh / H;
        const int b = (int)(row / Tn), t = (int)(row % Tn);
        const long long pos = (long long)start[b] + t;
        if (pos < 0 || pos >= cap) continue;
        const size_t src = (size_t)row * ldv + (size_t)h * DV + q;
        const size_t dst = (((size_t)b * H + h) * cap + (size_t)pos) * DV + q;
        const T kv = K[src], vv = V[src];
        Kc[dst] = kv;
        Vc[dst] = vv;
    }
}

// keys query (b, t) reads: min(start[b] + t + 1, cap); <= 0 for a negative start (the output row is then 0)
__device__ __forceinline__ int adec_len(const int* __restrict__ start, int b, int t, int cap) {
    const long long n = (long long)start[b] + t + 1;
    return n > cap ? cap : (n < 0 ? 0 : (int)n);
}

template <int DH>
__global__ void __launch_bounds__(ADEC_THREADS) adec_partial_kernel(const float* __restrict__ Q, int ldq, const float4* __restrict__ Kc,
                                                                    const float4* __restrict__ Vc, const int* __restrict__ start,
                                                                    float* __restrict__ O, float* __restrict__ ws, int T, int H, int cap,
                                                                    int nchunks, float c1) {
    constexpr int LPK = DH / 4, G = ADEC_THREADS / LPK, C = G * ADEC_KPG;
    static_assert(C == adec_chunk_of(DH), "chunk");
    __shared__ float4 ro[G * LPK];
    __shared__ float rl[G];
    __shared__ float red[ADEC_THREADS / 64];
    const int tid = threadIdx.x, g = tid / LPK, sub = tid % LPK;
    const int prob = blockIdx.x, chunk = blockIdx.y;
    const int row = prob / H, h = prob % H, b = row / T, t = row % T;
    const int n = adec_len(start, b, t, cap), c0 = chunk * C;
    float* __restrict__ out = O + (size_t)row * H * DH + (size_t)h * DH;
    if (c0 >= n) {  // the same decision in every thread of the block
        if (chunk == 0 && tid < DH) out[tid] = 0.f;
        return;
    }
    const float* __restrict__ qp = Q + (size_t)row * ldq + (size_t)h * DH + sub * 4;
    const float4 q = make_float4(qp[0], qp[1], qp[2], qp[3]);
    const size_t base = ((size_t)b * H + h) * cap * LPK + sub;
    float4 kk[ADEC_KPG], vv[ADEC_KPG];
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i) {
        const int j = c0 + i * G + g;
        kk[i] = Kc[base + (size_t)(j < n ? j : n - 1) * LPK];
    }
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i) {
        const int j = c0 + i * G + g;
        vv[i] = Vc[base + (size_t)(j < n ? j : n - 1) * LPK];
    }
    float s[ADEC_KPG], m = -INFINITY;
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i) {
        float d = q.x * kk[i].x;
        d = __builtin_fmaf(q.y, kk[i].y, d);
        d = __builtin_fmaf(q.z, kk[i].z, d);
        d = __builtin_fmaf(q.w, kk[i].w, d);
#pragma unroll
        for (int off = LPK / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
        s[i] = c0 + i * G + g < n ? d * c1 : -INFINITY;
        m = fmaxf(m, s[i]);
    }
    m = nk_wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));  // finite: key c0 is one of the problem's
    float l = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i) {
        const float p = c0 + i * G + g < n ? __builtin_amdgcn_exp2f(s[i] - m) : 0.f;
        l += p;
        acc.x = __builtin_fmaf(p, vv[i].x, acc.x);
        acc.y = __builtin_fmaf(p, vv[i].y, acc.y);
        acc.z = __builtin_fmaf(p, vv[i].z, acc.z);
        acc.w = __builtin_fmaf(p, vv[i].w, acc.w);
    }
    ro[g * LPK + sub] = acc;
    if (sub == 0) rl[g] = l;
    __syncthreads();
    if (tid >= DH) return;
    const float* __restrict__ rf = reinterpret_cast<const float*>(ro);
    float o = rf[tid], ls = rl[0];
#pragma unroll
    for (int k = 1; k < G; ++k) {  // the groups in order
        o += rf[k * DH + tid];
        ls += rl[k];
    }
    if (n <= C) {
        out[tid] = o / ls;
        return;
    }
    float* __restrict__ part = ws + ((size_t)prob * nchunks + chunk) * (DH + 2);
    part[tid] = o;
    if (tid == 0) {
        part[DH] = m;
        part[DH + 1] = ls;
    }
}

__global__ void __launch_bounds__(ADEC_THREADS) adec_generic_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ Kc,
                                                                    const float* __restrict__ Vc, const int* __restrict__ start,
                                                                    float* __restrict__ O, float* __restrict__ ws, int T, int H, int dh,
                                                                    int cap, int nchunks, float c1, int lpk) {
    constexpr int C = ADEC_CHUNK_GENERIC;
    static_assert(C == ADEC_THREADS, "one key per thread");
    __shared__ float sc[C];
    __shared__ float ro[ADEC_THREADS];
    __shared__ float red[ADEC_THREADS / 64];
    const int tid = threadIdx.x, G = ADEC_THREADS / lpk, g = tid / lpk, sub = tid & (lpk - 1);  // lpk keys per group: C / G
    const int prob = blockIdx.x, chunk = blockIdx.y;
    const int row = prob / H, h = prob % H, b = row / T, t = row % T;
    const int n = adec_len(start, b, t, cap), c0 = chunk * C;
    float* __restrict__ out = O + (size_t)row * H * dh + (size_t)h * dh;
    if (c0 >= n) {
        if (chunk == 0)
            for (int e = tid; e < dh; e += ADEC_THREADS) out[e] = 0.f;
        return;
    }
    const float* __restrict__ qp = Q + (size_t)row * ldq + (size_t)h * dh;
    const size_t base = ((size_t)b * H + h) * cap * dh;
    for (int i = 0; i < lpk; ++i) {
        const int j = c0 + i * G + g;
        const float* __restrict__ kr = Kc + base + (size_t)(j < n ? j : n - 1) * dh;
        float d = 0.f;
        for (int e = sub; e < dh; e += lpk) d = __builtin_fmaf(qp[e], kr[e], d);
        for (int off = lpk >> 1; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
        if (sub == 0) sc[i * G + g] = j < n ? d * c1 : -INFINITY;
    }
    __syncthreads();
    const float sv = sc[tid];
    const float m = nk_block_max<ADEC_THREADS>(sv, red);
    const float p = c0 + tid < n ? __builtin_amdgcn_exp2f(sv - m) : 0.f;
    const float l = nk_block_sum<ADEC_THREADS>(p, red);
    sc[tid] = p;  // a thread's own slot
    __syncthreads();
    const bool single = n <= C;
    float* __restrict__ part = ws + ((size_t)prob * nchunks + chunk) * ((size_t)dh + 2);
    for (int e0 = 0; e0 < dh; e0 += lpk) {
        const int e = e0 + sub;
        float acc = 0.f;
        if (e < dh)
            for (int i = 0; i < lpk; ++i) {
                const int jl = i * G + g, j = c0 + jl;
                acc = __builtin_fmaf(sc[jl], Vc[base + (size_t)(j < n ? j : n - 1) * dh + e], acc);
            }
        ro[tid] = acc;  // ro[g * lpk + sub]
        __syncthreads();
        if (tid < lpk && e0 + tid < dh) {
            float o = ro[tid];
            for (int k = 1; k < G; ++k) o += ro[k * lpk + tid];  // the groups in order
            if (single) out[e0 + tid] = o / l;
            else part[e0 + tid] = o;
        }
        __syncthreads();
    }
    if (!single && tid == 0) {
        part[dh] = m;
        part[dh + 1] = l;
    }
}

// the partials of every problem longer than one chunk, in chunk order
__global__ void __launch_bounds__(256) adec_combine_kernel(const float* __restrict__ ws, const int* __restrict__ start, float* __restrict__ O,
                                                           int T, int H, int dh, int cap, int nchunks, int C, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int e = (int)(i % dh);
    const long long prob = i / dh;
    const int row = (int)(prob / H), b = row / T, t = row % T;
    const int n = adec_len(start, b, t, cap);
    if (n <= C) return;  // written by the partial kernel
    const int nc = (n + C - 1) / C;
    const size_t stride = (size_t)dh + 2;
    const float* __restrict__ part = ws + (size_t)prob * nchunks * stride;
    float m = part[dh];
    for (int c = 1; c < nc; ++c) m = fmaxf(m, part[c * stride + dh]);
    float o = 0.f, l = 0.f;
    for (int c = 0; c < nc; ++c) {
        const float f = __builtin_amdgcn_exp2f(part[c * stride + dh] - m);
        o = __builtin_fmaf(part[c * stride + e], f, o);
        l = __builtin_fmaf(part[c * stride + dh + 1], f, l);
    }
    O[(size_t)prob * dh + e] = o / l;  // prob = (b*T + t)*H + h: column h*dh + e of row b*T + t
}

int adec_check(nk_device* dev, int B, int T, int H, int dh, int cap, const char* what) {
    NK_CHECK(dev != nullptr, "null device handle");
    NK_CHECK(B > 0 && T > 0 && H > 0 && dh > 0 && cap > 0, "%s: B, T, H, dh and cap must be positive, got %d, %d, %d, %d, %d", what, B, T, H, dh,
             cap);
    // B*T*H is grid.x of 256-thread blocks: a launch takes fewer than 2^32 threads along an axis
    NK_CHECK((long long)B * T * H < (1ll << 24) && (long long)H * dh <= 0x7fffffffLL, "%s: B*T*H must be below 2^24 and H*dh fit 31 bits", what);
    NK_CHECK((cap + adec_chunk_of(dh) - 1) / adec_chunk_of(dh) <= 65535, "%s: cap %d is more than 65535 chunks of %d keys", what, cap,
             adec_chunk_of(dh));
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_attention_decode_chunk(int dh) { return dh > 0 ? adec_chunk_of(dh) : 0; }

size_t nk_attention_decode_workspace(int B, int T, int H, int dh, int cap) {
    if (B <= 0 || T <= 0 || H <= 0 || dh <= 0 || cap <= 0) return 0;
    const int C = adec_chunk_of(dh);
    return (size_t)B * T * H * (size_t)((cap + C - 1) / C) * ((size_t)dh + 2);
}

int nk_kv_cache_append(nk_device* dev, float* Kc, float* Vc, const float* K, const float* V, int ld, const int* start, int B, int T, int H,
                       int dh, int cap) {
    if (int rc = adec_check(dev, B, T, H, dh, cap, "nk_kv_cache_append")) return rc;
    NK_CHECK(Kc != nullptr && Vc != nullptr && K != nullptr && V != nullptr && start != nullptr, "nk_kv_cache_append: null pointer");
    NK_CHECK(ld >= H * dh, "nk_kv_cache_append: row stride %d is shorter than H*dh = %d", ld, H * dh);
    NK_USE(dev);
    const bool vec = dh % 4 == 0 && ld % 4 == 0 && adec_al16(Kc) && adec_al16(Vc) && adec_al16(K) && adec_al16(V);
    const int DV = vec ? dh / 4 : dh;
    const long long total = (long long)B * T * H * DV;
    const dim3 grid(nk_stream_grid((size_t)total, 256)), block(256);
    if (vec)
        hipLaunchKernelGGL((kv_append_kernel<float4>), grid, block, 0, dev->compute, reinterpret_cast<float4*>(Kc), reinterpret_cast<float4*>(Vc),
                           reinterpret_cast<const float4*>(K), reinterpret_cast<const float4*>(V), (long long)(ld / 4), start, T, H, DV, cap,
                           total);
    else
        hipLaunchKernelGGL((kv_append_kernel<float>), grid, block, 0, dev->compute, Kc, Vc, K, V, (long long)ld, start, T, H, DV, cap, total);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int nk_attention_decode_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, float* O,
                            float* workspace, int B, int T, int H, int dh, int cap, float scale) {
    const char* what = "nk_attention_decode_fwd";
    if (int rc = adec_check(dev, B, T, H, dh, cap, what)) return rc;
    NK_CHECK(Q != nullptr && Kc != nullptr && Vc != nullptr && start != nullptr && O != nullptr && workspace != nullptr, "%s: null pointer", what);
    NK_CHECK(scale > 0.f && scale < INFINITY, "%s: scale must be positive and finite, got %g", what, (double)scale);
    NK_CHECK(ldq >= H * dh, "%s: row stride %d is shorter than H*dh = %d", what, ldq, H * dh);
    const bool vec = dh == 32 || dh == 64 || dh == 128;
    // the instantiation (and with it the chunk size and the summation order) is a function of dh alone: no silent scalar path
    NK_CHECK(!vec || (adec_al16(Kc) && adec_al16(Vc)), "%s: the caches must be 16-byte aligned", what);
    NK_USE(dev);
    const int C = adec_chunk_of(dh), nchunks = (cap + C - 1) / C, P = B * T * H;
    const float c1 = scale * ADEC_LOG2E;
    const dim3 grid(P, nchunks), block(ADEC_THREADS);
    const float4* k4 = reinterpret_cast<const float4*>(Kc);
    const float4* v4 = reinterpret_cast<const float4*>(Vc);
    if (dh == 32)
        hipLaunchKernelGGL((adec_partial_kernel<32>), grid, block, 0, dev->compute, Q, ldq, k4, v4, start, O, workspace, T, H, cap, nchunks, c1);
    else if (dh == 64)
        hipLaunchKernelGGL((adec_partial_kernel<64>), grid, block, 0, dev->compute, Q, ldq, k4, v4, start, O, workspace, T, H, cap, nchunks, c1);
    else if (dh == 128)
        hipLaunchKernelGGL((adec_partial_kernel<128>), grid, block, 0, dev->compute, Q, ldq, k4, v4, start, O, workspace, T, H, cap, nchunks, c1);
    else {
        int lpk = 1;
        while (lpk < 64 && lpk < dh) lpk *= 2;
        hipLaunchKernelGGL(adec_generic_kernel, grid, block, 0, dev->compute, Q, ldq, Kc, Vc, start, O, workspace, T, H, dh, cap, nchunks, c1, lpk);
    }
    NK_LAUNCH_CHECK();
    if (nchunks > 1) {
        const long long total = (long long)P * dh;
        hipLaunchKernelGGL(adec_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, dev->compute, workspace, start, O, T, H, dh,
                           cap, nchunks, C, total);
        NK_LAUNCH_CHECK();
    }
    return NK_OK;
}

}  // extern "C"
