// Grouped-query decode (ours; semantics in include/neuronika_hip.h): H query heads over Hkv <= H key / value heads, R = H / Hkv query
// heads per kv head.  Included by nk_norm.hip after nk_attention_decode.h, whose constants, adec_len, adec_check and
// adec_combine_kernel it uses as they are.  The decode step is bound by the bytes of K and V (cdna_hip_programming.md "Attention
// decode": up to 8 query rows per kv head, K/V straight to VGPRs), so the heads of a group share ONE read of their chunk:
//   partial   one 256-thread block per ((b, t, kv head), batch of at most ADEC_GQA_HEADS = 8 query heads of the group, chunk of
//             adec_chunk_of(dh) keys).  The block loads its chunk of K and V once with the lane / group ownership of
//             adec_partial_kernel (dh / 4 lanes own a key, 16-byte loads, keys >= n redirected to key n - 1 and their probability
//             SELECTED to 0) and keeps all 16 + 16 float4 per lane in registers; then, head by head, the arithmetic of
//             adec_partial_kernel statement for statement over those registers - dot, xor-shuffles, chunk maximum, exp2, the groups
//             in order.  The bits of a head's result are therefore those nk_attention_decode_fwd gives for the same query over the
//             same n keys and values: they do not depend on R, on the heads that share the block, or on B, T, cap.
//             (Three heads in flight per pass was measured and not kept: a head costs about 2 us of issue time in its block
//             either way, and the registers go from 176 to 241; four take 272, one wave per SIMD - DESIGN.md.)
//             Partials go to the workspace in nk_attention_decode_fwd's per-(b, t, h) layout; adec_combine_kernel merges them.
//             A group of more than 8 heads takes ceil(R / 8) blocks (each reads the chunk: 8 heads keep the register budget fixed).
//   generic   any other dh: adec_generic_kernel's body with the cache head h / R.  Nothing is shared; correctness only.
// No atomics, no scratch, nothing derived from the CU count.
#pragma once
#include "nk_attention_decode.h"

namespace {

constexpr int ADEC_GQA_HEADS = 8;  // query heads of one group a block serves from one read of the chunk

template <int DH>
__global__ void __launch_bounds__(ADEC_THREADS) adec_gqa_partial_kernel(const float* __restrict__ Q, int ldq, const float4* __restrict__ Kc,
                                                                        const float4* __restrict__ Vc, const int* __restrict__ start,
                                                                        float* __restrict__ O, float* __restrict__ ws, int T, int H, int Hkv,
                                                                        int cap, int nchunks, float c1) {
    constexpr int LPK = DH / 4, G = ADEC_THREADS / LPK, C = G * ADEC_KPG;
    static_assert(C == adec_chunk_of(DH), "chunk");
    __shared__ float4 ro[G * LPK];
    __shared__ float rl[G];
    __shared__ float red[ADEC_THREADS / 64];
    const int tid = threadIdx.x, g = tid / LPK, sub = tid % LPK;
    const int R = H / Hkv, nb = (R + ADEC_GQA_HEADS - 1) / ADEC_GQA_HEADS;
    const int hb = blockIdx.x % nb, pk = blockIdx.x / nb, chunk = blockIdx.y;
    const int row = pk / Hkv, kvh = pk % Hkv, b = row / T, t = row % T;
    const int h0 = kvh * R + hb * ADEC_GQA_HEADS, nh = R - hb * ADEC_GQA_HEADS < ADEC_GQA_HEADS ? R - hb * ADEC_GQA_HEADS : ADEC_GQA_HEADS;
    const int n = adec_len(start, b, t, cap), c0 = chunk * C;
    float* __restrict__ out = O + (size_t)row * H * DH + (size_t)h0 * DH;  // the block's nh heads are contiguous columns
    if (c0 >= n) {  // the same decision in every thread of the block
        if (chunk == 0)
            for (int e = tid; e < nh * DH; e += ADEC_THREADS) out[e] = 0.f;
        return;
    }
    const size_t base = ((size_t)b * Hkv + kvh) * cap * LPK + sub;
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
#pragma unroll 1
    for (int hq = 0; hq < nh; ++hq) {  // adec_partial_kernel's arithmetic per head, over the registers above
        const float* __restrict__ qp = Q + (size_t)row * ldq + (size_t)(h0 + hq) * DH + sub * 4;
        const float4 q = make_float4(qp[0], qp[1], qp[2], qp[3]);
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
        // the next head writes red before its first barrier and ro / rl after it: every read below is over by then
        if (tid < DH) {
            const float* __restrict__ rf = reinterpret_cast<const float*>(ro);
            float o = rf[tid], ls = rl[0];
#pragma unroll
            for (int k = 1; k < G; ++k) {  // the groups in order
                o += rf[k * DH + tid];
                ls += rl[k];
            }
            if (n <= C) {
                out[hq * DH + tid] = o / ls;
            } else {
                float* __restrict__ part = ws + (((size_t)row * H + h0 + hq) * nchunks + chunk) * (DH + 2);
                part[tid] = o;
                if (tid == 0) {
                    part[DH] = m;
                    part[DH + 1] = ls;
                }
            }
        }
    }
}

// adec_generic_kernel with the cache head h / R (that kernel stays as it is, so its body is restated here)
__global__ void __launch_bounds__(ADEC_THREADS) adec_gqa_generic_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ Kc,
                                                                        const float* __restrict__ Vc, const int* __restrict__ start,
                                                                        float* __restrict__ O, float* __restrict__ ws, int T, int H, int Hkv,
                                                                        int dh, int cap, int nchunks, float c1, int lpk) {
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
    const size_t base = ((size_t)b * Hkv + h / (H / Hkv)) * cap * dh;
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

}  // namespace

extern "C" {

int nk_attention_decode_gqa_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, float* O,
                                float* workspace, int B, int T, int H, int Hkv, int dh, int cap, float scale) {
    const char* what = "nk_attention_decode_gqa_fwd";
    NK_CHECK(dev != nullptr, "null device handle");
    NK_CHECK(Hkv > 0 && Hkv <= H && H % Hkv == 0, "%s: Hkv must be positive and divide H, got H = %d, Hkv = %d", what, H, Hkv);
    if (Hkv == H) return nk_attention_decode_fwd(dev, Q, ldq, Kc, Vc, start, O, workspace, B, T, H, dh, cap, scale);  // today's launches
    if (int rc = adec_check(dev, B, T, H, dh, cap, what)) return rc;
    NK_CHECK(Q != nullptr && Kc != nullptr && Vc != nullptr && start != nullptr && O != nullptr && workspace != nullptr, "%s: null pointer", what);
    NK_CHECK(scale > 0.f && scale < INFINITY, "%s: scale must be positive and finite, got %g", what, (double)scale);
    NK_CHECK(ldq >= H * dh, "%s: row stride %d is shorter than H*dh = %d", what, ldq, H * dh);
    const bool vec = dh == 32 || dh == 64 || dh == 128;
    NK_CHECK(!vec || (adec_al16(Kc) && adec_al16(Vc)), "%s: the caches must be 16-byte aligned", what);
    NK_USE(dev);
    const int C = adec_chunk_of(dh), nchunks = (cap + C - 1) / C, R = H / Hkv;
    const int P = B * T * H, PB = B * T * Hkv * ((R + ADEC_GQA_HEADS - 1) / ADEC_GQA_HEADS);  // PB <= P < 2^24
    const float c1 = scale * ADEC_LOG2E;
    const dim3 grid(PB, nchunks), block(ADEC_THREADS);
    const float4* k4 = reinterpret_cast<const float4*>(Kc);
    const float4* v4 = reinterpret_cast<const float4*>(Vc);
    if (dh == 32)
        hipLaunchKernelGGL((adec_gqa_partial_kernel<32>), grid, block, 0, dev->compute, Q, ldq, k4, v4, start, O, workspace, T, H, Hkv, cap, nchunks,
                           c1);
    else if (dh == 64)
        hipLaunchKernelGGL((adec_gqa_partial_kernel<64>), grid, block, 0, dev->compute, Q, ldq, k4, v4, start, O, workspace, T, H, Hkv, cap, nchunks,
                           c1);
    else if (dh == 128)
        hipLaunchKernelGGL((adec_gqa_partial_kernel<128>), grid, block, 0, dev->compute, Q, ldq, k4, v4, start, O, workspace, T, H, Hkv, cap,
                           nchunks, c1);
    else {
        int lpk = 1;
        while (lpk < 64 && lpk < dh) lpk *= 2;
        hipLaunchKernelGGL(adec_gqa_generic_kernel, dim3(P, nchunks), block, 0, dev->compute, Q, ldq, Kc, Vc, start, O, workspace, T, H, Hkv, dh,
                           cap, nchunks, c1, lpk);
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
