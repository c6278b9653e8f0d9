// Sliding-window decode (ours; semantics in include/neuronika_hip.h): query position i attends to the keys max(0, i - W + 1) .. i, on
// a linear cache (position p at slot p) or a rolling one (position p at slot p % cap).  Included by nk_norm.hip after
// nk_attention_gqa.h, whose constants, adec_chunk_of, adec_check and ADEC_GQA_HEADS it uses as they are.  A step reads at most W keys
// per kv head whatever the length: the grid and the workspace are sized by the window, never by the capacity.
//   chunks    stay aligned to ABSOLUTE positions: chunk c covers positions [cC, cC + C), C = adec_chunk_of(dh).  A problem with
//             n = start[b] + t + 1 and lo = max(0, n - W) visits chunks lo / C .. (n - 1) / C only - at most (W + C - 2) / C + 1 of
//             them - and blockIdx.y counts from lo / C.  Inside a chunk the lane / group ownership is adec_partial_kernel's by
//             position (group g owns positions c0 + g, c0 + G + g, ...), so for n <= W (lo = 0) every partial, and the merge, is
//             nk_attention_decode_fwd's bit for bit; and the bits of a problem depend on (q, its keys / values at [lo, n), n, W,
//             scale) alone - not on where a position is stored.
//   slots     s0 = the slot of position lo (lo % cap on a ring: one scalar remainder per block); position p is at s0 + (p - lo),
//             minus cap if that reaches cap (n - lo <= W <= cap, so one conditional subtract; it never fires on a linear cache).
//             No table, no dependent load.
//   partial   adw_partial_kernel<DH, NH>: adec_partial_kernel (NH = 1) / adec_gqa_partial_kernel (NH = 8 query heads over one
//             read of the chunk) statement for statement, with "position < n" replaced by "lo <= position < n".  Positions of a
//             visited chunk outside [lo, n): the load is redirected to position n - 1 (always in the window), the probability is
//             SELECTED to 0, the chunk's shift is the exact maximum over its in-window keys.  A window inside one chunk writes O.
//   combine   adw_combine_kernel: adec_combine_kernel over the problem's visited chunks, ascending.  No atomics, no arrival order.
//   generic   adw_generic_kernel: adec_gqa_generic_kernel's body (any other dh), with the window and the slots.
//   append    kv_append_ring_kernel: kv_append_kernel with slot (start[b] + t) % cap; every row with a position >= 0 is written.
#pragma once
#include "nk_attention_gqa.h"

namespace {

// positions stay 31-bit with a chunk to spare: c0 + C never overflows
constexpr long long ADW_MAX_POS = 0x7fffffffLL - 1024;

// window chunks a problem can touch: a function of W and C only
constexpr long long adw_chunks_of(long long W, int C) { return (W + C - 2) / C + 1; }

// keys query (b, t) ends at: start[b] + t + 1, clipped to cap on a linear cache; <= 0 for a negative start (the output row is then 0)
__device__ __forceinline__ int adw_len(const int* __restrict__ start, int b, int t, int cap, int ring) {
    const long long n = (long long)start[b] + t + 1;
    const long long top = ring ? ADW_MAX_POS : (long long)cap;
    return n > top ? (int)top : (n < 0 ? 0 : (int)n);
}

template <typename T>
__global__ void __launch_bounds__(256) kv_append_ring_kernel(T* __restrict__ Kc, T* __restrict__ Vc, const T* __restrict__ K,
                                                             const T* __restrict__ V, long long ldv, const int* __restrict__ start, int Tn,
                                                             int H, int DV, int cap, long long total) {
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const int q = (int)(i % DV);
        const long long rh = i / DV;
        const int h = (int)(rh % H);
        const long long row = rh / H;
        const int b = (int)(row / Tn), t = (int)(row % Tn);
        const long long pos = (long long)start[b] + t;
        if (pos < 0) continue;
        const size_t src = (size_t)row * ldv + (size_t)h * DV + q;
        const size_t dst = (((size_t)b * H + h) * cap + (size_t)(pos % cap)) * DV + q;  // T <= cap: no two rows of a sample share a slot
        const T kv = K[src], vv = V[src];
        Kc[dst] = kv;
        Vc[dst] = vv;
    }
}

// NH = 1: H == Hkv, one block per (b, t, h).  NH = ADEC_GQA_HEADS: one block per ((b, t, kv head), batch of at most NH heads).
template <int DH, int NH>
__global__ void __launch_bounds__(ADEC_THREADS) adw_partial_kernel(const float* __restrict__ Q, int ldq, const float4* __restrict__ Kc,
                                                                   const float4* __restrict__ Vc, const int* __restrict__ start,
                                                                   float* __restrict__ O, float* __restrict__ ws, int T, int H, int Hkv,
                                                                   int cap, int W, int ring, int nwc, float c1) {
    constexpr int LPK = DH / 4, G = ADEC_THREADS / LPK, C = G * ADEC_KPG;
    static_assert(C == adec_chunk_of(DH), "chunk");
    __shared__ float4 ro[G * LPK];
    __shared__ float rl[G];
    __shared__ float red[ADEC_THREADS / 64];
    const int tid = threadIdx.x, g = tid / LPK, sub = tid % LPK;
    const int R = H / Hkv, nb = (R + NH - 1) / NH;
    const int hb = blockIdx.x % nb, pk = blockIdx.x / nb;
    const int row = pk / Hkv, kvh = pk % Hkv, b = row / T, t = row % T;
    const int h0 = kvh * R + hb * NH, nh = NH == 1 ? 1 : (R - hb * NH < NH ? R - hb * NH : NH);
    const int n = adw_len(start, b, t, cap, ring), lo = n > W ? n - W : 0;
    float* __restrict__ out = O + (size_t)row * H * DH + (size_t)h0 * DH;  // the block's nh heads are contiguous columns
    if (n <= 0) {  // the same decision in every thread of the block
        if (blockIdx.y == 0)
            for (int e = tid; e < nh * DH; e += ADEC_THREADS) out[e] = 0.f;
        return;
    }
    const int cf = lo / C, cl = (n - 1) / C, chunk = cf + (int)blockIdx.y;
    if (chunk > cl) return;
    const int s0 = ring ? lo % cap : lo;  // the slot of position lo
    // positions relative to lo: key i of this lane group is r0 + i * G, inside the window iff 0 <= r < wn - ONE unsigned compare,
    // the cost of adec_partial_kernel's "position < n"
    const int r0 = chunk * C + g - lo;
    const unsigned wn = (unsigned)(n - lo);
    const size_t base = ((size_t)b * Hkv + kvh) * cap * LPK + sub;
    float4 kk[ADEC_KPG], vv[ADEC_KPG];
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i) {
        const int r = r0 + i * G;
        const int sl = s0 + ((unsigned)r < wn ? r : (int)wn - 1);
        kk[i] = Kc[base + (size_t)(sl >= cap ? sl - cap : sl) * LPK];
    }
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i) {
        const int r = r0 + i * G;
        const int sl = s0 + ((unsigned)r < wn ? r : (int)wn - 1);
        vv[i] = Vc[base + (size_t)(sl >= cap ? sl - cap : sl) * LPK];
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
            s[i] = (unsigned)(r0 + i * G) < wn ? d * c1 : -INFINITY;
            m = fmaxf(m, s[i]);
        }
        m = nk_wave_max(m);
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));  // finite: a visited chunk holds a key of the window
        float l = 0.f;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < ADEC_KPG; ++i) {
            const float p = (unsigned)(r0 + i * G) < wn ? __builtin_amdgcn_exp2f(s[i] - m) : 0.f;
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
            if (cf == cl) {
                out[hq * DH + tid] = o / ls;
            } else {
                float* __restrict__ part = ws + (((size_t)row * H + h0 + hq) * nwc + blockIdx.y) * (DH + 2);
                part[tid] = o;
                if (tid == 0) {
                    part[DH] = m;
                    part[DH + 1] = ls;
                }
            }
        }
    }
}

// adec_gqa_generic_kernel with the window and the slots (H == Hkv included: h / 1)
__global__ void __launch_bounds__(ADEC_THREADS) adw_generic_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ Kc,
                                                                   const float* __restrict__ Vc, const int* __restrict__ start,
                                                                   float* __restrict__ O, float* __restrict__ ws, int T, int H, int Hkv, int dh,
                                                                   int cap, int W, int ring, int nwc, float c1, int lpk) {
    constexpr int C = ADEC_CHUNK_GENERIC;
    static_assert(C == ADEC_THREADS, "one key per thread");
    __shared__ float sc[C];
    __shared__ float ro[ADEC_THREADS];
    __shared__ float red[ADEC_THREADS / 64];
    const int tid = threadIdx.x, G = ADEC_THREADS / lpk, g = tid / lpk, sub = tid & (lpk - 1);  // lpk keys per group: C / G
    const int prob = blockIdx.x;
    const int row = prob / H, h = prob % H, b = row / T, t = row % T;
    const int n = adw_len(start, b, t, cap, ring), lo = n > W ? n - W : 0;
    float* __restrict__ out = O + (size_t)row * H * dh + (size_t)h * dh;
    if (n <= 0) {
        if (blockIdx.y == 0)
            for (int e = tid; e < dh; e += ADEC_THREADS) out[e] = 0.f;
        return;
    }
    const int cf = lo / C, cl = (n - 1) / C, chunk = cf + (int)blockIdx.y;
    if (chunk > cl) return;
    const int c0 = chunk * C;
    const int s0 = ring ? lo % cap : lo;
    const float* __restrict__ qp = Q + (size_t)row * ldq + (size_t)h * dh;
    const size_t base = ((size_t)b * Hkv + h / (H / Hkv)) * cap * dh;
    for (int i = 0; i < lpk; ++i) {
        const int j = c0 + i * G + g;
        const bool in = j >= lo && j < n;
        const int sl = s0 + (in ? j : n - 1) - lo;
        const float* __restrict__ kr = Kc + base + (size_t)(sl >= cap ? sl - cap : sl) * dh;
        float d = 0.f;
        for (int e = sub; e < dh; e += lpk) d = __builtin_fmaf(qp[e], kr[e], d);
        for (int off = lpk >> 1; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
        if (sub == 0) sc[i * G + g] = in ? d * c1 : -INFINITY;
    }
    __syncthreads();
    const float sv = sc[tid];
    const float m = nk_block_max<ADEC_THREADS>(sv, red);
    const float p = (c0 + tid >= lo && c0 + tid < n) ? __builtin_amdgcn_exp2f(sv - m) : 0.f;
    const float l = nk_block_sum<ADEC_THREADS>(p, red);
    sc[tid] = p;  // a thread's own slot
    __syncthreads();
    const bool single = cf == cl;
    float* __restrict__ part = ws + ((size_t)prob * nwc + blockIdx.y) * ((size_t)dh + 2);
    for (int e0 = 0; e0 < dh; e0 += lpk) {
        const int e = e0 + sub;
        float acc = 0.f;
        if (e < dh)
            for (int i = 0; i < lpk; ++i) {
                const int jl = i * G + g, j = c0 + jl;
                const int sl = s0 + ((j >= lo && j < n) ? j : n - 1) - lo;
                acc = __builtin_fmaf(sc[jl], Vc[base + (size_t)(sl >= cap ? sl - cap : sl) * dh + e], acc);
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

// the partials of every problem whose window spans more than one chunk, in chunk order (adec_combine_kernel's arithmetic)
__global__ void __launch_bounds__(256) adw_combine_kernel(const float* __restrict__ ws, const int* __restrict__ start, float* __restrict__ O,
                                                          int T, int H, int dh, int cap, int W, int ring, int nwc, int C, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int e = (int)(i % dh);
    const long long prob = i / dh;
    const int row = (int)(prob / H), b = row / T, t = row % T;
    const int n = adw_len(start, b, t, cap, ring), lo = n > W ? n - W : 0;
    if (n <= 0) return;  // zeroed by the partial kernel
    const int nc = (n - 1) / C - lo / C + 1;
    if (nc == 1) return;  // written by the partial kernel
    const size_t stride = (size_t)dh + 2;
    const float* __restrict__ part = ws + (size_t)prob * nwc * stride;
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

}  // namespace

extern "C" {

size_t nk_attention_decode_window_workspace(int B, int T, int H, int dh, int window) {
    if (B <= 0 || T <= 0 || H <= 0 || dh <= 0 || window <= 0) return 0;
    return (size_t)B * T * H * (size_t)adw_chunks_of(window, adec_chunk_of(dh)) * ((size_t)dh + 2);
}

int nk_kv_cache_append_ring(nk_device* dev, float* Kc, float* Vc, const float* K, const float* V, int ld, const int* start, int B, int T,
                            int H, int dh, int cap) {
    const char* what = "nk_kv_cache_append_ring";
    if (int rc = adec_check(dev, B, T, H, dh, cap, what)) return rc;
    NK_CHECK(Kc != nullptr && Vc != nullptr && K != nullptr && V != nullptr && start != nullptr, "%s: null pointer", what);
    NK_CHECK(ld >= H * dh, "%s: row stride %d is shorter than H*dh = %d", what, ld, H * dh);
    NK_CHECK(T <= cap, "%s: %d rows per sample would overwrite each other in a ring of %d slots", what, T, cap);
    NK_USE(dev);
    const bool vec = dh % 4 == 0 && ld % 4 == 0 && adec_al16(Kc) && adec_al16(Vc) && adec_al16(K) && adec_al16(V);
    const int DV = vec ? dh / 4 : dh;
    const long long total = (long long)B * T * H * DV;
    const dim3 grid(nk_stream_grid((size_t)total, 256)), block(256);
    if (vec)
        hipLaunchKernelGGL((kv_append_ring_kernel<float4>), grid, block, 0, dev->compute, reinterpret_cast<float4*>(Kc),
                           reinterpret_cast<float4*>(Vc), reinterpret_cast<const float4*>(K), reinterpret_cast<const float4*>(V),
                           (long long)(ld / 4), start, T, H, DV, cap, total);
    else
        hipLaunchKernelGGL((kv_append_ring_kernel<float>), grid, block, 0, dev->compute, Kc, Vc, K, V, (long long)ld, start, T, H, DV, cap,
                           total);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int nk_attention_decode_window_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, float* O,
                                   float* workspace, int B, int T, int H, int Hkv, int dh, int cap, int window, int ring, float scale) {
    const char* what = "nk_attention_decode_window_fwd";
    NK_CHECK(dev != nullptr, "null device handle");
    NK_CHECK(Hkv > 0 && Hkv <= H && H % Hkv == 0, "%s: Hkv must be positive and divide H, got H = %d, Hkv = %d", what, H, Hkv);
    if (int rc = adec_check(dev, B, T, H, dh, cap, what)) return rc;
    NK_CHECK(Q != nullptr && Kc != nullptr && Vc != nullptr && start != nullptr && O != nullptr && workspace != nullptr, "%s: null pointer", what);
    NK_CHECK(scale > 0.f && scale < INFINITY, "%s: scale must be positive and finite, got %g", what, (double)scale);
    NK_CHECK(ldq >= H * dh, "%s: row stride %d is shorter than H*dh = %d", what, ldq, H * dh);
    NK_CHECK(window > 0, "%s: window must be positive, got %d", what, window);
    NK_CHECK(!ring || (long long)window + T - 1 <= cap, "%s: a ring of %d slots cannot hold a window of %d keys and %d new rows (window + T - 1 <= cap)",
             what, cap, window, T);
    const bool vec = dh == 32 || dh == 64 || dh == 128;
    NK_CHECK(!vec || (adec_al16(Kc) && adec_al16(Vc)), "%s: the caches must be 16-byte aligned", what);
    NK_USE(dev);
    // n <= cap on a linear cache, so a window above cap is the window cap: the same lo for every problem, fewer empty blocks
    const int W = window < cap ? window : cap;
    const int C = adec_chunk_of(dh), nwc = (int)adw_chunks_of(W, C), R = H / Hkv;
    NK_CHECK(nwc <= 65535, "%s: a window of %d keys is more than 65534 chunks of %d keys", what, W, C);
    const int P = B * T * H, PB = B * T * Hkv * ((R + ADEC_GQA_HEADS - 1) / ADEC_GQA_HEADS);  // PB <= P < 2^24
    const float c1 = scale * ADEC_LOG2E;
    const dim3 block(ADEC_THREADS);
    const float4* k4 = reinterpret_cast<const float4*>(Kc);
    const float4* v4 = reinterpret_cast<const float4*>(Vc);
#define NK_ADW_LAUNCH(DH)                                                                                                                  \
    do {                                                                                                                                   \
        if (R == 1)                                                                                                                        \
            hipLaunchKernelGGL((adw_partial_kernel<DH, 1>), dim3(P, nwc), block, 0, dev->compute, Q, ldq, k4, v4, start, O, workspace, T, H, \
                               Hkv, cap, W, ring, nwc, c1);                                                                                \
        else                                                                                                                               \
            hipLaunchKernelGGL((adw_partial_kernel<DH, ADEC_GQA_HEADS>), dim3(PB, nwc), block, 0, dev->compute, Q, ldq, k4, v4, start, O,  \
                               workspace, T, H, Hkv, cap, W, ring, nwc, c1);                                                               \
    } while (0)
    if (dh == 32)
        NK_ADW_LAUNCH(32);
    else if (dh == 64)
        NK_ADW_LAUNCH(64);
    else if (dh == 128)
        NK_ADW_LAUNCH(128);
    else {
        int lpk = 1;
        while (lpk < 64 && lpk < dh) lpk *= 2;
        hipLaunchKernelGGL(adw_generic_kernel, dim3(P, nwc), block, 0, dev->compute, Q, ldq, Kc, Vc, start, O, workspace, T, H, Hkv, dh, cap, W,
                           ring, nwc, c1, lpk);
    }
#undef NK_ADW_LAUNCH
    NK_LAUNCH_CHECK();
    if (nwc > 1) {
        const long long total = (long long)P * dh;
        hipLaunchKernelGGL(adw_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, dev->compute, workspace, start, O, T, H, dh,
                           cap, W, ring, nwc, C, total);
        NK_LAUNCH_CHECK();
    }
    return NK_OK;
}

}  // extern "C"
