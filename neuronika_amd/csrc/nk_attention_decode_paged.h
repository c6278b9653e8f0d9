// Paged key / value cache (ours; semantics in include/neuronika_hip.h, "paged decoding"): the keys and values of every sequence live
// in fixed-size pages of two pools, Kp / Vp (num_pages, Hkv, page, dh), and a device table int32 (B, max_pages) says which page holds
// which positions of which sample: position p of sample b is in page table[b*max_pages + p / page] at slot p % page.  Included by
// nk_norm.hip after nk_attention_decode.h, whose constants, bodies, combine kernels and host geometry it uses.
//   append    kv_pages_append_kernel<T>: kv_append_kernel with the page lookup in front of the store.  Rows with a position < 0 or
//             >= cap_v = max_pages * page, and rows whose table entry is outside [0, num_pages), are dropped.
//   copy      kv_pages_copy_kernel<T>: whole pages src[i] -> dst[i], every head, K and V, one streaming launch (what a fork that
//             diverges inside a shared page needs).  A pair with an id outside the pool is dropped.
//   partial   adp_partial_kernel<DH, NH> (all keys) and adpw_partial_kernel<DH, NH> (sliding window, linear positions): new SIGNATURES
//             around nk_attention_decode_body.h with its fifth switch ADEC_PAGED = 1, NH in {1, ADEC_GQA_HEADS} as adw_partial_kernel
//             has them.  Everything but "where a position lives" is the text of the contiguous kernels, so on equal keys the bits are
//             theirs: the summation order is by position, never by page.
//             Table reads: a lane looks up the entry of each of its 16 keys - AFTER the redirect of a position that does not count to
//             position n - 1, so an entry past the sequence's own pages or below its window is never read - and the source issues the
//             16 table reads before the 16 + 16 key / value loads: a chunk pays one dependent-load latency, not sixteen.  The entry is
//             clamped into the pool with one unsigned min (a no-op for a valid entry): a wrong table gives wrong numbers, never an
//             access outside the two allocations.  Pool offsets are 32-bit in units of 16 bytes (the host path refuses a larger pool).
//             What the compiler made of it (hipcc -O3, gfx950; profiles/attention_decode_paged_isa.md): the redirect makes the entry's
//             index a per-lane value, so the 16 table reads are VECTOR loads (global_load_dword), never scalar ones.  The eight-head
//             forms (170 - 176 VGPRs, the twins' counts) issue all 16 ahead of the 32 key / value loads.  The one-head forms (100
//             VGPRs without a window, 117 - 119 with one: four waves per SIMD like their twins) issue 8, then the other 8 among the
//             first key loads: two dependent-load latencies per chunk.  Scratch is 0 bytes everywhere.
//   generic   adp_generic_kernel / adpw_generic_kernel: the generic body with ADEC_PAGED = 1, a lookup per key row; correctness only.
//   combine   none of its own: adec_combine_kernel with cap := cap_v, adw_combine_kernel with ring = 0.
// No atomics, no scratch, nothing derived from the CU count.
#pragma once
#include "nk_attention_decode.h"

namespace {

// ---- append: row b*T + t of K / V -> position start[b] + t of every head of sample b, through the table.  DV = dh in units of T
template <typename T>
__global__ void __launch_bounds__(256) kv_pages_append_kernel(T* __restrict__ Kp, T* __restrict__ Vp, const T* __restrict__ K,
                                                              const T* __restrict__ V, long long ldv, const int* __restrict__ start,
                                                              const int* __restrict__ table, int max_pages, int Tn, int H, int DV, int psh,
                                                              int num_pages, long long total) {
    const long long step = (long long)gridDim.x * 256;
    const long long cap = (long long)max_pages << psh;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const int q = (int)(i % DV);
        const long long rh = i / DV;
        const int h = (int)(rh % H);
        const long long row = rh / H;
        const int b = (int)(row / Tn), t = (int)(row % Tn);
        const long long pos = (long long)start[b] + t;
        if (pos < 0 || pos >= cap) continue;
        const int pg = table[(size_t)b * max_pages + (size_t)(pos >> psh)];
        if ((unsigned)pg >= (unsigned)num_pages) continue;
        const size_t src = (size_t)row * ldv + (size_t)h * DV + q;
        const size_t dst = ((((size_t)pg * H + h) << psh) + (size_t)(pos & ((1ll << psh) - 1))) * DV + q;
        const T kv = K[src], vv = V[src];
        Kp[dst] = kv;
        Vp[dst] = vv;
    }
}

// ---- copy: page src[i] -> page dst[i], PE = Hkv * page * dh elements in units of T per page.  The pools are read and written: no
// __restrict__ on them
template <typename T>
__global__ void __launch_bounds__(256) kv_pages_copy_kernel(T* Kp, T* Vp, const int* __restrict__ src, const int* __restrict__ dst,
                                                            long long PE, int num_pages, long long total) {
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const long long pr = i / PE, e = i % PE;
        const int s = src[pr], d = dst[pr];
        if ((unsigned)s >= (unsigned)num_pages || (unsigned)d >= (unsigned)num_pages || s == d) continue;
        const T kv = Kp[(size_t)s * PE + e], vv = Vp[(size_t)s * PE + e];
        Kp[(size_t)d * PE + e] = kv;
        Vp[(size_t)d * PE + e] = vv;
    }
}

// ---- partial: two signatures around nk_attention_decode_body.h.  cap is the virtual capacity max_pages << psh, np1 = num_pages - 1
template <int DH, int NH>
__global__ void __launch_bounds__(ADEC_THREADS) adp_partial_kernel(const float* __restrict__ Q, int ldq, const float4* __restrict__ Kc,
                                                                   const float4* __restrict__ Vc, const int* __restrict__ start,
                                                                   const int* __restrict__ table, float* __restrict__ O,
                                                                   float* __restrict__ ws, int T, int H, int Hkv, int cap, int max_pages,
                                                                   int psh, unsigned np1, int nchunks, float c1) {
#define ADEC_GROUPED 1
#define ADEC_NH NH
#define ADEC_WINDOW 0
#define ADEC_PAGED 1
#include "nk_attention_decode_body.h"
#undef ADEC_GROUPED
#undef ADEC_NH
#undef ADEC_WINDOW
#undef ADEC_PAGED
}

template <int DH, int NH>
__global__ void __launch_bounds__(ADEC_THREADS) adpw_partial_kernel(const float* __restrict__ Q, int ldq, const float4* __restrict__ Kc,
                                                                    const float4* __restrict__ Vc, const int* __restrict__ start,
                                                                    const int* __restrict__ table, float* __restrict__ O,
                                                                    float* __restrict__ ws, int T, int H, int Hkv, int cap, int max_pages,
                                                                    int psh, unsigned np1, int W, int nchunks, float c1) {
    constexpr int ring = 0;  // pages hold linear positions
#define ADEC_GROUPED 1
#define ADEC_NH NH
#define ADEC_WINDOW 1
#define ADEC_PAGED 1
#include "nk_attention_decode_body.h"
#undef ADEC_GROUPED
#undef ADEC_NH
#undef ADEC_WINDOW
#undef ADEC_PAGED
}

// ---- generic: two signatures around nk_attention_decode_generic_body.h
__global__ void __launch_bounds__(ADEC_THREADS) adp_generic_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ Kc,
                                                                   const float* __restrict__ Vc, const int* __restrict__ start,
                                                                   const int* __restrict__ table, float* __restrict__ O,
                                                                   float* __restrict__ ws, int T, int H, int Hkv, int dh, int cap,
                                                                   int max_pages, int psh, unsigned np1, int nchunks, float c1, int lpk) {
#define ADEC_GROUPED 1
#define ADEC_WINDOW 0
#define ADEC_PAGED 1
#include "nk_attention_decode_generic_body.h"
#undef ADEC_GROUPED
#undef ADEC_WINDOW
#undef ADEC_PAGED
}

__global__ void __launch_bounds__(ADEC_THREADS) adpw_generic_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ Kc,
                                                                    const float* __restrict__ Vc, const int* __restrict__ start,
                                                                    const int* __restrict__ table, float* __restrict__ O,
                                                                    float* __restrict__ ws, int T, int H, int Hkv, int dh, int cap,
                                                                    int max_pages, int psh, unsigned np1, int W, int nchunks, float c1,
                                                                    int lpk) {
    constexpr int ring = 0;  // pages hold linear positions
#define ADEC_GROUPED 1
#define ADEC_WINDOW 1
#define ADEC_PAGED 1
#include "nk_attention_decode_generic_body.h"
#undef ADEC_GROUPED
#undef ADEC_WINDOW
#undef ADEC_PAGED
}

// page = 1 << shift with 16 <= page, or -1
int adp_shift(int page) {
    if (page < 16 || (page & (page - 1)) != 0) return -1;
    int s = 4;
    while ((1 << s) != page) ++s;
    return s;
}

// the geometry refusals both paged entry points share, in the order of the contiguous host path: the device, then the sizes (the
// page and the table first: the virtual capacity max_pages * page is made of them), then adec_check on the virtual capacity
int adp_check(nk_device* dev, const char* what, int B, int T, int H, int dh, int page, int max_pages, int num_pages) {
    NK_CHECK(dev != nullptr, "null device handle");
    NK_CHECK(adp_shift(page) >= 0, "%s: page must be a power of two and at least 16, got %d", what, page);
    NK_CHECK(max_pages > 0, "%s: max_pages must be positive, got %d", what, max_pages);
    NK_CHECK(num_pages > 0, "%s: num_pages must be positive, got %d", what, num_pages);
    NK_CHECK((long long)max_pages * page <= ADW_MAX_POS, "%s: max_pages * page = %lld positions must stay below 2^31 - 1024", what,
             (long long)max_pages * page);
    return adec_check(dev, B, T, H, dh, max_pages * page, what);
}

// One host path for the paged append, beside adec_append.
int adp_append(nk_device* dev, const char* what, float* Kp, float* Vp, const float* K, const float* V, int ld, const int* start,
               const int* table, int max_pages, int B, int T, int H, int dh, int page, int num_pages) {
    if (int rc = adp_check(dev, what, B, T, H, dh, page, max_pages, num_pages)) return rc;
    NK_CHECK(Kp != nullptr && Vp != nullptr && K != nullptr && V != nullptr && start != nullptr, "%s: null pointer", what);
    NK_CHECK(table != nullptr, "%s: null table", what);
    NK_CHECK(ld >= H * dh, "%s: row stride %d is shorter than H*dh = %d", what, ld, H * dh);
    NK_USE(dev);
    const bool vec = dh % 4 == 0 && ld % 4 == 0 && adec_al16(Kp) && adec_al16(Vp) && adec_al16(K) && adec_al16(V);
    const int DV = vec ? dh / 4 : dh, psh = adp_shift(page);
    const long long total = (long long)B * T * H * DV;
    const dim3 grid(nk_stream_grid((size_t)total, 256)), block(256);
    if (vec)
        hipLaunchKernelGGL((kv_pages_append_kernel<float4>), grid, block, 0, dev->compute, reinterpret_cast<float4*>(Kp),
                           reinterpret_cast<float4*>(Vp), reinterpret_cast<const float4*>(K), reinterpret_cast<const float4*>(V),
                           (long long)(ld / 4), start, table, max_pages, T, H, DV, psh, num_pages, total);
    else
        hipLaunchKernelGGL((kv_pages_append_kernel<float>), grid, block, 0, dev->compute, Kp, Vp, K, V, (long long)ld, start, table, max_pages, T,
                           H, DV, psh, num_pages, total);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int adp_copy(nk_device* dev, const char* what, float* Kp, float* Vp, const int* src, const int* dst, int n, int H, int dh, int page,
             int num_pages) {
    NK_CHECK(dev != nullptr, "null device handle");
    NK_CHECK(n >= 0 && H > 0 && dh > 0, "%s: n must not be negative and H, dh must be positive, got %d, %d, %d", what, n, H, dh);
    NK_CHECK(adp_shift(page) >= 0, "%s: page must be a power of two and at least 16, got %d", what, page);
    NK_CHECK(num_pages > 0, "%s: num_pages must be positive, got %d", what, num_pages);
    NK_CHECK((long long)H * dh <= 0x7fffffffLL, "%s: H*dh must fit 31 bits", what);
    if (n == 0) return NK_OK;
    NK_CHECK(Kp != nullptr && Vp != nullptr && src != nullptr && dst != nullptr, "%s: null pointer", what);
    NK_USE(dev);
    const bool vec = dh % 4 == 0 && adec_al16(Kp) && adec_al16(Vp);
    const long long PE = (long long)H * page * (vec ? dh / 4 : dh), total = PE * n;
    const dim3 grid(nk_stream_grid((size_t)total, 256)), block(256);
    if (vec)
        hipLaunchKernelGGL((kv_pages_copy_kernel<float4>), grid, block, 0, dev->compute, reinterpret_cast<float4*>(Kp),
                           reinterpret_cast<float4*>(Vp), src, dst, PE, num_pages, total);
    else
        hipLaunchKernelGGL((kv_pages_copy_kernel<float>), grid, block, 0, dev->compute, Kp, Vp, src, dst, PE, num_pages, total);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

// One host path for the paged attention, beside adec_fwd: the same refusals in the same order and words, the same expressions for
// the geometry with cap := cap_v, the contiguous forms' combine kernels.  window == 0: every key; window > 0: the sliding window.
int adp_fwd(nk_device* dev, const char* what, const float* Q, int ldq, const float* Kp, const float* Vp, const int* start, const int* table,
            int max_pages, float* O, float* workspace, int B, int T, int H, int Hkv, int dh, int page, int num_pages, int window, float scale) {
    NK_CHECK(dev != nullptr, "null device handle");
    NK_CHECK(Hkv > 0 && Hkv <= H && H % Hkv == 0, "%s: Hkv must be positive and divide H, got H = %d, Hkv = %d", what, H, Hkv);
    if (int rc = adp_check(dev, what, B, T, H, dh, page, max_pages, num_pages)) return rc;
    NK_CHECK(Q != nullptr && Kp != nullptr && Vp != nullptr && start != nullptr && O != nullptr && workspace != nullptr, "%s: null pointer", what);
    NK_CHECK(table != nullptr, "%s: null table", what);
    NK_CHECK(scale > 0.f && scale < INFINITY, "%s: scale must be positive and finite, got %g", what, (double)scale);
    NK_CHECK(ldq >= H * dh, "%s: row stride %d is shorter than H*dh = %d", what, ldq, H * dh);
    NK_CHECK(window >= 0, "%s: window must not be negative, got %d", what, window);
    const bool vec = dh == 32 || dh == 64 || dh == 128, win = window > 0;
    NK_CHECK(!vec || (adec_al16(Kp) && adec_al16(Vp)), "%s: the caches must be 16-byte aligned", what);
    // the vector kernels keep a key's pool offset in 32 bits, in units of 16 bytes
    NK_CHECK(!vec || (long long)num_pages * Hkv * page * (dh / 4) <= 0xffffffffLL, "%s: a pool of %d pages is more than 2^32 16-byte units", what,
             num_pages);
    NK_USE(dev);
    const int cap = max_pages * page, psh = adp_shift(page);
    const unsigned np1 = (unsigned)num_pages - 1u;
    const int W = window < cap ? window : cap;
    const int C = adec_chunk_of(dh), nchunks = win ? (int)adw_chunks_of(W, C) : (cap + C - 1) / C, R = H / Hkv;
    if (win) NK_CHECK(nchunks <= 65535, "%s: a window of %d keys is more than 65534 chunks of %d keys", what, W, C);
    const int P = B * T * H, PB = B * T * Hkv * ((R + ADEC_GQA_HEADS - 1) / ADEC_GQA_HEADS);  // PB <= P < 2^24
    const float c1 = scale * ADEC_LOG2E;
    const dim3 per_head(P, nchunks), per_batch(PB, nchunks), block(ADEC_THREADS);
    const float4* k4 = reinterpret_cast<const float4*>(Kp);
    const float4* v4 = reinterpret_cast<const float4*>(Vp);
#define ADP_LAUNCH(DH)                                                                                                                        \
    do {                                                                                                                                      \
        if (!win && R == 1)                                                                                                                   \
            hipLaunchKernelGGL((adp_partial_kernel<DH, 1>), per_head, block, 0, dev->compute, Q, ldq, k4, v4, start, table, O, workspace, T,  \
                               H, Hkv, cap, max_pages, psh, np1, nchunks, c1);                                                                \
        else if (!win)                                                                                                                        \
            hipLaunchKernelGGL((adp_partial_kernel<DH, ADEC_GQA_HEADS>), per_batch, block, 0, dev->compute, Q, ldq, k4, v4, start, table, O,  \
                               workspace, T, H, Hkv, cap, max_pages, psh, np1, nchunks, c1);                                                  \
        else if (R == 1)                                                                                                                      \
            hipLaunchKernelGGL((adpw_partial_kernel<DH, 1>), per_head, block, 0, dev->compute, Q, ldq, k4, v4, start, table, O, workspace, T, \
                               H, Hkv, cap, max_pages, psh, np1, W, nchunks, c1);                                                             \
        else                                                                                                                                  \
            hipLaunchKernelGGL((adpw_partial_kernel<DH, ADEC_GQA_HEADS>), per_batch, block, 0, dev->compute, Q, ldq, k4, v4, start, table, O, \
                               workspace, T, H, Hkv, cap, max_pages, psh, np1, W, nchunks, c1);                                               \
    } while (0)
    if (dh == 32)
        ADP_LAUNCH(32);
    else if (dh == 64)
        ADP_LAUNCH(64);
    else if (dh == 128)
        ADP_LAUNCH(128);
    else {
        int lpk = 1;
        while (lpk < 64 && lpk < dh) lpk *= 2;
        if (!win)
            hipLaunchKernelGGL(adp_generic_kernel, per_head, block, 0, dev->compute, Q, ldq, Kp, Vp, start, table, O, workspace, T, H, Hkv, dh, cap,
                               max_pages, psh, np1, nchunks, c1, lpk);
        else
            hipLaunchKernelGGL(adpw_generic_kernel, per_head, block, 0, dev->compute, Q, ldq, Kp, Vp, start, table, O, workspace, T, H, Hkv, dh, cap,
                               max_pages, psh, np1, W, nchunks, c1, lpk);
    }
#undef ADP_LAUNCH
    NK_LAUNCH_CHECK();
    if (nchunks > 1) {
        const long long total = (long long)P * dh;
        const dim3 grid((unsigned)((total + 255) / 256));
        if (win)
            hipLaunchKernelGGL(adw_combine_kernel, grid, dim3(256), 0, dev->compute, workspace, start, O, T, H, dh, cap, W, 0, nchunks, C, total);
        else
            hipLaunchKernelGGL(adec_combine_kernel, grid, dim3(256), 0, dev->compute, workspace, start, O, T, H, dh, cap, nchunks, C, total);
        NK_LAUNCH_CHECK();
    }
    return NK_OK;
}

}  // namespace

extern "C" {

size_t nk_attention_decode_paged_workspace(int B, int T, int H, int dh, int max_pages, int page, int window) {
    if (adp_shift(page) < 0 || max_pages <= 0 || window < 0 || (long long)max_pages * page > ADW_MAX_POS) return 0;
    return window > 0 ? nk_attention_decode_window_workspace(B, T, H, dh, window)
                      : nk_attention_decode_workspace(B, T, H, dh, max_pages * page);
}

int nk_kv_pages_append(nk_device* dev, float* Kp, float* Vp, const float* K, const float* V, int ld, const int* start, const int* table,
                       int max_pages, int B, int T, int H, int dh, int page, int num_pages) {
    return adp_append(dev, "nk_kv_pages_append", Kp, Vp, K, V, ld, start, table, max_pages, B, T, H, dh, page, num_pages);
}

int nk_kv_pages_copy(nk_device* dev, float* Kp, float* Vp, const int* src, const int* dst, int n, int H, int dh, int page, int num_pages) {
    return adp_copy(dev, "nk_kv_pages_copy", Kp, Vp, src, dst, n, H, dh, page, num_pages);
}

int nk_attention_decode_paged_fwd(nk_device* dev, const float* Q, int ldq, const float* Kp, const float* Vp, const int* start,
                                  const int* table, int max_pages, float* O, float* workspace, int B, int T, int H, int Hkv, int dh, int page,
                                  int num_pages, int window, float scale) {
    return adp_fwd(dev, "nk_attention_decode_paged_fwd", Q, ldq, Kp, Vp, start, table, max_pages, O, workspace, B, T, H, Hkv, dh, page,
                   num_pages, window, scale);
}

}  // extern "C"
