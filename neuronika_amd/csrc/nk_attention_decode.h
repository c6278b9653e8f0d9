// Incremental decoding (ours; semantics in include/neuronika_hip.h): the key / value cache of a causal attention layer and the
// single-query attention over it, in three forms - plain (H heads of keys), grouped (H query heads over Hkv <= H key / value heads,
// R = H / Hkv query heads per kv head) and sliding-window (query position i attends to the keys max(0, i - W + 1) .. i, on a linear
// cache, position p at slot p, or a rolling one, position p at slot p % cap).  Included by nk_norm.hip, the row-kernel unit.
// Memory-bound, no MFMA: a query row reads its cached keys and values once, straight into registers with 16-byte loads (no LDS
// staging: nothing is shared between waves, cdna_hip_programming.md "GEMV / M <= 16" and "Attention decode").
// The three forms are three kernel SIGNATURES per family - the kernel-argument layout is part of the machine code - around ONE body
// each, included textually and switched by compile-time constants (grouped indexing, window and slots, heads per block, and
// ADEC_PAGED, 0 in this header: the paged signatures around the same bodies are in nk_attention_decode_paged.h):
// nk_attention_decode_body.h for the vector partial kernels, nk_attention_decode_generic_body.h for the generic ones,
// nk_attention_decode_combine_body.h for the combine; the append is one function template with a ring flag, below.  So the bit
// contracts are structural: the grouped result is the plain result, the windowed result at n <= W is both, and the bits of a
// problem depend on (q, its keys / values, n, W, scale) alone.
//   append    a transposing copy (B*T, H*dh) rows -> (B, H, cap, dh), K and V in one launch; 16-byte accesses where dh % 4 == 0 and
//             the strides / pointers allow it (T = float4), scalar otherwise (T = float).  kv_append_kernel: slot start[b] + t,
//             positions >= cap are dropped.  kv_append_ring_kernel: slot (start[b] + t) % cap, every row with a position >= 0 is
//             written.
//   partial   adec_partial_kernel<DH>: one 256-thread block per (problem (b, t, h), chunk of ADEC_CHUNK keys).  The chunk size is
//             a compile-time constant of the dh instantiation - never a function of the CU count, B, H, T, cap or a tuning knob - so
//             the summation order of a problem depends on its own length alone.  A group of dh / 4 lanes owns a key: 16-byte loads,
//             a partial dot of four elements per lane, xor-shuffles inside the group.  A group owns keys g, g + G, g + 2G ... of the
//             chunk (the block reads G consecutive keys = 4 KiB per step), ADEC_KPG = 16 of them; the source issues all 16 key loads
//             and all 16 value loads before the first use - the intent; the compiler settles on 108 VGPRs, so it does not keep all
//             32 float4 live and orders some loads later.  The same group then owns the same keys' values.  The chunk's shift is
//             its exact maximum, so nothing is rescaled inside a chunk.  Keys >= n: the load is redirected to key n - 1 (never a
//             read past the problem's own rows, never a value of the uninitialised tail in a register) and the probability is
//             SELECTED to 0, not multiplied.  A problem of one chunk writes O directly; otherwise (m, l, unnormalised o[dh]) go to
//             the workspace.
//             adec_gqa_partial_kernel<DH>: the decode step is bound by the bytes of K and V, so the heads of a group share ONE read
//             of their chunk: one block per ((b, t, kv head), batch of at most ADEC_GQA_HEADS = 8 query heads of the group, chunk).
//             The block loads its chunk of K and V once and keeps all 16 + 16 float4 per lane in registers; then, head by head,
//             the same statements over those registers.  The bits of a head's result do not depend on R, on the heads that share
//             the block, or on B, T, cap.  A group of more than 8 heads takes ceil(R / 8) blocks (each reads the chunk: 8 heads keep
//             the register budget fixed).  Partials go to the workspace in the per-(b, t, h) layout.
//             (Three heads in flight per pass was measured and not kept: a head costs about 2 us of issue time in its block
//             either way, and the registers go from 176 to 241; four take 272, one wave per SIMD - DESIGN.md.)
//             adw_partial_kernel<DH, NH>: NH = 1 for H == Hkv, NH = ADEC_GQA_HEADS otherwise.  Chunks stay aligned to ABSOLUTE
//             positions: chunk c covers positions [cC, cC + C).  A problem with n = start[b] + t + 1 and lo = max(0, n - W) visits
//             chunks lo / C .. (n - 1) / C only - at most (W + C - 2) / C + 1 of them - and blockIdx.y counts from lo / C: the grid
//             and the workspace are sized by the window, never by the capacity.  Inside a chunk the ownership is by position, so
//             for n <= W (lo = 0) every partial, and the merge, is the plain form's.  Slots: s0 = the slot of position lo (lo % cap
//             on a ring: one scalar remainder per block); position p is at s0 + (p - lo), minus cap if that reaches cap (n - lo <=
//             W <= cap, so one conditional subtract; it never fires on a linear cache).  No table, no dependent load.  Positions of
//             a visited chunk outside [lo, n): the load is redirected to position n - 1 (always in the window), the probability is
//             SELECTED to 0, the chunk's shift is the exact maximum over its in-window keys.  A window inside one chunk writes O.
//   combine   one thread per (problem, column): the problem's partials in ascending chunk order, in the exp2 form of the fused core -
//             M = max m_c, O = sum_c o_c exp2(m_c - M), L = sum_c l_c exp2(m_c - M), O / L.  No atomics, no arrival order.
//             adw_combine_kernel: the same over the problem's visited chunks.
//   generic   any other dh (dh % 4 != 0 included): scalar accesses, a chunk of 256 keys, groups of lpk = the power of two >= dh
//             (64 at most) lanes per key; scores and probabilities through LDS, columns in blocks of lpk.  One block per (b, t, h)
//             in all three forms (the cache head is h / R): nothing is shared; correctness only.
// No atomics, no scratch, nothing derived from the CU count.
#pragma once
#include "nk_common.h"

namespace {

constexpr int ADEC_THREADS = 256;
constexpr int ADEC_KPG = 16;             // keys per lane group and chunk in the vector instantiations: 16 + 16 float4 loads per lane
constexpr int ADEC_CHUNK_GENERIC = 256;  // one key per thread in the generic kernel's softmax
constexpr int ADEC_GQA_HEADS = 8;        // query heads of one group a block serves from one read of the chunk
constexpr float ADEC_LOG2E = 1.44269504088896341f;
// positions stay 31-bit with a chunk to spare: c0 + C never overflows
constexpr long long ADW_MAX_POS = 0x7fffffffLL - 1024;

// keys per chunk: part of the summation order, a constant of the library per head size
constexpr int adec_chunk_of(int dh) {
    return dh == 32 || dh == 64 || dh == 128 ? (ADEC_THREADS / (dh / 4)) * ADEC_KPG : ADEC_CHUNK_GENERIC;
}
// window chunks a problem can touch: a function of W and C only
constexpr long long adw_chunks_of(long long W, int C) { return (W + C - 2) / C + 1; }
bool adec_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// keys query (b, t) ends at: start[b] + t + 1, clipped to cap on a linear cache; <= 0 for a negative start (the output row is then 0)
__device__ __forceinline__ int adec_len(const int* __restrict__ start, int b, int t, int cap, int ring) {
    const long long n = (long long)start[b] + t + 1;
    const long long top = ring ? ADW_MAX_POS : (long long)cap;
    return n > top ? (int)top : (n < 0 ? 0 : (int)n);
}

// slot of a position at most one lap past the end of a ring of cap slots (never fires on a linear cache)
__device__ __forceinline__ int adec_wrap(int sl, int cap) { return sl >= cap ? sl - cap : sl; }

// ---- append: row b*T + t of K / V -> position start[b] + t of every head of sample b.  DV = dh in units of T, ldv = the row stride
// in units of T.  RING: the slot is the position % cap (T <= cap: no two rows of a sample share a slot)
template <typename T, bool RING>
__device__ __forceinline__ void kv_append_body(T* __restrict__ Kc, T* __restrict__ Vc, const T* __restrict__ K, const T* __restrict__ V,
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
        if (pos < 0 || (!RING && pos >= cap)) continue;
        const size_t src = (size_t)row * ldv + (size_t)h * DV + q;
        const size_t dst = (((size_t)b * H + h) * cap + (size_t)(RING ? pos % cap : pos)) * DV + q;
        const T kv = K[src], vv = V[src];
        Kc[dst] = kv;
        Vc[dst] = vv;
    }
}
template <typename T>
__global__ void __launch_bounds__(256) kv_append_kernel(T* __restrict__ Kc, T* __restrict__ Vc, const T* __restrict__ K, const T* __restrict__ V,
                                                        long long ldv, const int* __restrict__ start, int Tn, int H, int DV, int cap,
                                                        long long total) {
    kv_append_body<T, false>(Kc, Vc, K, V, ldv, start, Tn, H, DV, cap, total);
}
template <typename T>
__global__ void __launch_bounds__(256) kv_append_ring_kernel(T* __restrict__ Kc, T* __restrict__ Vc, const T* __restrict__ K,
                                                             const T* __restrict__ V, long long ldv, const int* __restrict__ start, int Tn,
                                                             int H, int DV, int cap, long long total) {
    kv_append_body<T, true>(Kc, Vc, K, V, ldv, start, Tn, H, DV, cap, total);
}

// ---- partial: three signatures around nk_attention_decode_body.h
template <int DH>
__global__ void __launch_bounds__(ADEC_THREADS) adec_partial_kernel(const float* __restrict__ Q, int ldq, const float4* __restrict__ Kc,
                                                                    const float4* __restrict__ Vc, const int* __restrict__ start,
                                                                    float* __restrict__ O, float* __restrict__ ws, int T, int H, int cap,
                                                                    int nchunks, float c1) {
#define ADEC_GROUPED 0
#define ADEC_NH 1
#define ADEC_WINDOW 0
#define ADEC_PAGED 0
#include "nk_attention_decode_body.h"
#undef ADEC_PAGED
#undef ADEC_GROUPED
#undef ADEC_NH
#undef ADEC_WINDOW
}

template <int DH>
__global__ void __launch_bounds__(ADEC_THREADS) adec_gqa_partial_kernel(const float* __restrict__ Q, int ldq, const float4* __restrict__ Kc,
                                                                        const float4* __restrict__ Vc, const int* __restrict__ start,
                                                                        float* __restrict__ O, float* __restrict__ ws, int T, int H, int Hkv,
                                                                        int cap, int nchunks, float c1) {
#define ADEC_GROUPED 1
#define ADEC_NH ADEC_GQA_HEADS
#define ADEC_WINDOW 0
#define ADEC_PAGED 0
#include "nk_attention_decode_body.h"
#undef ADEC_PAGED
#undef ADEC_GROUPED
#undef ADEC_NH
#undef ADEC_WINDOW
}

// NH = 1: H == Hkv, one block per (b, t, h).  NH = ADEC_GQA_HEADS: one block per ((b, t, kv head), batch of at most NH heads).
template <int DH, int NH>
__global__ void __launch_bounds__(ADEC_THREADS) adw_partial_kernel(const float* __restrict__ Q, int ldq, const float4* __restrict__ Kc,
                                                                   const float4* __restrict__ Vc, const int* __restrict__ start,
                                                                   float* __restrict__ O, float* __restrict__ ws, int T, int H, int Hkv,
                                                                   int cap, int W, int ring, int nchunks, float c1) {
#define ADEC_GROUPED 1
#define ADEC_NH NH
#define ADEC_WINDOW 1
#define ADEC_PAGED 0
#include "nk_attention_decode_body.h"
#undef ADEC_PAGED
#undef ADEC_GROUPED
#undef ADEC_NH
#undef ADEC_WINDOW
}

// ---- generic: three signatures around nk_attention_decode_generic_body.h
__global__ void __launch_bounds__(ADEC_THREADS) adec_generic_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ Kc,
                                                                    const float* __restrict__ Vc, const int* __restrict__ start,
                                                                    float* __restrict__ O, float* __restrict__ ws, int T, int H, int dh,
                                                                    int cap, int nchunks, float c1, int lpk) {
#define ADEC_GROUPED 0
#define ADEC_WINDOW 0
#define ADEC_PAGED 0
#include "nk_attention_decode_generic_body.h"
#undef ADEC_PAGED
#undef ADEC_GROUPED
#undef ADEC_WINDOW
}

__global__ void __launch_bounds__(ADEC_THREADS) adec_gqa_generic_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ Kc,
                                                                        const float* __restrict__ Vc, const int* __restrict__ start,
                                                                        float* __restrict__ O, float* __restrict__ ws, int T, int H, int Hkv,
                                                                        int dh, int cap, int nchunks, float c1, int lpk) {
#define ADEC_GROUPED 1
#define ADEC_WINDOW 0
#define ADEC_PAGED 0
#include "nk_attention_decode_generic_body.h"
#undef ADEC_PAGED
#undef ADEC_GROUPED
#undef ADEC_WINDOW
}

__global__ void __launch_bounds__(ADEC_THREADS) adw_generic_kernel(const float* __restrict__ Q, int ldq, const float* __restrict__ Kc,
                                                                   const float* __restrict__ Vc, const int* __restrict__ start,
                                                                   float* __restrict__ O, float* __restrict__ ws, int T, int H, int Hkv, int dh,
                                                                   int cap, int W, int ring, int nchunks, float c1, int lpk) {
#define ADEC_GROUPED 1
#define ADEC_WINDOW 1
#define ADEC_PAGED 0
#include "nk_attention_decode_generic_body.h"
#undef ADEC_PAGED
#undef ADEC_GROUPED
#undef ADEC_WINDOW
}

// ---- combine: the partials of every problem that spans more than one chunk, in chunk order - two signatures around
// nk_attention_decode_combine_body.h
__global__ void __launch_bounds__(256) adec_combine_kernel(const float* __restrict__ ws, const int* __restrict__ start, float* __restrict__ O,
                                                           int T, int H, int dh, int cap, int nchunks, int C, long long total) {
#define ADEC_WINDOW 0
#include "nk_attention_decode_combine_body.h"
#undef ADEC_WINDOW
}

__global__ void __launch_bounds__(256) adw_combine_kernel(const float* __restrict__ ws, const int* __restrict__ start, float* __restrict__ O,
                                                          int T, int H, int dh, int cap, int W, int ring, int nchunks, int C, long long total) {
#define ADEC_WINDOW 1
#include "nk_attention_decode_combine_body.h"
#undef ADEC_WINDOW
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

// One host path for both appends.  `what` names the entry point in every refusal.
int adec_append(nk_device* dev, const char* what, bool ring, float* Kc, float* Vc, const float* K, const float* V, int ld, const int* start,
                int B, int T, int H, int dh, int cap) {
    if (int rc = adec_check(dev, B, T, H, dh, cap, what)) return rc;
    NK_CHECK(Kc != nullptr && Vc != nullptr && K != nullptr && V != nullptr && start != nullptr, "%s: null pointer", what);
    NK_CHECK(ld >= H * dh, "%s: row stride %d is shorter than H*dh = %d", what, ld, H * dh);
    NK_CHECK(!ring || T <= cap, "%s: %d rows per sample would overwrite each other in a ring of %d slots", what, T, cap);
    NK_USE(dev);
    const bool vec = dh % 4 == 0 && ld % 4 == 0 && adec_al16(Kc) && adec_al16(Vc) && adec_al16(K) && adec_al16(V);
    const int DV = vec ? dh / 4 : dh;
    const long long total = (long long)B * T * H * DV;
    const dim3 grid(nk_stream_grid((size_t)total, 256)), block(256);
    float4* kc4 = reinterpret_cast<float4*>(Kc);
    float4* vc4 = reinterpret_cast<float4*>(Vc);
    const float4* k4 = reinterpret_cast<const float4*>(K);
    const float4* v4 = reinterpret_cast<const float4*>(V);
    if (vec && ring)
        hipLaunchKernelGGL((kv_append_ring_kernel<float4>), grid, block, 0, dev->compute, kc4, vc4, k4, v4, (long long)(ld / 4), start, T, H, DV,
                           cap, total);
    else if (vec)
        hipLaunchKernelGGL((kv_append_kernel<float4>), grid, block, 0, dev->compute, kc4, vc4, k4, v4, (long long)(ld / 4), start, T, H, DV, cap,
                           total);
    else if (ring)
        hipLaunchKernelGGL((kv_append_ring_kernel<float>), grid, block, 0, dev->compute, Kc, Vc, K, V, (long long)ld, start, T, H, DV, cap, total);
    else
        hipLaunchKernelGGL((kv_append_kernel<float>), grid, block, 0, dev->compute, Kc, Vc, K, V, (long long)ld, start, T, H, DV, cap, total);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

// One host path for the three forms of the attention: the refusals in the order and the words of each entry point (`what` names it),
// the geometry, the partial or generic launch, the combine.  ADEC_PLAIN looks at none of Hkv, window, ring.
enum AdecForm { ADEC_PLAIN, ADEC_GQA, ADEC_WIN };
int adec_fwd(nk_device* dev, const char* what, AdecForm form, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start,
             float* O, float* workspace, int B, int T, int H, int Hkv, int dh, int cap, int window, int ring, float scale) {
    const bool win = form == ADEC_WIN;
    if (form != ADEC_PLAIN) {
        NK_CHECK(dev != nullptr, "null device handle");
        NK_CHECK(Hkv > 0 && Hkv <= H && H % Hkv == 0, "%s: Hkv must be positive and divide H, got H = %d, Hkv = %d", what, H, Hkv);
    }
    if (form == ADEC_GQA && Hkv == H)  // the plain form's launches, and its name in a refusal
        return adec_fwd(dev, "nk_attention_decode_fwd", ADEC_PLAIN, Q, ldq, Kc, Vc, start, O, workspace, B, T, H, H, dh, cap, 0, 0, scale);
    if (int rc = adec_check(dev, B, T, H, dh, cap, what)) return rc;
    NK_CHECK(Q != nullptr && Kc != nullptr && Vc != nullptr && start != nullptr && O != nullptr && workspace != nullptr, "%s: null pointer", what);
    NK_CHECK(scale > 0.f && scale < INFINITY, "%s: scale must be positive and finite, got %g", what, (double)scale);
    NK_CHECK(ldq >= H * dh, "%s: row stride %d is shorter than H*dh = %d", what, ldq, H * dh);
    if (win) {
        NK_CHECK(window > 0, "%s: window must be positive, got %d", what, window);
        NK_CHECK(!ring || (long long)window + T - 1 <= cap,
                 "%s: a ring of %d slots cannot hold a window of %d keys and %d new rows (window + T - 1 <= cap)", what, cap, window, T);
    }
    const bool vec = dh == 32 || dh == 64 || dh == 128;
    // the instantiation (and with it the chunk size and the summation order) is a function of dh alone: no silent scalar path
    NK_CHECK(!vec || (adec_al16(Kc) && adec_al16(Vc)), "%s: the caches must be 16-byte aligned", what);
    NK_USE(dev);
    // n <= cap on a linear cache, so a window above cap is the window cap: the same lo for every problem, fewer empty blocks
    const int W = window < cap ? window : cap;
    // chunks per problem in the grid and the workspace: by the capacity, or by the window
    const int C = adec_chunk_of(dh), nchunks = win ? (int)adw_chunks_of(W, C) : (cap + C - 1) / C, R = H / Hkv;
    if (win) NK_CHECK(nchunks <= 65535, "%s: a window of %d keys is more than 65534 chunks of %d keys", what, W, C);
    const int P = B * T * H, PB = B * T * Hkv * ((R + ADEC_GQA_HEADS - 1) / ADEC_GQA_HEADS);  // PB <= P < 2^24
    const float c1 = scale * ADEC_LOG2E;
    const dim3 per_head(P, nchunks), per_batch(PB, nchunks), block(ADEC_THREADS);
    const float4* k4 = reinterpret_cast<const float4*>(Kc);
    const float4* v4 = reinterpret_cast<const float4*>(Vc);
#define ADEC_LAUNCH(DH)                                                                                                                       \
    do {                                                                                                                                      \
        if (form == ADEC_PLAIN)                                                                                                               \
            hipLaunchKernelGGL((adec_partial_kernel<DH>), per_head, block, 0, dev->compute, Q, ldq, k4, v4, start, O, workspace, T, H, cap,   \
                               nchunks, c1);                                                                                                  \
        else if (form == ADEC_GQA)                                                                                                            \
            hipLaunchKernelGGL((adec_gqa_partial_kernel<DH>), per_batch, block, 0, dev->compute, Q, ldq, k4, v4, start, O, workspace, T, H,   \
                               Hkv, cap, nchunks, c1);                                                                                        \
        else if (R == 1)                                                                                                                      \
            hipLaunchKernelGGL((adw_partial_kernel<DH, 1>), per_head, block, 0, dev->compute, Q, ldq, k4, v4, start, O, workspace, T, H, Hkv, \
                               cap, W, ring, nchunks, c1);                                                                                    \
        else                                                                                                                                  \
            hipLaunchKernelGGL((adw_partial_kernel<DH, ADEC_GQA_HEADS>), per_batch, block, 0, dev->compute, Q, ldq, k4, v4, start, O,         \
                               workspace, T, H, Hkv, cap, W, ring, nchunks, c1);                                                              \
    } while (0)
    if (dh == 32)
        ADEC_LAUNCH(32);
    else if (dh == 64)
        ADEC_LAUNCH(64);
    else if (dh == 128)
        ADEC_LAUNCH(128);
    else {
        int lpk = 1;
        while (lpk < 64 && lpk < dh) lpk *= 2;
        if (form == ADEC_PLAIN)
            hipLaunchKernelGGL(adec_generic_kernel, per_head, block, 0, dev->compute, Q, ldq, Kc, Vc, start, O, workspace, T, H, dh, cap, nchunks,
                               c1, lpk);
        else if (form == ADEC_GQA)
            hipLaunchKernelGGL(adec_gqa_generic_kernel, per_head, block, 0, dev->compute, Q, ldq, Kc, Vc, start, O, workspace, T, H, Hkv, dh, cap,
                               nchunks, c1, lpk);
        else
            hipLaunchKernelGGL(adw_generic_kernel, per_head, block, 0, dev->compute, Q, ldq, Kc, Vc, start, O, workspace, T, H, Hkv, dh, cap, W,
                               ring, nchunks, c1, lpk);
    }
#undef ADEC_LAUNCH
    NK_LAUNCH_CHECK();
    if (nchunks > 1) {
        const long long total = (long long)P * dh;
        const dim3 grid((unsigned)((total + 255) / 256));
        if (win)
            hipLaunchKernelGGL(adw_combine_kernel, grid, dim3(256), 0, dev->compute, workspace, start, O, T, H, dh, cap, W, ring, nchunks, C, total);
        else
            hipLaunchKernelGGL(adec_combine_kernel, grid, dim3(256), 0, dev->compute, workspace, start, O, T, H, dh, cap, nchunks, C, total);
        NK_LAUNCH_CHECK();
    }
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

size_t nk_attention_decode_window_workspace(int B, int T, int H, int dh, int window) {
    if (B <= 0 || T <= 0 || H <= 0 || dh <= 0 || window <= 0) return 0;
    return (size_t)B * T * H * (size_t)adw_chunks_of(window, adec_chunk_of(dh)) * ((size_t)dh + 2);
}

int nk_kv_cache_append(nk_device* dev, float* Kc, float* Vc, const float* K, const float* V, int ld, const int* start, int B, int T, int H,
                       int dh, int cap) {
    return adec_append(dev, "nk_kv_cache_append", false, Kc, Vc, K, V, ld, start, B, T, H, dh, cap);
}

int nk_kv_cache_append_ring(nk_device* dev, float* Kc, float* Vc, const float* K, const float* V, int ld, const int* start, int B, int T,
                            int H, int dh, int cap) {
    return adec_append(dev, "nk_kv_cache_append_ring", true, Kc, Vc, K, V, ld, start, B, T, H, dh, cap);
}

int nk_attention_decode_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, float* O,
                            float* workspace, int B, int T, int H, int dh, int cap, float scale) {
    return adec_fwd(dev, "nk_attention_decode_fwd", ADEC_PLAIN, Q, ldq, Kc, Vc, start, O, workspace, B, T, H, H, dh, cap, 0, 0, scale);
}

int nk_attention_decode_gqa_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, float* O,
                                float* workspace, int B, int T, int H, int Hkv, int dh, int cap, float scale) {
    return adec_fwd(dev, "nk_attention_decode_gqa_fwd", ADEC_GQA, Q, ldq, Kc, Vc, start, O, workspace, B, T, H, Hkv, dh, cap, 0, 0, scale);
}

int nk_attention_decode_window_fwd(nk_device* dev, const float* Q, int ldq, const float* Kc, const float* Vc, const int* start, float* O,
                                   float* workspace, int B, int T, int H, int Hkv, int dh, int cap, int window, int ring, float scale) {
    return adec_fwd(dev, "nk_attention_decode_window_fwd", ADEC_WIN, Q, ldq, Kc, Vc, start, O, workspace, B, T, H, Hkv, dh, cap, window, ring,
                    scale);
}

}  // extern "C"
