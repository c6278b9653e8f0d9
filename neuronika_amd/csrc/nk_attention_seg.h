// Packed sequences in the fused core: document-masked causal attention, forward and backward (ours; semantics in
// include/neuronika_hip.h).  attention_seg_kernel is nk_attention_band.h's attention_band_kernel with the left edge of every row READ
// from a device array instead of computed from the window: query r of sample b attends to the keys lo_eff[r] .. r,
//   lo_eff[r] = min(r, max(lo[b][r], r - span + 1, 0)),
// `lo` a (B, S) int32 array shared by the heads of a sample, `span` the longest run any row may keep.  Included by nk_norm.hip AFTER
// nk_attention_band.h, whose geometry (ab_padded / ab_ld / ab_extent with W := span), tile helpers (tile_write / tile_flush /
// wave_lds_handover), constants and argument check it uses as they are; the kernel, its args struct and the staging macros are copies,
// for the reason given there (the inventoried units and the band header stay byte for byte).
//
// The clamp is the memory-safety guarantee: whatever `lo` holds, lo_eff[r] lies in [max(0, r - span + 1), r], every tile a wave
// computes lies in the block's staged range [kt0, nt) of the band geometry for (S, span), and the loops run over that range only.
// PRECONDITION (the host layer guarantees it): lo_eff never decreases with r inside a sample.  With an array that breaks it the call
// stays memory-safe - the same tiles are staged, every address is one the band geometry defines - and its results are unspecified.
//
// The walk.  kt0 = 4 js(qb), nt, ld, the extent and the mask-word layout are the band's with W := span.  Per wave, from the array:
//   lo_w = lo_eff[q0] / 32, hi_w = (lo_eff[min(q0 + 31, S - 1)] - 1) / 32 (or -1), hi_3 the same from the block's last row; element
//   mask key >= lo_eff[row] (the CLAMPED row min(r, S - 1) for a padded query).  Three wave-uniform loads (through readfirstlane) and one per lane in the prologue.
//   Tiles in [kt0, lo_w): the forward computes, draws and writes nothing; the backward writes zero tiles of dS and Pd.  (The block
//   stages them all the same: its range is the band's.)
//   contract  the band's: scores written on the tiles a wave computes, -inf at masked positions; dS and Pd defined, and exactly 0 at
//             masked positions, on every 128 x 128 block (qb, j) with js(qb) <= j <= qb; nothing else written or read.  Draws stay at
//             (bh SP + r) SP + k, statistics (B*H, SP, 2).
// Neighbours.  The lazy softmax shift moves for a whole wave when ANY of its 32 rows asks, as in the causal and band kernels, and
// a document's rows are still bit-identical whatever its neighbours hold: a row of a LATER document of the same wave has all its
// keys in the wave's diagonal tile, where it asks unconditionally (its first finite tile), so what it holds changes no decision; at
// every other tile its scores are -inf and a move of the shift leaves it at -1e30; and masked products are exact zeros.
// Specialisations carried: RAGGED, dh 32 / 64 / 128.  Not carried: FULL and the KEEP = false forward (`scores == NULL` is refused).
// dK / dV: the band's strip loop with W := span.  No entry point reads `lo` on the host or allocates: the node can be captured.
#pragma once
#include "nk_attention_band.h"

namespace {

struct SegArgs {
    const float* x1;   // pass-1 operand, flat (B*S) x (H*dh) layout: forward K, backward V
    const float* x2;   // pass-2 operand:                               forward V, backward K
    const float* bq;   // per-query operand:                            forward Q, backward dO
    const float* ctx;  // backward only: the forward output O
    float* out;        // forward O, backward dQ
    float* scores;     // banded (see above): written forward, read backward
    float* ds;         // backward: dS
    float* dropped;    // backward: Pd
    unsigned* maskbits;
    float* stats;      // (B*H, SP, 2)
    int S, H, nqb, ntile;
    int ldx, ldq, ldc, ldo;   // row strides of the projection-layout operands (nk_attention.hip: AttnArgs)
    float scale, keep, dscale, c1;
    unsigned keep_lt;
    int rev;
    unsigned long long seed, offset;
    int assign;
    int SP;            // S rounded up to a multiple of 32
    int W;             // span: the longest run lo_eff .. r any row may keep (<= S)
    const int* lo;     // (B, S): the first key a row may see, before the clamp (as_lo_eff)
    int ld;            // row stride of scores / dS / Pd
    long long ext;     // floats per (sample, head) of each
};

// The clamp that makes every content of `lo` memory-safe: the effective left edge of row r (r < S) lies inside the band of `span`
// keys that the scratch geometry is sized for, and never right of the diagonal.
__device__ __forceinline__ int as_lo_eff(const int* lo, int r, int span) { return min(r, max(max(lo[r], r - span + 1), 0)); }

template <bool BWD, bool MASKED, int OCC, int DH, bool RAGGED>
__global__ __launch_bounds__(AB_NT, OCC) void attention_seg_kernel(const SegArgs p) {
    constexpr int X1_LD = ab_x1_ld(DH), X2_LD = ab_x2_ld(DH);
    constexpr int ND = DH / 32;   // output column tiles
    constexpr int NR = DH / 32;   // float4 per thread and operand of a staged key tile (32 keys x DH)
    constexpr int C4 = DH / 4;    // float4 per key row
    __shared__ __attribute__((aligned(16))) float x1s[2][32 * X1_LD];
    __shared__ __attribute__((aligned(16))) float x2s[2][32 * X2_LD];
    __shared__ __attribute__((aligned(16))) float scr[AB_NT / 64][(BWD ? 2 : 1) * 32 * AB_SCR_LD];  // per wave: tile scratch (backward: dS | Pd)
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane & 31, h = lane >> 5;
    const int seq = nkmma::xcd_chunk(blockIdx.x, gridDim.x);
    const int bh = seq / p.nqb, qb = p.rev ? p.nqb - 1 - seq % p.nqb : seq % p.nqb;
    const long long samp = (long long)(bh / p.H) * p.S, hoff = (long long)(bh % p.H) * DH;
    const long long flat0 = samp * p.ldx + hoff;
    const int q0 = qb * AB_QB + w * 32;
    const bool on = q0 < p.S;  // wave-uniform: the wave has at least one query
    const int SP = p.SP;
    const int nt = min(p.ntile, 4 * qb + 4);                      // one past the last key tile this block stages
    const int kt0 = 4 * (max(0, AB_QB * qb - p.W + 1) / AB_QB);   // the first one: 4 js(qb)
    const int dk = 4 * qb + w;                                    // this wave's diagonal tile (< ntile whenever `on`)
    // the per-wave bounds come from the array: a handful of scalar loads (q0, qb and S are wave-uniform).  Rows end at S - 1: a
    // padded query is a copy of that row
    const int* const lo_s = p.lo + samp;                          // this sample's edges
    const int last_w = min(q0 + 31, p.S - 1), last_3 = min(AB_QB * qb + 127, p.S - 1);
    const int lo_first = __builtin_amdgcn_readfirstlane(as_lo_eff(lo_s, on ? q0 : 0, p.W));
    const int lo_last = __builtin_amdgcn_readfirstlane(as_lo_eff(lo_s, last_w, p.W));
    const int lo_blk = __builtin_amdgcn_readfirstlane(as_lo_eff(lo_s, last_3, p.W));
    const int lo_w = lo_first / 32;                               // its first tile
    // its last tile with a key left of some row's edge - lo_eff never decreases, so the wave's last row has the largest - and the
    // same for the block's last row
    const int hi_w = lo_last > 0 ? (lo_last - 1) / 32 : -1;
    const int hi_3 = lo_blk > 0 ? (lo_blk - 1) / 32 : -1;
    const int left_end = max(kt0, min(hi_3 + 1, 4 * qb));         // [kt0, left_end): edge; [left_end, 4 qb): whole; [4 qb, nt): edge
    const float* x1 = p.x1 + flat0;
    const float* x2 = p.x2 + flat0;

    // ---- cooperative staging of one key tile (32 keys x DH of each operand): NR + NR float4 per thread ------------------
    unsigned goff[NR], goff_last[NR], s1[NR], s2[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int idx = tid + AB_NT * r, key = idx / C4, c4 = idx % C4;
        goff[r] = (unsigned)(key * p.ldx + 4 * c4);
        goff_last[r] = RAGGED ? (unsigned)(min(key, p.S - 1 - 32 * (p.ntile - 1)) * p.ldx + 4 * c4) : goff[r];  // last key tile: rows clamped to S - 1
        s1[r] = (unsigned)((8 * ((key >> 2) & 3) + 4 * (key >> 4) + (key & 3)) * X1_LD + 4 * c4);
        s2[r] = (unsigned)(key * X2_LD + ((4 * c4 + 32 * (key >> 4)) & (DH - 1)));
    }
    // NAMED registers, not arrays (nk_attention.hip: an array written under `if (more)` goes to scratch memory)
    float4 sa0, sa1, sa2, sa3, sb0, sb1, sb2, sb3;
#define AS_STAGE_LOAD(KT)                                                                                        \
    do {                                                                                                         \
        const long long t0_ = (long long)(KT) * 32 * p.ldx;                                                      \
        const bool lt_ = RAGGED && (KT) == p.ntile - 1;   /* wave-uniform */                                     \
        const unsigned g0_ = lt_ ? goff_last[0] : goff[0], g1_ = lt_ ? goff_last[NR > 1 ? 1 : 0] : goff[NR > 1 ? 1 : 0],         \
                       g2_ = lt_ ? goff_last[NR > 2 ? 2 : 0] : goff[NR > 2 ? 2 : 0], g3_ = lt_ ? goff_last[NR > 2 ? 3 : 0] : goff[NR > 2 ? 3 : 0]; \
        sa0 = *reinterpret_cast<const float4*>(x1 + t0_ + g0_);                                                 \
        if constexpr (NR > 1) sa1 = *reinterpret_cast<const float4*>(x1 + t0_ + g1_);                           \
        if constexpr (NR > 2) { sa2 = *reinterpret_cast<const float4*>(x1 + t0_ + g2_);                         \
                                sa3 = *reinterpret_cast<const float4*>(x1 + t0_ + g3_); }                       \
        sb0 = *reinterpret_cast<const float4*>(x2 + t0_ + g0_);                                                 \
        if constexpr (NR > 1) sb1 = *reinterpret_cast<const float4*>(x2 + t0_ + g1_);                           \
        if constexpr (NR > 2) { sb2 = *reinterpret_cast<const float4*>(x2 + t0_ + g2_);                         \
                                sb3 = *reinterpret_cast<const float4*>(x2 + t0_ + g3_); }                       \
        (void)g1_; (void)g2_; (void)g3_;                                                                         \
    } while (0)
#define AS_STAGE_STORE(BUF)                                                                                      \
    do {                                                                                                         \
        *reinterpret_cast<float4*>(&x1s[BUF][s1[0]]) = sa0;                                                      \
        if constexpr (NR > 1) *reinterpret_cast<float4*>(&x1s[BUF][s1[NR > 1 ? 1 : 0]]) = sa1;                   \
        if constexpr (NR > 2) { *reinterpret_cast<float4*>(&x1s[BUF][s1[NR > 2 ? 2 : 0]]) = sa2;                 \
                                *reinterpret_cast<float4*>(&x1s[BUF][s1[NR > 2 ? 3 : 0]]) = sa3; }               \
        *reinterpret_cast<float4*>(&x2s[BUF][s2[0]]) = sb0;                                                      \
        if constexpr (NR > 1) *reinterpret_cast<float4*>(&x2s[BUF][s2[NR > 1 ? 1 : 0]]) = sb1;                   \
        if constexpr (NR > 2) { *reinterpret_cast<float4*>(&x2s[BUF][s2[NR > 2 ? 2 : 0]]) = sb2;                 \
                                *reinterpret_cast<float4*>(&x2s[BUF][s2[NR > 2 ? 3 : 0]]) = sb3; }               \
    } while (0)

    // ---- per-query state ----------------------------------------------------------------------------------------
    const int qrow = on ? q0 + q : 0;                        // row of the scratch tensors (padded rows exist there)
    const int row = RAGGED ? min(qrow, p.S - 1) : qrow;      // row of the projection layout
    float4 bq[DH / 8];  // B operand of pass 1: element (query, dh = 8j + 4h + c)
    {
        const float* b = p.bq + samp * p.ldq + hoff + (long long)row * p.ldq + 4 * h;
#pragma unroll
        for (int j = 0; j < DH / 8; ++j) bq[j] = *reinterpret_cast<const float4*>(b + 8 * j);
    }
    const int lo_row = as_lo_eff(lo_s, row, p.W);   // this row's first key (row < S always)
    float m_run = -1e30f, l_run = 0.f;  // forward: online softmax (shift, sum); backward: the stored shift and 1 / sum
    float dot = 0.f;
    if (BWD) {
        const float2 ms = *reinterpret_cast<const float2*>(p.stats + ((long long)bh * SP + qrow) * 2);
        m_run = ms.x; l_run = ms.y;
        const float* o = p.ctx + samp * p.ldc + hoff + (long long)row * p.ldc + 4 * h;
#pragma unroll
        for (int j = 0; j < DH / 8; ++j) {
            const float4 ov = *reinterpret_cast<const float4*>(o + 8 * j);
            dot += (bq[j].x * ov.x + bq[j].y * ov.y) + (bq[j].z * ov.z + bq[j].w * ov.w);
        }
        dot += __shfl_xor(dot, 32, 64);
        if (MASKED) dot *= p.keep;
    }
    f32x16 oacc[ND];  // out^T tiles: oacc[d] holds dh 32 d .. 32 d + 31 of this lane's query
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;

    // element index of (row q0, key 0) in the banded tensors (geometry of W = span): keys left of 128 js(qb) are never addressed from this row
    const long long rowbase = (long long)bh * p.ext + (long long)(on ? q0 : 0) * p.ld;
    const uint2 key = make_uint2((unsigned)p.seed, (unsigned)(p.seed >> 32));
    // the draws stay indexed in the padded (B*H, SP, SP) tensor: 8 per Philox call
    const unsigned long long ctr0 = (unsigned long long)((((long long)bh * SP + (on ? q0 : 0)) + q) * SP) / 8 + 2 * h + p.offset;
    float* scrw = scr[w];
    float* scrb = scrw + (BWD ? 32 * AB_SCR_LD : 0);
    float4 sn0, sn1, sn2, sn3;   // backward: the score tile of the NEXT iteration, in the coalesced load layout
    unsigned mkn = 0;            // and this row's 32 dropout bits of that tile
    // this wave's mask words: [bh][query tile][kt - kt0][q], ld / 32 key tiles per query tile
    unsigned* const mwave = MASKED ? p.maskbits + (((long long)bh * (SP / 32) + (on ? q0 / 32 : 0)) * (p.ld / 32)) * 32 + q : nullptr;
    const unsigned* mload = mwave;
    const float* sload = p.scores + rowbase + (long long)(lane >> 3) * p.ld + 4 * (lane & 7);
#define AS_SCORES_LOAD(KT)                                                                       \
    do {                                                                                         \
        sn0 = *reinterpret_cast<const float4*>(sload + (KT) * 32);                               \
        sn1 = *reinterpret_cast<const float4*>(sload + (long long)8 * p.ld + (KT) * 32);         \
        sn2 = *reinterpret_cast<const float4*>(sload + (long long)16 * p.ld + (KT) * 32);        \
        sn3 = *reinterpret_cast<const float4*>(sload + (long long)24 * p.ld + (KT) * 32);        \
        if (MASKED) mkn = mload[((KT) - kt0) * 32];                                              \
    } while (0)
#define AS_SCORES_TO_LDS()                                                                       \
    do {                                                                                         \
        float* sw_ = &scrw[(lane >> 3) * AB_SCR_LD + 4 * (lane & 7)];                            \
        *reinterpret_cast<float4*>(sw_) = sn0;                                                   \
        *reinterpret_cast<float4*>(sw_ + 8 * AB_SCR_LD) = sn1;                                   \
        *reinterpret_cast<float4*>(sw_ + 16 * AB_SCR_LD) = sn2;                                  \
        *reinterpret_cast<float4*>(sw_ + 24 * AB_SCR_LD) = sn3;                                  \
    } while (0)
    // kt0 is even: the first staged tile goes to image 0, as `kt & 1` says.  The wave's first score tile is lo_w's: it waits in the
    // wave's own scratch while the block stages the tiles in front of it
    AS_STAGE_LOAD(kt0);
    if (BWD && on) AS_SCORES_LOAD(lo_w);
    AS_STAGE_STORE(0);
    if (BWD && on) AS_SCORES_TO_LDS();
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): every prologue load has landed (nk_attention.hip)
    __syncthreads();

    // two rounds of (edge tiles, whole tiles): the left edge and the tiles behind it, then the diagonal square and nothing - ONE copy of
    // each body (a third copy cost the masked forward and the backward registers they do not have)
#pragma clang loop unroll(disable)
    for (int part = 0; part < 2; ++part) {
        const int e0 = part == 0 ? kt0 : 4 * qb, e1 = part == 0 ? left_end : nt;
        for (int kt = e0; kt < e1; ++kt) {
#define NK_SEG_EDGE true
#include "nk_attention_seg_tile.h"
#undef NK_SEG_EDGE
        }
        if (part == 0) {
            for (int kt = left_end; kt < 4 * qb; ++kt) {
#define NK_SEG_EDGE false
#include "nk_attention_seg_tile.h"
#undef NK_SEG_EDGE
            }
        }
    }
#undef AS_STAGE_LOAD
#undef AS_STAGE_STORE
#undef AS_SCORES_LOAD
#undef AS_SCORES_TO_LDS
    if (!on) return;
    // ---- epilogue: lane (query q, half h) owns dh = 32 d + 8 c + 4 h + {0..3} ----------------------------------------
    float* orow = p.out + samp * p.ldo + hoff + (long long)row * p.ldo + 4 * h;
    const bool qvalid = !RAGGED || qrow < p.S;  // a padded query's copy of row S - 1 stays in the scratch
    if (!BWD) {
        const float inv = 1.f / l_run;
        const float io = MASKED ? inv * p.dscale : inv;
        if (qvalid) {
#pragma unroll
            for (int d = 0; d < ND; ++d)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    *reinterpret_cast<float4*>(orow + 32 * d + 8 * c) =
                        make_float4(oacc[d][4 * c] * io, oacc[d][4 * c + 1] * io, oacc[d][4 * c + 2] * io, oacc[d][4 * c + 3] * io);
        }
        if (h == 0) *reinterpret_cast<float2*>(p.stats + ((long long)bh * SP + qrow) * 2) = make_float2(m_run, inv);
    } else if (qvalid) {
        // every old value is loaded before the first store (a store may alias the next load: a one-walk `+=` serialises)
        float4 old[ND][4];
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                old[d][c] = p.assign ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(orow + 32 * d + 8 * c);
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                *reinterpret_cast<float4*>(orow + 32 * d + 8 * c) =
                    make_float4(old[d][c].x + oacc[d][4 * c], old[d][c].y + oacc[d][4 * c + 1], old[d][c].z + oacc[d][4 * c + 2],
                                old[d][c].w + oacc[d][4 * c + 3]);
    }
}

template <bool BWD, int DH>
int as_launch_dh(nk_device* dev, SegArgs& a, int B, int S, int H, double p, int train, uint64_t seed, uint64_t offset, float scale, int span) {
    a.S = S; a.H = H; a.nqb = (S + AB_QB - 1) / AB_QB; a.SP = ab_padded(S); a.ntile = a.SP / 32;
    a.W = span < S ? span : S;   // (a span that holds every key is the span S: the same geometry, no overflow in r - W)
    a.ld = ab_ld(S, span); a.ext = ab_extent(S, span);
    a.scale = scale; a.c1 = scale * 1.44269504088896341f; a.keep = (float)(1.0 - p); a.dscale = 1.f / (1.f - (float)p);
    a.seed = seed; a.offset = offset;
    a.rev = 1;   // longest walk first, as the causal kernels
    a.keep_lt = nk_keep_threshold(1.0 - p);
    const bool masked = train && p != 0.0;
    if (!BWD && masked)
        if (int rc = nk_refuse_capture(dev, "nk_attention_seg_fwd: the Philox offset (every replay would draw the same mask)",
                                       "run the training-mode dropout eagerly, or capture the evaluation graph")) return rc;
    const dim3 grid((unsigned)(B * H * a.nqb)), block(AB_NT);
    const bool ragged = S % 32 != 0;
    // blocks per CU the register budget is sized for: the causal kernels' (nk_attention.hip, attention_launch_dh)
    // - except the masked DH = 64 forward: the causal one is sized for three blocks and spills 28 - 44 bytes per lane to get there; the
    // band's extra wave-uniform state (three more tile bounds next to the 32 SGPRs of lane masks) pushed that to 44 - 100 bytes, so
    // it is sized for two blocks and spills nothing.  Not measured for this kernel; the causal kernel's own measurement of the
    // trade was 1.36 ms at three blocks against 1.37 - 1.41 ms at two
    constexpr int OCC = DH == 128 ? 1 : (BWD ? 2 : 3);
    constexpr int OCC_M = (!BWD && DH == 64) ? 2 : OCC;   // the MASKED instantiations
    if (ragged) {
        if (masked) hipLaunchKernelGGL((attention_seg_kernel<BWD, true, OCC_M, DH, true>), grid, block, 0, dev->compute, a);
        else hipLaunchKernelGGL((attention_seg_kernel<BWD, false, OCC, DH, true>), grid, block, 0, dev->compute, a);
    } else {
        if (masked) hipLaunchKernelGGL((attention_seg_kernel<BWD, true, OCC_M, DH, false>), grid, block, 0, dev->compute, a);
        else hipLaunchKernelGGL((attention_seg_kernel<BWD, false, OCC, DH, false>), grid, block, 0, dev->compute, a);
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}
template <bool BWD>
int as_launch(nk_device* dev, SegArgs& a, int B, int S, int H, int dh, double p, int train, uint64_t seed, uint64_t offset, float scale,
              int span) {
    if (dh == 32) return as_launch_dh<BWD, 32>(dev, a, B, S, H, p, train, seed, offset, scale, span);
    if (dh == 128) return as_launch_dh<BWD, 128>(dev, a, B, S, H, p, train, seed, offset, scale, span);
    return as_launch_dh<BWD, 64>(dev, a, B, S, H, p, train, seed, offset, scale, span);
}

int as_fwd_impl(nk_device* dev, const float* Q, const float* K, const float* V, const int* lo, int ld_qkv, float* scores, float* stats, uint32_t* mask_bits,
                float* O, int B, int S, int H, int dh, float scale, double p, int train, uint64_t seed, uint64_t offset, int span) {
    const char* what = "nk_attention_seg_fwd";
    NK_CHECK(dev != nullptr, "null device handle");
    NK_CHECK(span > 0, "%s: span must be positive, got %d", what, span);
    if (int rc = ab_check(B, S, H, dh, p, train, scale, span, what)) return rc;
    NK_CHECK(Q && K && V && O, "null pointer in %s", what);
    NK_CHECK(lo != nullptr, "%s needs the (B, S) array of left edges", what);
    NK_CHECK(scores && stats, "%s keeps the scores and the row statistics: there is no inference form, both buffers are needed", what);
    NK_CHECK(mask_bits || !(train && p != 0.0), "%s: dropout is active, the mask_bits buffer is needed", what);
    NK_CHECK(ab_al16(Q) && ab_al16(K) && ab_al16(V) && ab_al16(scores) && ab_al16(O) && ab_al16(stats), "%s needs 16-byte aligned buffers", what);
    NK_CHECK((long long)B * S * ld_qkv < (1ll << 31), "attention: the packed projection layout exceeds 2^31 elements");
    NK_USE(dev);
    nk_prof_start(dev, NK_KERNEL_ATTENTION, ab_flops(B, S, H, dh, span) /* the band's pairs: an upper bound, the edges stay on the device */);
    SegArgs a{};
    a.x1 = K; a.x2 = V; a.bq = Q; a.out = O; a.scores = scores; a.stats = stats; a.maskbits = mask_bits; a.lo = lo;
    a.ldx = ld_qkv; a.ldq = ld_qkv; a.ldc = H * dh; a.ldo = H * dh;
    const int rc = as_launch<false>(dev, a, B, S, H, dh, p, train, seed, offset, scale, span);
    nk_prof_stop(dev);
    return rc;
}

int as_bwd_impl(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO, const float* O, const float* scores,
                const float* stats, const uint32_t* mask_bits, const float* Q, const float* K, const float* V, const int* lo, int ld_qkv, int B, int S, int H,
                int dh, float scale, double p, int train, int assign_dq, int assign_dk, int assign_dv, int span) {
    const char* what = "nk_attention_seg_bwd";
    NK_CHECK(dev != nullptr, "null device handle");
    NK_CHECK(span > 0, "%s: span must be positive, got %d", what, span);
    if (int rc = ab_check(B, S, H, dh, p, train, scale, span, what)) return rc;
    NK_CHECK(dQ && dK && dV && dS && dropped && dO && O && scores && stats && Q && K && V, "null pointer in %s", what);
    NK_CHECK(lo != nullptr, "%s needs the (B, S) array of left edges", what);
    NK_CHECK(mask_bits || !(train && p != 0.0), "%s: dropout is active, the forward's mask_bits are needed", what);
    NK_CHECK(ab_al16(dQ) && ab_al16(dK) && ab_al16(dV) && ab_al16(dS) && ab_al16(dropped) && ab_al16(dO) && ab_al16(O) && ab_al16(scores) &&
                 ab_al16(stats) && ab_al16(Q) && ab_al16(K) && ab_al16(V),
             "%s needs 16-byte aligned buffers", what);
    NK_CHECK((long long)B * S * ld_qkv < (1ll << 31), "attention: the packed projection layout exceeds 2^31 elements");
    NK_USE(dev);
    nk_prof_start(dev, NK_KERNEL_ATTENTION, ab_flops(B, S, H, dh, span) /* the band's pairs: an upper bound, the edges stay on the device */);
    SegArgs a{};
    a.x1 = V; a.x2 = K; a.bq = dO; a.ctx = O; a.out = dQ; a.scores = const_cast<float*>(scores); a.ds = dS; a.dropped = dropped;
    a.stats = const_cast<float*>(stats); a.maskbits = const_cast<uint32_t*>(mask_bits); a.assign = assign_dq ? 1 : 0; a.lo = lo;
    a.ldx = ld_qkv; a.ldq = H * dh; a.ldc = H * dh; a.ldo = ld_qkv;
    int rc = as_launch<true>(dev, a, B, S, H, dh, p, train, 0, 0, scale, span);
    nk_prof_stop(dev);
    if (rc) return rc;
    // dK_bh (+)= dS_bh^T . Q_bh and dV_bh (+)= Pd_bh^T . dO_bh per strip of 128 keys, over the queries of the blocks that staged the
    // strip: j .. min(nqb - 1, j + nb).  A, B and C advanced to (128 j, 128 j); the A operand's row stride is ld - shorter than the
    // logical width SP, which the product never sees: it reads m <= 128 columns of K <= ld rows, and its tile window K ld + 128 is the
    // causal strip's with SP for ld.
    const int d = H * dh, ld = ab_ld(S, span);
    const long long ext = ab_extent(S, span), nb = ((long long)(span < S ? span : S) - 1 + AB_QB - 1) / AB_QB;   // (not ld / 128 - 1: ld is clamped to SP)
    const long long so = (long long)S * d, sq = (long long)S * ld_qkv, po = (long long)H * ext, pi = ext;
    for (int j0 = 0; j0 < S; j0 += AB_QB) {
        const long long last = (long long)j0 + (nb + 1) * AB_QB;   // one past the last query row whose block staged the strip
        const int m = S - j0 < AB_QB ? S - j0 : AB_QB, k = (int)((last < S ? last : S) - j0);
        const long long da = (long long)j0 * ld + j0, dq = (long long)j0 * ld_qkv, dd = (long long)j0 * d;
        rc = nk_sgemm_pair_batched(dev, B, H, 1, 0, m, dh, k, dS + da, ld, po, pi, Q + dq, ld_qkv, sq, dh, assign_dk ? 0.f : 1.f, dK + dq,
                                   ld_qkv, sq, dh, 1, 0, m, dh, k, dropped + da, ld, po, pi, dO + dd, d, so, dh, assign_dv ? 0.f : 1.f,
                                   dV + dq, ld_qkv, sq, dh);
        if (rc) return rc;
    }
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_attention_seg_fwd(nk_device* dev, const float* Q, const float* K, const float* V, const int* lo, float* scores, float* stats,
                         uint32_t* mask_bits, float* O, int B, int S, int H, int dh, int span, float scale, double p, int train, uint64_t seed,
                         uint64_t offset) {
    return as_fwd_impl(dev, Q, K, V, lo, H * dh, scores, stats, mask_bits, O, B, S, H, dh, scale, p, train, seed, offset, span);
}
int nk_attention_seg_bwd(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO, const float* O,
                         const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q, const float* K, const float* V,
                         const int* lo, int B, int S, int H, int dh, int span, float scale, double p, int train, int assign_dq, int assign_dk,
                         int assign_dv) {
    return as_bwd_impl(dev, dQ, dK, dV, dS, dropped, dO, O, scores, stats, mask_bits, Q, K, V, lo, H * dh, B, S, H, dh, scale, p, train,
                       assign_dq, assign_dk, assign_dv, span);
}
int nk_attention_qkv_seg_fwd(nk_device* dev, const float* QKV, const int* lo, float* scores, float* stats, uint32_t* mask_bits, float* O,
                             int B, int S, int H, int dh, int span, float scale, double p, int train, uint64_t seed, uint64_t offset) {
    NK_CHECK(QKV != nullptr, "null pointer in nk_attention_qkv_seg_fwd");
    const int d = H * dh;
    return as_fwd_impl(dev, QKV, QKV + d, QKV + 2 * d, lo, 3 * d, scores, stats, mask_bits, O, B, S, H, dh, scale, p, train, seed, offset, span);
}
int nk_attention_qkv_seg_bwd(nk_device* dev, float* dQKV, float* dS, float* dropped, const float* dO, const float* O, const float* scores,
                             const float* stats, const uint32_t* mask_bits, const float* QKV, const int* lo, int B, int S, int H, int dh,
                             int span, float scale, double p, int train, int assign) {
    NK_CHECK(dQKV && QKV, "null pointer in nk_attention_qkv_seg_bwd");
    const int d = H * dh;
    return as_bwd_impl(dev, dQKV, dQKV + d, dQKV + 2 * d, dS, dropped, dO, O, scores, stats, mask_bits, QKV, QKV + d, QKV + 2 * d, lo, 3 * d, B,
                       S, H, dh, scale, p, train, assign, assign, assign, span);
}

}  // extern "C"
