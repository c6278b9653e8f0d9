// Attention with a left edge per row in the fused core, forward and backward (ours; semantics in include/neuronika_hip.h).
// attention_band_kernel is the causal instantiation of nk_attention.hip's attention_kernel - 256 threads, 128 queries per block, key
// tiles of 32, the transposed score tile in registers between the two mfma_f32_32x32x2f32 products, online softmax in the exp2 domain
// with the lazy shift, two Philox calls per lane and tile packed to one bit per score, -inf stored at masked scores; the same tile body,
// nk_attention_tile.h, and the helpers of nk_attention_core.h - with a walk that also skips the key tiles LEFT of the rows' edges:
// O(S W) work and O(S W) scratch.  Two forms of one kernel (template parameter SEG):
//   band  sliding window: query r attends to the keys max(0, r - W + 1) .. r, the edge computed from the window W.
//   seg   packed sequences, document-masked causal attention: query r of sample b attends to the keys lo_eff[r] .. r,
//           lo_eff[r] = min(r, max(lo[b][r], r - span + 1, 0)),
//         the edge READ from `lo`, a (B, S) int32 device array shared by the heads of a sample; `span` is the longest run any row may
//         keep and takes the window's place (W := span) in everything below.
// Included by nk_norm.hip.
//
// The walk.  k_lo(qb) = max(0, 128 qb - W + 1), js(qb) = k_lo(qb) / 128.
//   block qb  stages key tiles kt0 = 4 js(qb) .. min(ntile, 4 qb + 4) - 1 and nothing else.
//   wave w    (rows r0 = 128 qb + 32 w ..) computes tiles lo_w = max(0, r0 - W + 1) / 32 <= kt <= dk = 4 qb + w.  Tiles kt <= hi_w =
//             floor((min(r0 + 31, S - 1) - W) / 32) hold keys k <= r - W of some row (one such tile when W % 32 < 2, two otherwise);
//             tile dk is the causal diagonal tile; a window below 32 keys makes both edges meet in one tile.
//   loops     two rounds of (edge tiles, whole tiles): [kt0, min(hi_3 + 1, 4 qb)), the left edge, runs the body under the per-wave
//             predicate and element masks (EDGE); the tiles up to 4 qb are whole for every wave and run the body as it is (see FULL
//             in nk_attention.hip for why that matters); the second round is the diagonal square [4 qb, nt), EDGE again, and no
//             whole tiles.  One textual copy of each body.  A staged tile a wave does not compute: the forward writes nothing, the
//             backward writes zero tiles of dS and Pd.
//   contract  dS and Pd are defined, and exactly 0 at masked positions, on every 128 x 128 block (qb, j) with js(qb) <= j <= qb;
//             scores are written on the computed tiles (-inf at masked positions); nothing else is written or read.
// Banded scratch.  scores, dS and Pd are addressed as head_base + r * ld + k with ld = min(SP, 128 (ceil((W - 1) / 128) + 1)): the
// plain (SP, SP) matrix with a row stride shorter than its width.  A row's touched columns start at 128 js(qb) - which never
// decreases with r - and span at most ld, so no two touched elements share an address; ld is a multiple of 128 (or SP, of 32), so
// the 16-byte tile stores survive.  Per head: (SP - 1) ld + SP floats (nk_attention_band_scratch).  Mask words: [bh][SP / 32 query
// tiles][ld / 32 key tiles, counted from kt0 of the query tile's block][32 queries] (nk_attention_band_mask_words per head).
// Statistics stay (B*H, SP, 2).  W >= S: ld = SP, kt0 = 0, no left edge - the causal layouts and, tile for tile, the causal arithmetic.
// Dropout draws keep their position in the PADDED S x S index space, (bh SP + r) SP + k.
// The seg form.  The clamp is the memory-safety guarantee: whatever `lo` holds, lo_eff[r] lies in [max(0, r - span + 1), r], every tile a
// wave computes lies in the block's staged range [kt0, nt) of the band geometry for (S, span), and the loops run over that range only.
// PRECONDITION (the host layer guarantees it): lo_eff never decreases with r inside a sample.  With an array that breaks it the call
// stays memory-safe - the same tiles are staged, every address is one the band geometry defines - and its results are unspecified.
//   walk      kt0, nt, ld, the extent and the mask-word layout are the band's.  Per wave, from the array: lo_w = lo_eff[q0] / 32,
//             hi_w = (lo_eff[min(q0 + 31, S - 1)] - 1) / 32 (or -1), hi_3 the same from the block's last row; element mask
//             key >= lo_eff[row] (the CLAMPED row min(r, S - 1) for a padded query).  Three wave-uniform loads (through readfirstlane)
//             and one per lane in the prologue.  Tiles in [kt0, lo_w): the forward computes, draws and writes nothing; the backward
//             writes zero tiles of dS and Pd.  (The block stages them all the same: its range is the band's.)
//   contract  the band's.  No entry point reads `lo` on the host or allocates: the node can be captured.
// Neighbours.  The lazy softmax shift moves for a whole wave when ANY of its 32 rows asks, as in the causal kernels, and a document's
// rows are still bit-identical whatever its neighbours hold: a row of a LATER document of the same wave has all its keys in the wave's
// diagonal tile, where it asks unconditionally (its first finite tile), so what it holds changes no decision; at every other tile its
// scores are -inf and a move of the shift leaves it at -1e30; and masked products are exact zeros.
// Specialisations carried: RAGGED (S % 32 != 0), dh 32 / 64 / 128.  Not carried: FULL (S % 128 == 0 without the `on` test) and the
// KEEP = false inference forward (`scores == NULL` is refused) - neither was measured to pay here, and every instantiation has to be
// reached by a test.
// dK / dV: strip_products over the queries of blocks j .. min(nqb - 1, j + ceil((W - 1) / 128)).
#pragma once
#include <string>

#include "nk_attention_core.h"

namespace {

// the geometry, on the host: the one source of the layout (exported below)
constexpr int ab_padded(int S) { return (S + 31) / 32 * 32; }
inline int ab_ld(int S, int W) {
    const long long SP = ab_padded(S), nb = ((long long)W - 1 + 127) / 128;   // blocks left of a block's own that its band reaches
    const long long ld = 128 * (nb + 1);
    return (int)(ld < SP ? ld : SP);
}
inline long long ab_extent(int S, int W) { return (long long)(ab_padded(S) - 1) * ab_ld(S, W) + ab_padded(S); }

// The kernel's arguments: AttnArgs (its `scores` banded, see above) and the band geometry.  The seg form carries the edge array too
template <bool SEG> struct BandArgs;
template <> struct BandArgs<false> : AttnArgs {
    int W;             // the window
    int ld;            // row stride of scores / dS / Pd
    long long ext;     // floats per (sample, head) of each
};
template <> struct BandArgs<true> : AttnArgs {
    int W;             // span: the longest run lo_eff .. r any row may keep (<= S)
    const int* lo;     // (B, S): the first key a row may see, before the clamp (as_lo_eff)
    int ld;
    long long ext;
};

// The clamp that makes every content of `lo` memory-safe: the effective left edge of row r (r < S) lies inside the band of `span`
// keys that the scratch geometry is sized for, and never right of the diagonal.
__device__ __forceinline__ int as_lo_eff(const int* lo, int r, int span) { return min(r, max(max(lo[r], r - span + 1), 0)); }

// The prologue and the epilogue are attention_kernel's, statement for statement: as force-inlined functions shared by both kernels they
// moved the register allocation and the instruction count of nearly every instantiation of both.
#define NK_ATT_LEFT true   // rows have a left edge (nk_attention_tile.h)
template <bool BWD, bool MASKED, int OCC, int DH, bool RAGGED, bool SEG>
__global__ __launch_bounds__(A_NT, OCC) void attention_band_kernel(const BandArgs<SEG> p) {
    constexpr bool KEEP = true;   // (there is no inference form)
    constexpr int X1_LD = x1_ld(DH), X2_LD = x2_ld(DH);
    constexpr int ND = DH / 32;   // output column tiles
    constexpr int NR = DH / 32;   // float4 per thread and operand of a staged key tile (32 keys x DH)
    constexpr int C4 = DH / 4;    // float4 per key row
    __shared__ __attribute__((aligned(16))) float x1s[2][32 * X1_LD];
    __shared__ __attribute__((aligned(16))) float x2s[2][32 * X2_LD];
    __shared__ __attribute__((aligned(16))) float scr[A_NT / 64][(BWD ? 2 : 1) * 32 * SCR_LD];  // per wave: tile scratch (backward: dS | Pd)
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = lane & 31, h = lane >> 5;
    const int seq = nkmma::xcd_chunk(blockIdx.x, gridDim.x);
    const int bh = seq / p.nqb, qb = p.rev ? p.nqb - 1 - seq % p.nqb : seq % p.nqb;
    const long long samp = (long long)(bh / p.H) * p.S, hoff = (long long)(bh % p.H) * DH;
    const long long flat0 = samp * p.ldx + hoff;
    const int q0 = qb * A_QB + w * 32;
    const bool on = q0 < p.S;  // wave-uniform: the wave has at least one query
    const int SP = p.SP;
    const int nt = min(p.ntile, 4 * qb + 4);                      // one past the last key tile this block stages
    const int kt0 = 4 * (max(0, A_QB * qb - p.W + 1) / A_QB);     // the first one: 4 js(qb)
    const int dk = 4 * qb + w;                                    // this wave's diagonal tile (< ntile whenever `on`)
    // this wave's first tile (lo_w), its last tile with a key left of some row's edge (hi_w; rows end at S - 1: a padded query is a copy
    // of that row), and the same for the block's last wave - the largest of the four (hi_3)
    int lo_w, hi_w, hi_3;
    const int* lo_s = nullptr;
    if constexpr (SEG) {
        // from the array: a handful of scalar loads (q0, qb and S are wave-uniform).  lo_eff never decreases, so the last row has the largest
        lo_s = p.lo + samp;   // this sample's edges
        const int last_w = min(q0 + 31, p.S - 1), last_3 = min(A_QB * qb + 127, p.S - 1);
        const int lo_first = __builtin_amdgcn_readfirstlane(as_lo_eff(lo_s, on ? q0 : 0, p.W));
        const int lo_last = __builtin_amdgcn_readfirstlane(as_lo_eff(lo_s, last_w, p.W));
        const int lo_blk = __builtin_amdgcn_readfirstlane(as_lo_eff(lo_s, last_3, p.W));
        lo_w = lo_first / 32;
        hi_w = lo_last > 0 ? (lo_last - 1) / 32 : -1;
        hi_3 = lo_blk > 0 ? (lo_blk - 1) / 32 : -1;
    } else {
        lo_w = max(0, q0 - p.W + 1) / 32;
        hi_w = min(q0 + 31, p.S - 1) - p.W >= 0 ? (min(q0 + 31, p.S - 1) - p.W) / 32 : -1;
        hi_3 = min(A_QB * qb + 127, p.S - 1) - p.W >= 0 ? (min(A_QB * qb + 127, p.S - 1) - p.W) / 32 : -1;
    }
    const int left_end = max(kt0, min(hi_3 + 1, 4 * qb));         // [kt0, left_end): edge; [left_end, 4 qb): whole; [4 qb, nt): edge
    const float* x1 = p.x1 + flat0;
    const float* x2 = p.x2 + flat0;

    // ---- cooperative staging of one key tile (32 keys x DH of each operand): NR + NR float4 per thread ------------------
    unsigned goff[NR], goff_last[NR], s1[NR], s2[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int idx = tid + A_NT * r, key = idx / C4, c4 = idx % C4;
        goff[r] = (unsigned)(key * p.ldx + 4 * c4);
        goff_last[r] = RAGGED ? (unsigned)(min(key, p.S - 1 - 32 * (p.ntile - 1)) * p.ldx + 4 * c4) : goff[r];  // last key tile: rows clamped to S - 1
        s1[r] = (unsigned)((8 * ((key >> 2) & 3) + 4 * (key >> 4) + (key & 3)) * X1_LD + 4 * c4);
        s2[r] = (unsigned)(key * X2_LD + ((4 * c4 + 32 * (key >> 4)) & (DH - 1)));
    }
    float4 sa0, sa1, sa2, sa3, sb0, sb1, sb2, sb3;   // the staged tile on its way to LDS (A_STAGE_LOAD / A_STAGE_STORE)

    // ---- per-query state ----------------------------------------------------------------------------------------
    const int qrow = on ? q0 + q : 0;                        // row of the scratch tensors (padded rows exist there)
    const int row = RAGGED ? min(qrow, p.S - 1) : qrow;      // row of the projection layout
    float4 bq[DH / 8];  // B operand of pass 1: element (query, dh = 8j + 4h + c)
    {
        const float* b = p.bq + samp * p.ldq + hoff + (long long)row * p.ldq + 4 * h;
#pragma unroll
        for (int j = 0; j < DH / 8; ++j) bq[j] = *reinterpret_cast<const float4*>(b + 8 * j);
    }
    int lo_row;   // this row's first key (row < S always)
    if constexpr (SEG) lo_row = as_lo_eff(lo_s, row, p.W);
    else lo_row = row - p.W + 1;
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

    // element index of (row q0, key 0) in the banded tensors: keys left of 128 js(qb) are never addressed from this row
    const long long rowbase = (long long)bh * p.ext + (long long)(on ? q0 : 0) * p.ld;
    const uint2 key = make_uint2((unsigned)p.seed, (unsigned)(p.seed >> 32));
    // the draws stay indexed in the padded (B*H, SP, SP) tensor: 8 per Philox call
    const unsigned long long ctr0 = (unsigned long long)((((long long)bh * SP + (on ? q0 : 0)) + q) * SP) / 8 + 2 * h + p.offset;
    float* scrw = scr[w];
    float* scrb = scrw + (BWD ? 32 * SCR_LD : 0);
    float4 sn0, sn1, sn2, sn3;   // backward: the score tile of the NEXT iteration, in the coalesced load layout
    unsigned mkn = 0;            // and this row's 32 dropout bits of that tile
    // this wave's mask words: [bh][query tile][kt - kt0][q], ld / 32 key tiles per query tile
    unsigned* const mwave = MASKED ? p.maskbits + (((long long)bh * (SP / 32) + (on ? q0 / 32 : 0)) * (p.ld / 32)) * 32 + q : nullptr;
    const unsigned* mload = mwave;
    const float* sload = p.scores + rowbase + (long long)(lane >> 3) * p.ld + 4 * (lane & 7);
    const int sld = p.ld;
    // kt0 is even: the first staged tile goes to image 0, as `kt & 1` says.  The wave's first score tile is lo_w's: it waits in the
    // wave's own scratch while the block stages the tiles in front of it
    A_STAGE_LOAD(kt0);
    if (BWD && on) A_SCORES_LOAD(lo_w);
    A_STAGE_STORE(0);
    if (BWD && on) A_SCORES_TO_LDS();
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): every prologue load has landed (attention_kernel says why)
    __syncthreads();

    // two rounds of (edge tiles, whole tiles): the left edge and the tiles behind it, then the diagonal square and nothing - ONE copy of
    // each body (a third copy cost the masked forward and the backward registers they do not have)
#pragma clang loop unroll(disable)
    for (int part = 0; part < 2; ++part) {
        const int e0 = part == 0 ? kt0 : 4 * qb, e1 = part == 0 ? left_end : nt;
        for (int kt = e0; kt < e1; ++kt) {
#define NK_ATT_TAIL true
#include "nk_attention_tile.h"
#undef NK_ATT_TAIL
        }
        if (part == 0) {
            for (int kt = left_end; kt < 4 * qb; ++kt) {
#define NK_ATT_TAIL false
#include "nk_attention_tile.h"
#undef NK_ATT_TAIL
            }
        }
    }
#undef NK_ATT_LEFT
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

// algorithmic flops of one direction's two products: sum over r of min(r + 1, W) (query, key) pairs
double ab_flops(int B, int S, int H, int dh, int W) {
    const double w = W < S ? W : S;
    const double pairs = w * (w + 1) / 2 + ((double)S - w) * w;
    return 4.0 * B * H * dh * pairs;
}

// One host path for both forms.  SEG: `lo` is the (B, S) array of left edges and `window` the span; otherwise `lo` is not looked at.
// `what` names the entry point in every refusal.
template <bool BWD, int DH, bool SEG>
int ab_launch_dh(nk_device* dev, BandArgs<SEG>& a, const char* what, int B, int S, int H, double p, int train, uint64_t seed, uint64_t offset,
                 float scale, int window) {
    a.S = S; a.H = H; a.nqb = (S + A_QB - 1) / A_QB; a.SP = ab_padded(S); a.ntile = a.SP / 32;
    a.W = window < S ? window : S;   // (a window that holds every key is the window S: the same band, no overflow in r - W)
    a.ld = ab_ld(S, window); a.ext = ab_extent(S, window);
    a.scale = scale; a.c1 = scale * 1.44269504088896341f; a.keep = (float)(1.0 - p); a.dscale = 1.f / (1.f - (float)p);
    a.seed = seed; a.offset = offset;
    a.rev = 1;   // longest walk first, as the causal kernels
    a.keep_lt = nk_keep_threshold(1.0 - p);
    const bool masked = train && p != 0.0;
    if (!BWD && masked)
        if (int rc = nk_refuse_capture(dev, (std::string(what) + ": the Philox offset (every replay would draw the same mask)").c_str(),
                                       "run the training-mode dropout eagerly, or capture the evaluation graph")) return rc;
    const dim3 grid((unsigned)(B * H * a.nqb)), block(A_NT);
    const bool ragged = S % 32 != 0;
    // blocks per CU the register budget is sized for: the causal kernels' (nk_attention.hip, attention_launch_dh)
    // - except the masked DH = 64 forward: the causal one is sized for three blocks and spills 28 - 44 bytes per lane to get there; the
    // band's extra wave-uniform state (three more tile bounds next to the 32 SGPRs of lane masks) pushed that to 44 - 100 bytes, so
    // it is sized for two blocks and spills nothing.  Not measured for this kernel; the causal kernel's own measurement of the
    // trade was 1.36 ms at three blocks against 1.37 - 1.41 ms at two
    constexpr int OCC = DH == 128 ? 1 : (BWD ? 2 : 3);
    constexpr int OCC_M = (!BWD && DH == 64) ? 2 : OCC;   // the MASKED instantiations
    if (ragged) {
        if (masked) hipLaunchKernelGGL((attention_band_kernel<BWD, true, OCC_M, DH, true, SEG>), grid, block, 0, dev->compute, a);
        else hipLaunchKernelGGL((attention_band_kernel<BWD, false, OCC, DH, true, SEG>), grid, block, 0, dev->compute, a);
    } else {
        if (masked) hipLaunchKernelGGL((attention_band_kernel<BWD, true, OCC_M, DH, false, SEG>), grid, block, 0, dev->compute, a);
        else hipLaunchKernelGGL((attention_band_kernel<BWD, false, OCC, DH, false, SEG>), grid, block, 0, dev->compute, a);
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}
template <bool BWD, bool SEG>
int ab_launch(nk_device* dev, BandArgs<SEG>& a, const char* what, int B, int S, int H, int dh, double p, int train, uint64_t seed,
              uint64_t offset, float scale, int window) {
    if (dh == 32) return ab_launch_dh<BWD, 32>(dev, a, what, B, S, H, p, train, seed, offset, scale, window);
    if (dh == 128) return ab_launch_dh<BWD, 128>(dev, a, what, B, S, H, p, train, seed, offset, scale, window);
    return ab_launch_dh<BWD, 64>(dev, a, what, B, S, H, p, train, seed, offset, scale, window);
}

template <bool SEG>
int ab_fwd_impl(nk_device* dev, const char* what, const float* Q, const float* K, const float* V, const int* lo, int ld_qkv, float* scores,
                float* stats, uint32_t* mask_bits, float* O, int B, int S, int H, int dh, float scale, double p, int train, uint64_t seed,
                uint64_t offset, int window) {
    NK_CHECK(dev != nullptr, "null device handle");
    if (SEG) NK_CHECK(window > 0, "%s: span must be positive, got %d", what, window);
    if (int rc = attention_check(B, S, H, dh, p, train, scale, ab_ld(S, window), what, window)) return rc;
    NK_CHECK(Q && K && V && O, "null pointer in %s", what);
    if (SEG) NK_CHECK(lo != nullptr, "%s needs the (B, S) array of left edges", what);
    NK_CHECK(scores && stats, "%s keeps the scores and the row statistics: there is no inference form, both buffers are needed", what);
    NK_CHECK(mask_bits || !(train && p != 0.0), "%s: dropout is active, the mask_bits buffer is needed", what);
    NK_CHECK(attn_al16(Q) && attn_al16(K) && attn_al16(V) && attn_al16(scores) && attn_al16(O) && attn_al16(stats),
             "%s needs 16-byte aligned buffers", what);
    NK_CHECK((long long)B * S * ld_qkv < (1ll << 31), "attention: the packed projection layout exceeds 2^31 elements");
    NK_USE(dev);
    nk_prof_start(dev, NK_KERNEL_ATTENTION, ab_flops(B, S, H, dh, window) /* seg: the band's pairs, an upper bound - the edges stay on the device */);
    BandArgs<SEG> a{};
    a.x1 = K; a.x2 = V; a.bq = Q; a.out = O; a.scores = scores; a.stats = stats; a.maskbits = mask_bits;
    if constexpr (SEG) a.lo = lo;
    a.ldx = ld_qkv; a.ldq = ld_qkv; a.ldc = H * dh; a.ldo = H * dh;
    const int rc = ab_launch<false>(dev, a, what, B, S, H, dh, p, train, seed, offset, scale, window);
    nk_prof_stop(dev);
    return rc;
}

template <bool SEG>
int ab_bwd_impl(nk_device* dev, const char* what, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO, const float* O,
                const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q, const float* K, const float* V,
                const int* lo, int ld_qkv, int B, int S, int H, int dh, float scale, double p, int train, int assign_dq, int assign_dk,
                int assign_dv, int window) {
    NK_CHECK(dev != nullptr, "null device handle");
    if (SEG) NK_CHECK(window > 0, "%s: span must be positive, got %d", what, window);
    if (int rc = attention_check(B, S, H, dh, p, train, scale, ab_ld(S, window), what, window)) return rc;
    NK_CHECK(dQ && dK && dV && dS && dropped && dO && O && scores && stats && Q && K && V, "null pointer in %s", what);
    if (SEG) NK_CHECK(lo != nullptr, "%s needs the (B, S) array of left edges", what);
    NK_CHECK(mask_bits || !(train && p != 0.0), "%s: dropout is active, the forward's mask_bits are needed", what);
    NK_CHECK(attn_al16(dQ) && attn_al16(dK) && attn_al16(dV) && attn_al16(dS) && attn_al16(dropped) && attn_al16(dO) && attn_al16(O) &&
                 attn_al16(scores) && attn_al16(stats) && attn_al16(Q) && attn_al16(K) && attn_al16(V),
             "%s needs 16-byte aligned buffers", what);
    NK_CHECK((long long)B * S * ld_qkv < (1ll << 31), "attention: the packed projection layout exceeds 2^31 elements");
    NK_USE(dev);
    nk_prof_start(dev, NK_KERNEL_ATTENTION, ab_flops(B, S, H, dh, window) /* seg: the band's pairs, an upper bound - the edges stay on the device */);
    BandArgs<SEG> a{};
    a.x1 = V; a.x2 = K; a.bq = dO; a.ctx = O; a.out = dQ; a.scores = const_cast<float*>(scores); a.ds = dS; a.dropped = dropped;
    a.stats = const_cast<float*>(stats); a.maskbits = const_cast<uint32_t*>(mask_bits); a.assign = assign_dq ? 1 : 0;
    if constexpr (SEG) a.lo = lo;
    a.ldx = ld_qkv; a.ldq = H * dh; a.ldc = H * dh; a.ldo = ld_qkv;
    const int rc = ab_launch<true>(dev, a, what, B, S, H, dh, p, train, 0, 0, scale, window);
    nk_prof_stop(dev);
    if (rc) return rc;
    // the strips reach nb blocks down (not ld / 128 - 1: ld is clamped to SP)
    const long long nb = ((long long)a.W - 1 + A_QB - 1) / A_QB;
    return strip_products(dev, dK, dV, dS, dropped, dO, Q, ld_qkv, B, S, H, dh, assign_dk, assign_dv, a.ld, a.ext, nb);
}

}  // namespace

extern "C" {

int nk_attention_band_ld(int S, int window) { return S > 0 && window > 0 ? ab_ld(S, window) : 0; }
size_t nk_attention_band_scratch(int S, int window) { return S > 0 && window > 0 ? (size_t)ab_extent(S, window) : 0; }
size_t nk_attention_band_mask_words(int S, int window) { return S > 0 && window > 0 ? (size_t)ab_padded(S) * (size_t)(ab_ld(S, window) / 32) : 0; }

int nk_attention_band_fwd(nk_device* dev, const float* Q, const float* K, const float* V, float* scores, float* stats, uint32_t* mask_bits,
                          float* O, int B, int S, int H, int dh, float scale, double p, int train, uint64_t seed, uint64_t offset, int window) {
    return ab_fwd_impl<false>(dev, "nk_attention_band_fwd", Q, K, V, nullptr, H * dh, scores, stats, mask_bits, O, B, S, H, dh, scale, p, train,
                              seed, offset, window);
}
int nk_attention_band_bwd(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO, const float* O,
                          const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q, const float* K, const float* V,
                          int B, int S, int H, int dh, float scale, double p, int train, int assign_dq, int assign_dk, int assign_dv, int window) {
    return ab_bwd_impl<false>(dev, "nk_attention_band_bwd", dQ, dK, dV, dS, dropped, dO, O, scores, stats, mask_bits, Q, K, V, nullptr, H * dh,
                              B, S, H, dh, scale, p, train, assign_dq, assign_dk, assign_dv, window);
}
int nk_attention_qkv_band_fwd(nk_device* dev, const float* QKV, float* scores, float* stats, uint32_t* mask_bits, float* O, int B, int S, int H,
                              int dh, float scale, double p, int train, uint64_t seed, uint64_t offset, int window) {
    NK_CHECK(QKV != nullptr, "null pointer in nk_attention_qkv_band_fwd");
    const int d = H * dh;
    return ab_fwd_impl<false>(dev, "nk_attention_band_fwd", QKV, QKV + d, QKV + 2 * d, nullptr, 3 * d, scores, stats, mask_bits, O, B, S, H, dh,
                              scale, p, train, seed, offset, window);
}
int nk_attention_qkv_band_bwd(nk_device* dev, float* dQKV, float* dS, float* dropped, const float* dO, const float* O, const float* scores,
                              const float* stats, const uint32_t* mask_bits, const float* QKV, int B, int S, int H, int dh, float scale,
                              double p, int train, int assign, int window) {
    NK_CHECK(dQKV && QKV, "null pointer in nk_attention_qkv_band_bwd");
    const int d = H * dh;
    return ab_bwd_impl<false>(dev, "nk_attention_band_bwd", dQKV, dQKV + d, dQKV + 2 * d, dS, dropped, dO, O, scores, stats, mask_bits, QKV,
                              QKV + d, QKV + 2 * d, nullptr, 3 * d, B, S, H, dh, scale, p, train, assign, assign, assign, window);
}

int nk_attention_seg_fwd(nk_device* dev, const float* Q, const float* K, const float* V, const int* lo, float* scores, float* stats,
                         uint32_t* mask_bits, float* O, int B, int S, int H, int dh, int span, float scale, double p, int train, uint64_t seed,
                         uint64_t offset) {
    return ab_fwd_impl<true>(dev, "nk_attention_seg_fwd", Q, K, V, lo, H * dh, scores, stats, mask_bits, O, B, S, H, dh, scale, p, train, seed,
                             offset, span);
}
int nk_attention_seg_bwd(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO, const float* O,
                         const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q, const float* K, const float* V,
                         const int* lo, int B, int S, int H, int dh, int span, float scale, double p, int train, int assign_dq, int assign_dk,
                         int assign_dv) {
    return ab_bwd_impl<true>(dev, "nk_attention_seg_bwd", dQ, dK, dV, dS, dropped, dO, O, scores, stats, mask_bits, Q, K, V, lo, H * dh, B, S, H,
                             dh, scale, p, train, assign_dq, assign_dk, assign_dv, span);
}
int nk_attention_qkv_seg_fwd(nk_device* dev, const float* QKV, const int* lo, float* scores, float* stats, uint32_t* mask_bits, float* O,
                             int B, int S, int H, int dh, int span, float scale, double p, int train, uint64_t seed, uint64_t offset) {
    NK_CHECK(QKV != nullptr, "null pointer in nk_attention_qkv_seg_fwd");
    const int d = H * dh;
    return ab_fwd_impl<true>(dev, "nk_attention_seg_fwd", QKV, QKV + d, QKV + 2 * d, lo, 3 * d, scores, stats, mask_bits, O, B, S, H, dh, scale,
                             p, train, seed, offset, span);
}
int nk_attention_qkv_seg_bwd(nk_device* dev, float* dQKV, float* dS, float* dropped, const float* dO, const float* O, const float* scores,
                             const float* stats, const uint32_t* mask_bits, const float* QKV, const int* lo, int B, int S, int H, int dh,
                             int span, float scale, double p, int train, int assign) {
    NK_CHECK(dQKV && QKV, "null pointer in nk_attention_qkv_seg_bwd");
    const int d = H * dh;
    return ab_bwd_impl<true>(dev, "nk_attention_seg_bwd", dQKV, dQKV + d, dQKV + 2 * d, dS, dropped, dO, O, scores, stats, mask_bits, QKV,
                             QKV + d, QKV + 2 * d, lo, 3 * d, B, S, H, dh, scale, p, train, assign, assign, assign, span);
}

}  // extern "C"
