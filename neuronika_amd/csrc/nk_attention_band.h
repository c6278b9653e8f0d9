// Sliding-window attention in the fused core, forward and backward (ours; semantics in include/neuronika_hip.h): query r attends to
// the keys max(0, r - W + 1) .. r.  attention_band_kernel is the causal instantiation of nk_attention.hip's attention_kernel - 256
// threads, 128 queries per block, key tiles of 32, the transposed score tile in registers between the two mfma_f32_32x32x2f32
// products, online softmax in the exp2 domain with the lazy shift, two Philox calls per lane and tile packed to one bit per score,
// -inf stored at masked scores - with a walk that also skips the key tiles LEFT of the band: O(S W) work and O(S W) scratch.
// Included by nk_norm.hip.  nk_attention.hip is a unit whose instantiations are inventoried one by one and stays as it is, so this
// header carries its own copies of the small helpers it shares with that file (the args struct, tile_write / tile_flush, the staging
// macros): the duplication is the price of leaving the inventoried unit untouched.
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
// Specialisations carried: RAGGED (S % 32 != 0).  Not carried: FULL (S % 128 == 0 without the `on` test) and the KEEP = false
// inference forward - neither was measured to pay here, and every instantiation has to be reached by a test.
// dK / dV: one nk_sgemm_pair_batched per strip of 128 keys over the queries of blocks j .. min(nqb - 1, j + ceil((W - 1) / 128)).
#pragma once
#include <cmath>

#include "nk_mma.h"

namespace {

using nkmma::f32x16;

constexpr int AB_NT = 256;      // 4 waves, 32 queries each
constexpr int AB_QB = 128;      // queries per block
constexpr int AB_SCR_LD = 36;   // per-wave 32 x 32 transposition scratch
constexpr int ab_x1_ld(int dh) { return dh + 4; }   // pass-1 operand image [mfma row][dh], padded by 4
constexpr int ab_x2_ld(int dh) { return dh; }       // pass-2 operand image [key][dh rotated by 32 for keys >= 16]

// the geometry, on the host: the one source of the layout (exported below)
constexpr int ab_padded(int S) { return (S + 31) / 32 * 32; }
inline int ab_ld(int S, int W) {
    const long long SP = ab_padded(S), nb = ((long long)W - 1 + 127) / 128;   // blocks left of a block's own that its band reaches
    const long long ld = 128 * (nb + 1);
    return (int)(ld < SP ? ld : SP);
}
inline long long ab_extent(int S, int W) { return (long long)(ab_padded(S) - 1) * ab_ld(S, W) + ab_padded(S); }

struct BandArgs {
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
    int W;             // the window
    int ld;            // row stride of scores / dS / Pd
    long long ext;     // floats per (sample, head) of each
};

// (nk_attention.hip's helpers, see the note at the top)
__device__ __forceinline__ void wave_lds_handover() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ void tile_write(float* scrw, const float (&v)[16], int lane) {
    const int q = lane & 31, h = lane >> 5;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        *reinterpret_cast<float4*>(&scrw[q * AB_SCR_LD + 16 * h + 4 * c]) = make_float4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
}
__device__ __forceinline__ void tile_flush(const float* scrw, float* g /* &T[row0][kt*32] */, int ld, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = 8 * i + (lane >> 3), c = 4 * (lane & 7);
        const float4 t = *reinterpret_cast<const float4*>(&scrw[r * AB_SCR_LD + c]);
        nk_store_stream(reinterpret_cast<float4*>(g + (long long)r * ld + c), t);
    }
}

template <bool BWD, bool MASKED, int OCC, int DH, bool RAGGED>
__global__ __launch_bounds__(AB_NT, OCC) void attention_band_kernel(const BandArgs p) {
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
    const int lo_w = max(0, q0 - p.W + 1) / 32;                   // its first tile
    // its last tile with a key left of some row's window (rows end at S - 1: a padded query is a copy of that row), and the same for
    // the block's last wave - the largest of the four
    const int hi_w = min(q0 + 31, p.S - 1) - p.W >= 0 ? (min(q0 + 31, p.S - 1) - p.W) / 32 : -1;
    const int hi_3 = min(AB_QB * qb + 127, p.S - 1) - p.W >= 0 ? (min(AB_QB * qb + 127, p.S - 1) - p.W) / 32 : -1;
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
#define AB_STAGE_LOAD(KT)                                                                                        \
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
#define AB_STAGE_STORE(BUF)                                                                                      \
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
    float* scrb = scrw + (BWD ? 32 * AB_SCR_LD : 0);
    float4 sn0, sn1, sn2, sn3;   // backward: the score tile of the NEXT iteration, in the coalesced load layout
    unsigned mkn = 0;            // and this row's 32 dropout bits of that tile
    // this wave's mask words: [bh][query tile][kt - kt0][q], ld / 32 key tiles per query tile
    unsigned* const mwave = MASKED ? p.maskbits + (((long long)bh * (SP / 32) + (on ? q0 / 32 : 0)) * (p.ld / 32)) * 32 + q : nullptr;
    const unsigned* mload = mwave;
    const float* sload = p.scores + rowbase + (long long)(lane >> 3) * p.ld + 4 * (lane & 7);
#define AB_SCORES_LOAD(KT)                                                                       \
    do {                                                                                         \
        sn0 = *reinterpret_cast<const float4*>(sload + (KT) * 32);                               \
        sn1 = *reinterpret_cast<const float4*>(sload + (long long)8 * p.ld + (KT) * 32);         \
        sn2 = *reinterpret_cast<const float4*>(sload + (long long)16 * p.ld + (KT) * 32);        \
        sn3 = *reinterpret_cast<const float4*>(sload + (long long)24 * p.ld + (KT) * 32);        \
        if (MASKED) mkn = mload[((KT) - kt0) * 32];                                              \
    } while (0)
#define AB_SCORES_TO_LDS()                                                                       \
    do {                                                                                         \
        float* sw_ = &scrw[(lane >> 3) * AB_SCR_LD + 4 * (lane & 7)];                            \
        *reinterpret_cast<float4*>(sw_) = sn0;                                                   \
        *reinterpret_cast<float4*>(sw_ + 8 * AB_SCR_LD) = sn1;                                   \
        *reinterpret_cast<float4*>(sw_ + 16 * AB_SCR_LD) = sn2;                                  \
        *reinterpret_cast<float4*>(sw_ + 24 * AB_SCR_LD) = sn3;                                  \
    } while (0)
    // kt0 is even: the first staged tile goes to image 0, as `kt & 1` says.  The wave's first score tile is lo_w's: it waits in the
    // wave's own scratch while the block stages the tiles in front of it
    AB_STAGE_LOAD(kt0);
    if (BWD && on) AB_SCORES_LOAD(lo_w);
    AB_STAGE_STORE(0);
    if (BWD && on) AB_SCORES_TO_LDS();
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): every prologue load has landed (nk_attention.hip)
    __syncthreads();

    // two rounds of (edge tiles, whole tiles): the left edge and the tiles behind it, then the diagonal square and nothing - ONE copy of
    // each body (a third copy cost the masked forward and the backward registers they do not have)
#pragma clang loop unroll(disable)
    for (int part = 0; part < 2; ++part) {
        const int e0 = part == 0 ? kt0 : 4 * qb, e1 = part == 0 ? left_end : nt;
        for (int kt = e0; kt < e1; ++kt) {
#define NK_BAND_EDGE true
#include "nk_attention_band_tile.h"
#undef NK_BAND_EDGE
        }
        if (part == 0) {
            for (int kt = left_end; kt < 4 * qb; ++kt) {
#define NK_BAND_EDGE false
#include "nk_attention_band_tile.h"
#undef NK_BAND_EDGE
            }
        }
    }
#undef AB_STAGE_LOAD
#undef AB_STAGE_STORE
#undef AB_SCORES_LOAD
#undef AB_SCORES_TO_LDS
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

bool ab_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// attention_check of nk_attention.hip with the banded extents
int ab_check(int B, int S, int H, int dh, double p, int train, float scale, int window, const char* what) {
    NK_CHECK(p >= 0.0 && p <= 1.0, "Wrong probability received: %g.", p);
    NK_CHECK(scale > 0.f && scale < 1e30f, "fused attention needs a positive finite scale (the row max is taken before scaling), got %g", (double)scale);
    NK_CHECK(B > 0 && S > 0 && H > 0, "attention: non-positive geometry");
    NK_CHECK(window > 0, "%s: window must be positive, got %d", what, window);
    NK_CHECK(nk_attention_supported(S, dh, p, train), "fused attention needs dh in {32, 64, 128} and p < 1 in training (S=%d dh=%d p=%g)", S, dh, p);
    NK_CHECK((long long)B * H * (ab_padded(S) / 32) * (ab_ld(S, window) / 32) < (1ll << 31) / 32, "attention: the mask words exceed 2^31");
    NK_CHECK((long long)B * S * H * dh < (1ll << 31), "attention: the projection layout exceeds 2^31 elements");
    return NK_OK;
}

// algorithmic flops of one direction's two products: sum over r of min(r + 1, W) (query, key) pairs
double ab_flops(int B, int S, int H, int dh, int W) {
    const double w = W < S ? W : S;
    const double pairs = w * (w + 1) / 2 + ((double)S - w) * w;
    return 4.0 * B * H * dh * pairs;
}

template <bool BWD, int DH>
int ab_launch_dh(nk_device* dev, BandArgs& a, int B, int S, int H, double p, int train, uint64_t seed, uint64_t offset, float scale, int window) {
    a.S = S; a.H = H; a.nqb = (S + AB_QB - 1) / AB_QB; a.SP = ab_padded(S); a.ntile = a.SP / 32;
    a.W = window < S ? window : S;   // (a window that holds every key is the window S: the same band, no overflow in r - W)
    a.ld = ab_ld(S, window); a.ext = ab_extent(S, window);
    a.scale = scale; a.c1 = scale * 1.44269504088896341f; a.keep = (float)(1.0 - p); a.dscale = 1.f / (1.f - (float)p);
    a.seed = seed; a.offset = offset;
    a.rev = 1;   // longest walk first, as the causal kernels
    a.keep_lt = nk_keep_threshold(1.0 - p);
    const bool masked = train && p != 0.0;
    if (!BWD && masked)
        if (int rc = nk_refuse_capture(dev, "nk_attention_band_fwd: the Philox offset (every replay would draw the same mask)",
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
        if (masked) hipLaunchKernelGGL((attention_band_kernel<BWD, true, OCC_M, DH, true>), grid, block, 0, dev->compute, a);
        else hipLaunchKernelGGL((attention_band_kernel<BWD, false, OCC, DH, true>), grid, block, 0, dev->compute, a);
    } else {
        if (masked) hipLaunchKernelGGL((attention_band_kernel<BWD, true, OCC_M, DH, false>), grid, block, 0, dev->compute, a);
        else hipLaunchKernelGGL((attention_band_kernel<BWD, false, OCC, DH, false>), grid, block, 0, dev->compute, a);
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}
template <bool BWD>
int ab_launch(nk_device* dev, BandArgs& a, int B, int S, int H, int dh, double p, int train, uint64_t seed, uint64_t offset, float scale,
              int window) {
    if (dh == 32) return ab_launch_dh<BWD, 32>(dev, a, B, S, H, p, train, seed, offset, scale, window);
    if (dh == 128) return ab_launch_dh<BWD, 128>(dev, a, B, S, H, p, train, seed, offset, scale, window);
    return ab_launch_dh<BWD, 64>(dev, a, B, S, H, p, train, seed, offset, scale, window);
}

int ab_fwd_impl(nk_device* dev, const float* Q, const float* K, const float* V, int ld_qkv, float* scores, float* stats, uint32_t* mask_bits,
                float* O, int B, int S, int H, int dh, float scale, double p, int train, uint64_t seed, uint64_t offset, int window) {
    const char* what = "nk_attention_band_fwd";
    NK_CHECK(dev != nullptr, "null device handle");
    if (int rc = ab_check(B, S, H, dh, p, train, scale, window, what)) return rc;
    NK_CHECK(Q && K && V && O, "null pointer in %s", what);
    NK_CHECK(scores && stats, "%s keeps the scores and the row statistics: there is no inference form, both buffers are needed", what);
    NK_CHECK(mask_bits || !(train && p != 0.0), "%s: dropout is active, the mask_bits buffer is needed", what);
    NK_CHECK(ab_al16(Q) && ab_al16(K) && ab_al16(V) && ab_al16(scores) && ab_al16(O) && ab_al16(stats), "%s needs 16-byte aligned buffers", what);
    NK_CHECK((long long)B * S * ld_qkv < (1ll << 31), "attention: the packed projection layout exceeds 2^31 elements");
    NK_USE(dev);
    nk_prof_start(dev, NK_KERNEL_ATTENTION, ab_flops(B, S, H, dh, window));
    BandArgs a{};
    a.x1 = K; a.x2 = V; a.bq = Q; a.out = O; a.scores = scores; a.stats = stats; a.maskbits = mask_bits;
    a.ldx = ld_qkv; a.ldq = ld_qkv; a.ldc = H * dh; a.ldo = H * dh;
    const int rc = ab_launch<false>(dev, a, B, S, H, dh, p, train, seed, offset, scale, window);
    nk_prof_stop(dev);
    return rc;
}

int ab_bwd_impl(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO, const float* O, const float* scores,
                const float* stats, const uint32_t* mask_bits, const float* Q, const float* K, const float* V, int ld_qkv, int B, int S, int H,
                int dh, float scale, double p, int train, int assign_dq, int assign_dk, int assign_dv, int window) {
    const char* what = "nk_attention_band_bwd";
    NK_CHECK(dev != nullptr, "null device handle");
    if (int rc = ab_check(B, S, H, dh, p, train, scale, window, what)) return rc;
    NK_CHECK(dQ && dK && dV && dS && dropped && dO && O && scores && stats && Q && K && V, "null pointer in %s", what);
    NK_CHECK(mask_bits || !(train && p != 0.0), "%s: dropout is active, the forward's mask_bits are needed", what);
    NK_CHECK(ab_al16(dQ) && ab_al16(dK) && ab_al16(dV) && ab_al16(dS) && ab_al16(dropped) && ab_al16(dO) && ab_al16(O) && ab_al16(scores) &&
                 ab_al16(stats) && ab_al16(Q) && ab_al16(K) && ab_al16(V),
             "%s needs 16-byte aligned buffers", what);
    NK_CHECK((long long)B * S * ld_qkv < (1ll << 31), "attention: the packed projection layout exceeds 2^31 elements");
    NK_USE(dev);
    nk_prof_start(dev, NK_KERNEL_ATTENTION, ab_flops(B, S, H, dh, window));
    BandArgs a{};
    a.x1 = V; a.x2 = K; a.bq = dO; a.ctx = O; a.out = dQ; a.scores = const_cast<float*>(scores); a.ds = dS; a.dropped = dropped;
    a.stats = const_cast<float*>(stats); a.maskbits = const_cast<uint32_t*>(mask_bits); a.assign = assign_dq ? 1 : 0;
    a.ldx = ld_qkv; a.ldq = H * dh; a.ldc = H * dh; a.ldo = ld_qkv;
    int rc = ab_launch<true>(dev, a, B, S, H, dh, p, train, 0, 0, scale, window);
    nk_prof_stop(dev);
    if (rc) return rc;
    // dK_bh (+)= dS_bh^T . Q_bh and dV_bh (+)= Pd_bh^T . dO_bh per strip of 128 keys, over the queries of the blocks that staged the
    // strip: j .. min(nqb - 1, j + nb).  A, B and C advanced to (128 j, 128 j); the A operand's row stride is ld - shorter than the
    // logical width SP, which the product never sees: it reads m <= 128 columns of K <= ld rows, and its tile window K ld + 128 is the
    // causal strip's with SP for ld.
    const int d = H * dh, ld = ab_ld(S, window);
    const long long ext = ab_extent(S, window), nb = ((long long)(window < S ? window : S) - 1 + AB_QB - 1) / AB_QB;   // (not ld / 128 - 1: ld is clamped to SP)
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

int nk_attention_band_ld(int S, int window) { return S > 0 && window > 0 ? ab_ld(S, window) : 0; }
size_t nk_attention_band_scratch(int S, int window) { return S > 0 && window > 0 ? (size_t)ab_extent(S, window) : 0; }
size_t nk_attention_band_mask_words(int S, int window) { return S > 0 && window > 0 ? (size_t)ab_padded(S) * (size_t)(ab_ld(S, window) / 32) : 0; }

int nk_attention_band_fwd(nk_device* dev, const float* Q, const float* K, const float* V, float* scores, float* stats, uint32_t* mask_bits,
                          float* O, int B, int S, int H, int dh, float scale, double p, int train, uint64_t seed, uint64_t offset, int window) {
    return ab_fwd_impl(dev, Q, K, V, H * dh, scores, stats, mask_bits, O, B, S, H, dh, scale, p, train, seed, offset, window);
}
int nk_attention_band_bwd(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO, const float* O,
                          const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q, const float* K, const float* V,
                          int B, int S, int H, int dh, float scale, double p, int train, int assign_dq, int assign_dk, int assign_dv, int window) {
    return ab_bwd_impl(dev, dQ, dK, dV, dS, dropped, dO, O, scores, stats, mask_bits, Q, K, V, H * dh, B, S, H, dh, scale, p, train, assign_dq,
                       assign_dk, assign_dv, window);
}
int nk_attention_qkv_band_fwd(nk_device* dev, const float* QKV, float* scores, float* stats, uint32_t* mask_bits, float* O, int B, int S, int H,
                              int dh, float scale, double p, int train, uint64_t seed, uint64_t offset, int window) {
    NK_CHECK(QKV != nullptr, "null pointer in nk_attention_qkv_band_fwd");
    const int d = H * dh;
    return ab_fwd_impl(dev, QKV, QKV + d, QKV + 2 * d, 3 * d, scores, stats, mask_bits, O, B, S, H, dh, scale, p, train, seed, offset, window);
}
int nk_attention_qkv_band_bwd(nk_device* dev, float* dQKV, float* dS, float* dropped, const float* dO, const float* O, const float* scores,
                              const float* stats, const uint32_t* mask_bits, const float* QKV, int B, int S, int H, int dh, float scale,
                              double p, int train, int assign, int window) {
    NK_CHECK(dQKV && QKV, "null pointer in nk_attention_qkv_band_bwd");
    const int d = H * dh;
    return ab_bwd_impl(dev, dQKV, dQKV + d, dQKV + 2 * d, dS, dropped, dO, O, scores, stats, mask_bits, QKV, QKV + d, QKV + 2 * d, 3 * d, B, S, H,
                       dh, scale, p, train, assign, assign, assign, window);
}

}  // extern "C"
