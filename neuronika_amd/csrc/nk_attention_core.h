// What the fused attention kernels share: attention_kernel (nk_attention.hip: every key, or the causal triangle) and
// attention_band_kernel (nk_attention_band.h: a left edge per row, from a window or from an array).  Constants, the argument struct,
// the tile helpers, the staging macros, the argument check and the dK / dV strip products - each once.  No kernel lives here; the
// body of one key tile, which both kernels include inside their loops, is nk_attention_tile.h.
#pragma once
#include <cmath>
#include <cstdlib>

#include "nk_mma.h"

namespace {

using nkmma::f32x16;

// Head dimension DH in {32, 64, 128} (template parameter): DH / 32 MFMA column tiles of the output, DH / 8 b128 k-groups of the
// score product.  64 is the C5 geometry the register / LDS budgets were tuned for (three forward blocks per CU); 128 holds 64 + 64
// VGPRs of per-query operand and output accumulators and 66 KB of staged K / V per block - one block per CU, still one kernel per
// direction instead of the node-by-node path; 32 halves everything.
constexpr int A_NT = 256;   // 4 waves, 32 queries each
constexpr int A_QB = 128;   // queries per block
constexpr int SCR_LD = 36;  // per-wave 32 x 32 transposition scratch
// pass-1 operand image [mfma row][dh], padded by 4: b128 fragment reads of 16 rows hit 16 distinct slots
constexpr int x1_ld(int dh) { return dh + 4; }
// pass-2 operand image [key][dh rotated by 32 for keys >= 16]: the two lane halves read disjoint banks (DH = 32: no rotation
// possible, the halves share banks - a two-way conflict on 16 of the tile's LDS reads)
constexpr int x2_ld(int dh) { return dh; }

// The arguments of attention_kernel, and the common prefix of attention_band_kernel's (BandArgs, nk_attention_band.h)
struct AttnArgs {
    const float* x1;   // pass-1 operand, flat (B*S) x (H*dh) layout: forward K, backward V
    const float* x2;   // pass-2 operand:                               forward V, backward K
    const float* bq;   // per-query operand:                            forward Q, backward dO
    const float* ctx;  // backward only: the forward output O (for sum_k dP * P = keep * dO . O)
    float* out;        // forward O, backward dQ
    float* scores;     // (B*H, S, S) raw scores: written forward, read backward
    float* ds;         // backward: dS
    float* dropped;    // backward: Pd
    unsigned* maskbits;  // (B*H, S/32 query tiles, S/32 key tiles, 32 queries) words: the dropout draws, 1 bit per score (bit 16h + e of
                         // word [bh][qt][kt][q] = key 32 kt + 16 h + e of query 32 qt + q kept): written forward, read backward.  A wave's
                         // 32 words of one tile are ONE 128-byte line (row-major (B*H, S, S/32) made every tile 32 scattered 4-byte stores:
                         // 16.8 M partial-line write requests per C5 forward next to the 33.5 M of the scores)
    float* stats;      // (B*H, S, 2): the shift m2 (log2 units; row max of s*c1 minus at most 6) and 1 / sum_k exp2(s*c1 - m2)
    int S, H, nqb, ntile;
    // row strides (floats) of the projection-layout operands: a (B*S, H*dh) matrix of its own has ld = H*dh; Q, K, V (and dQ,
    // dK, dV) that are column blocks of ONE packed (B*S, 3*H*dh) projection output have ld = 3*H*dh
    int ldx;           // x1, x2
    int ldq;           // bq
    int ldc;           // ctx
    int ldo;           // out
    float scale, keep, dscale;
    float c1;          // scale * log2(e): exponents are taken in base 2
    unsigned keep_lt;  // a draw v is kept iff v < keep_lt = floor((1 - p) * 2^32)  (nk_common.h: the Bernoulli construction)
    int rev;           // causal: a head's query blocks in descending order (longest walk first); sits in the 4 bytes of padding in front of `seed`
    unsigned long long seed, offset;
    int assign;        // backward: dQ = (1) or += (0)
    int SP;            // S rounded up to a multiple of 32: row count and row stride of the (B*H, SP, SP) scratch tensors (scores, dS, Pd,
                       // statistics, mask words).  SP == S except for ragged sequence lengths (read by the RAGGED instantiations only)
};

// Wave-private LDS round trip: every lane's ds_write is issued before any lane's ds_read (LDS is in-order per wave); the
// fences keep the compiler from reordering across the hand-over.
__device__ __forceinline__ void wave_lds_handover() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// registers (lane = query q, half h, 16 consecutive keys 16h..16h+15) -> 32 x 32 tile of a row-major tensor of row stride ld, as
// 128-byte row segments (8 lanes x 16 B) instead of 64 scattered 16-byte pieces per store instruction.  Two halves, issued
// far apart: the tile goes to the wave's LDS scratch as soon as it is computed, and is read back and stored to HBM after
// the second MFMA product of the iteration - the ds_write -> ds_read round trip (a few hundred cycles, and there are only
// two or three waves per SIMD to hide it) then runs under 32 MFMAs instead of stalling the wave.
__device__ __forceinline__ void tile_write(float* scrw, const float (&v)[16], int lane) {
    const int q = lane & 31, h = lane >> 5;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        *reinterpret_cast<float4*>(&scrw[q * SCR_LD + 16 * h + 4 * c]) = make_float4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
}
__device__ __forceinline__ void tile_flush(const float* scrw, float* g /* &T[row0][kt*32] */, int ld, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = 8 * i + (lane >> 3), c = 4 * (lane & 7);
        const float4 t = *reinterpret_cast<const float4*>(&scrw[r * SCR_LD + c]);
        nk_store_stream(reinterpret_cast<float4*>(g + (long long)r * ld + c), t);
    }
}

// ---- staging and score loads of both kernels.  Macros over the names the kernels declare (tid-derived offsets goff / goff_last / s1 /
// s2, the LDS images x1s / x2s, the wave's scratch scrw, and the walk's `kt0` and `sld`: the first key tile the block stages and the row
// stride of the scores) because the staged values live in NAMED registers (up to four float4 per operand), not arrays: `float4 st[NR]`
// written under `if (more)` and read a loop body later is kept in scratch memory by the compiler (measured: 64 bytes of private
// segment, four scratch stores and loads per tile), and so is a small array of LDS pointers.
//   float4 sa0, sa1, sa2, sa3, sb0, sb1, sb2, sb3;   cooperative staging of one key tile (32 keys x DH of each operand)
//   float4 sn0, sn1, sn2, sn3; unsigned mkn;         backward: the score tile of the NEXT iteration and the row's 32 dropout bits
#define A_STAGE_LOAD(KT)                                                                                         \
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
#define A_STAGE_STORE(BUF)                                                                                       \
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
// the coalesced load layout: lane -> rows 8i + lane / 8, 16 B each; the mask words are counted from the block's first staged tile
#define A_SCORES_LOAD(KT)                                                                        \
    do {                                                                                         \
        sn0 = *reinterpret_cast<const float4*>(sload + (KT) * 32);                               \
        sn1 = *reinterpret_cast<const float4*>(sload + (long long)8 * sld + (KT) * 32);          \
        sn2 = *reinterpret_cast<const float4*>(sload + (long long)16 * sld + (KT) * 32);         \
        sn3 = *reinterpret_cast<const float4*>(sload + (long long)24 * sld + (KT) * 32);         \
        if (MASKED) mkn = mload[((KT) - kt0) * 32];                                              \
    } while (0)
#define A_SCORES_TO_LDS()                                                                        \
    do {                                                                                         \
        float* sw_ = &scrw[(lane >> 3) * SCR_LD + 4 * (lane & 7)];                               \
        *reinterpret_cast<float4*>(sw_) = sn0;                                                   \
        *reinterpret_cast<float4*>(sw_ + 8 * SCR_LD) = sn1;                                      \
        *reinterpret_cast<float4*>(sw_ + 16 * SCR_LD) = sn2;                                     \
        *reinterpret_cast<float4*>(sw_ + 24 * SCR_LD) = sn3;                                     \
    } while (0)

bool attn_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The argument check of every entry point of both kernels.  ld: row stride of the scratch tensors, SP or the band's.  what / window: the
// band forms name themselves and pass their window (or span), refused when not positive - before anything derived from it is looked at.
int attention_check(int B, int S, int H, int dh, double p, int train, float scale, int ld, const char* what = nullptr, int window = 1) {
    NK_CHECK(p >= 0.0 && p <= 1.0, "Wrong probability received: %g.", p);
    NK_CHECK(scale > 0.f && scale < 1e30f, "fused attention needs a positive finite scale (the row max is taken before scaling), got %g", (double)scale);
    NK_CHECK(B > 0 && S > 0 && H > 0, "attention: non-positive geometry");
    NK_CHECK(window > 0, "%s: window must be positive, got %d", what, window);
    NK_CHECK(nk_attention_supported(S, dh, p, train), "fused attention needs dh in {32, 64, 128} and p < 1 in training (S=%d dh=%d p=%g)", S, dh, p);
    NK_CHECK((long long)B * H * ((S + 31) / 32) * (ld / 32) < (1ll << 31) / 32, "attention: the mask words exceed 2^31");
    NK_CHECK((long long)B * S * H * dh < (1ll << 31), "attention: the projection layout exceeds 2^31 elements");
    return NK_OK;
}

// dK_bh (+)= dS_bh^T . Q_bh and dV_bh (+)= Pd_bh^T . dO_bh where dS and Pd are defined on some 128 x 128 blocks only (the kernels never
// visit the others; garbage times zero is NaN): one pair of products per strip of 128 keys, over the queries of the blocks that staged
// the strip - j .. min(nqb - 1, j + nb) - with A, B and C advanced to (128 j, 128 j).  ld / ext: row stride and floats per (sample, head)
// of dS and Pd.  Causal: ld = SP, ext = SP * SP and nb = nqb, every strip reduces down to row S.  Band: ld may be shorter than the
// logical width SP, which the product never sees: it reads m <= 128 columns of K <= ld rows, and its tile window K ld + 128 is the
// causal strip's with SP for ld.  S / 128 launches of B*H (pairs of) blocks; the chained-launch rule for reductions longer than 2048
// products is nk_sgemm's own and applies per strip.
int strip_products(nk_device* dev, float* dK, float* dV, const float* dS, const float* dropped, const float* dO, const float* Q, int ld_qkv,
                   int B, int S, int H, int dh, int assign_dk, int assign_dv, int ld, long long ext, long long nb) {
    const int d = H * dh;
    const long long so = (long long)S * d, sq = (long long)S * ld_qkv, po = (long long)H * ext, pi = ext;
    for (int j0 = 0; j0 < S; j0 += A_QB) {
        const long long last = (long long)j0 + (nb + 1) * A_QB;   // one past the last query row whose block staged the strip
        const int m = S - j0 < A_QB ? S - j0 : A_QB, k = (int)((last < S ? last : S) - j0);
        const long long da = (long long)j0 * ld + j0, dq = (long long)j0 * ld_qkv, dd = (long long)j0 * d;
        if (int rc = nk_sgemm_pair_batched(dev, B, H, 1, 0, m, dh, k, dS + da, ld, po, pi, Q + dq, ld_qkv, sq, dh, assign_dk ? 0.f : 1.f,
                                           dK + dq, ld_qkv, sq, dh, 1, 0, m, dh, k, dropped + da, ld, po, pi, dO + dd, d, so, dh,
                                           assign_dv ? 0.f : 1.f, dV + dq, ld_qkv, sq, dh)) return rc;
    }
    return NK_OK;
}

}  // namespace
