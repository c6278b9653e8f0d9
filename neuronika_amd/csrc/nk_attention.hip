// Fused attention core of the composed multi-head attention (note below the table: the module is a
// composition of MatrixMatrixMulT a-2, Multiplication a-4, Softmax a-7, Dropout a-8, MatrixMatrixMul a-1 per (sample, head)):
//
//   forward   S = Q_bh . K_bh^T ;  P = softmax(S * scale, axis 1) ;  Pd = dropout(P) ;  O_bh = Pd . V_bh
//   backward  dPd = dO_bh . V_bh^T ;  dP = dPd * noise            (DropoutBackward, node/dropout/mod.rs:113-128: mask only)
//             dS  = P * (dP - sum_k dP * P) * scale               (SoftmaxBackward :84-104, MultiplicationBackwardLeft)
//             dQ_bh += dS . K_bh          [dK_bh += dS^T . Q_bh and dV_bh += Pd^T . dO_bh stay batched GEMMs on dS / Pd]
//
// Why one kernel per direction: composed from GEMMs and row kernels the (B*H, S, S) tensors cross HBM 11 times per step
// (2.1 GB each at C5) and the K = 64 GEMMs that write them run at half the MFMA rate because 2.1 GB of C stores queue
// behind 64-deep reductions.  Here a block owns 128 queries of one (sample, head), walks the keys in tiles of 32 and keeps
// the 32 x 32 score tile ON CHIP between the two MFMA products; the big tensors cross HBM 6 times (forward writes S;
// backward reads S, writes dS and Pd; the two remaining GEMMs read dS and Pd).
//
// Layout trick (what keeps the score tile in registers): the tile is computed TRANSPOSED, C[key][query] = X1 . Bq^T, so a
// lane owns one query (column = lane & 31) and 16 keys of it.  Row statistics (max, sum, the backward dot) are then
// per-lane scalars plus one cross-half shuffle, and the C registers are directly the B operand of the second product
// out^T[dh][query] = X2^T . C (the MFMA wants B[k][n] with n = lane & 31, k chosen by the lane half: exactly what C holds
// when MFMA step e pairs key 16*0 + e with key 16*1 + e).  Rows of the MFMA tile are permuted so that a lane's 16
// registers are 16 CONSECUTIVE keys: two Philox calls of the shared draw layout (8 consecutive elements per call)
// and 64-byte runs towards HBM fall out of that.
//
// The forward uses the online softmax in the base-2 exponent domain (running shift m2 and sum of exp2(s*c1 - m2), c1 =
// scale * log2(e); the shift follows the running maximum lazily - it only has to keep the exponents <= 6 - and the out
// accumulator is rescaled when it moves) and stores (m2, 1 / sum) per row; the backward recomputes
// P = exp2(S * c1 - m2) / sum from the stored scores with those.  Against the node-by-node composition this changes the order
// of the row sum and replaces two divisions by a reciprocal and a product - inside the f32 tolerance of SURVEY.md 8c (ii),
// checked against the oracle, not bit-equal to the three-node path.
#include "nk_attention_core.h"

namespace {

// FULL: S is a multiple of 128, every wave of every block has queries.  Not a micro-optimisation: with a run-time `on`
// the loop body sits under a branch, the compiler's wait-count bookkeeping merges the two paths at the join and waits for
// ALL outstanding vector memory operations (the tile stores just issued included) before the staged tile may go to LDS;
// with the branch gone it waits for exactly the staging loads and the stores drain under the next tile's MFMAs.
// KEEP (forward only): write what the backward pass needs (scores, row statistics, dropout bits).  false = inference: O only,
// 2.1 GB of stores and the buffers themselves disappear.
// RAGGED: S is not a multiple of 32.  The scratch tensors are padded to SP = ceil32(S) rows and columns, so every tile access to
// them stays whole; what is left to guard is the caller's projection layout: key rows and query rows beyond S are CLAMPED to row
// S - 1 when loaded (a sample's rows are followed by the next sample's, or by the end of the buffer), padded keys get a score of
// -inf in the forward (probability exactly 0; the stored -inf makes the backward's recomputed probability, dS and Pd exactly 0 too),
// padded queries compute a copy of row S - 1 that is never stored outside the scratch.  The dropout draws of score (bh, r, k) are
// indexed in the PADDED tensor ((bh * SP + r) * SP + k), which keeps a lane's 16 keys on two whole Philox calls.
// CAUSAL: query r attends to keys k <= r (the composition with one Addition node in front of the Softmax: scores + M, M[r][k] = 0 for
// k <= r and -inf above; Softmax gives exactly 0 there).  Query block qb (rows 128 qb ..) stages key tiles 0 .. min(ntile, 4 qb + 4) - 1
// and nothing beyond; its wave w (rows 32 (4 qb + w) ..) computes tiles kt <= dk = 4 qb + w.  Tiles kt < 4 qb are whole for all four
// waves and run the loop body as it is (the MAIN part: no predicate, see FULL); the last (at most) four tiles are the TAIL part, the
// same body under a per-wave predicate: tile dk is the wave's diagonal tile, where key 32 dk + 16 h + e is masked for query
// 32 dk + q when 16 h + e > q - the forward stores -inf as its score, exactly as RAGGED does for padded keys, so the backward's
// recomputed probability, dS and Pd are exactly 0 there without a second test; for kt > dk the wave takes part in the staging and
// the barrier, draws nothing, and (backward) writes ZERO tiles of dS and Pd, so that both are defined on every 128 x 128 block that
// touches or lies below the diagonal (what the dK / dV products read).  Score, dS, Pd and mask-word tiles above that are neither
// written nor read.  Dropout draws keep their positions in the padded tensor (a masked position's draw is unused).  The blocks of a
// head are handed out longest first (p.rev): they differ in length by nqb x and the short ones fill the end of the grid.
#define NK_ATT_LEFT false   // rows start at key 0 (nk_attention_tile.h)
template <bool BWD, bool MASKED, bool FULL, int OCC, bool KEEP = true, int DH = 64, bool RAGGED = false, bool CAUSAL = false>
__global__ __launch_bounds__(A_NT, OCC) void attention_kernel(const AttnArgs p) {
    static_assert(!(RAGGED && FULL), "ragged sequence lengths take the guarded instantiation");
    constexpr int X1_LD = x1_ld(DH), X2_LD = x2_ld(DH);
    constexpr int ND = DH / 32;   // output column tiles
    constexpr int NR = DH / 32;   // float4 per thread and operand of a staged key tile (32 keys x DH)
    constexpr int C4 = DH / 4;    // float4 per key row
    __shared__ __attribute__((aligned(16))) float x1s[2][32 * X1_LD];
    __shared__ __attribute__((aligned(16))) float x2s[2][32 * X2_LD];
    __shared__ __attribute__((aligned(16))) float scr[A_NT / 64][(BWD ? 2 : 1) * 32 * SCR_LD];  // per wave: tile scratch (backward: dS | Pd)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int q = lane & 31, h = lane >> 5;
    // blocks of one (sample, head) are consecutive in the sequence and one XCD takes a contiguous chunk of it: the 512 KB
    // of K and V a head's blocks share stay in that XCD's L2
    const int seq = nkmma::xcd_chunk(blockIdx.x, gridDim.x);
    const int bh = seq / p.nqb, qb = CAUSAL && p.rev ? p.nqb - 1 - seq % p.nqb : seq % p.nqb;
    const long long samp = (long long)(bh / p.H) * p.S, hoff = (long long)(bh % p.H) * DH;
    const long long flat0 = samp * p.ldx + hoff;   // (sample, head) origin in x1 / x2; bq, ctx and out have their own row strides
    const int q0 = qb * A_QB + w * 32;
    const bool on = FULL ? true : q0 < p.S;  // wave-uniform: the wave has at least one query
    const int SP = RAGGED ? p.SP : p.S;
    const int nt = CAUSAL ? min(p.ntile, 4 * qb + 4) : p.ntile;   // key tiles this block walks
    const int dk = 4 * qb + w;                                    // causal: this wave's diagonal tile (< ntile whenever `on`)
    const float* x1 = p.x1 + flat0;
    const float* x2 = p.x2 + flat0;

    // ---- cooperative staging of one key tile (32 keys x DH of each operand): NR + NR float4 per thread ------------------
    unsigned goff[NR], goff_last[NR], s1[NR], s2[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int idx = tid + A_NT * r, key = idx / C4, c4 = idx % C4;
        goff[r] = (unsigned)(key * p.ldx + 4 * c4);
        goff_last[r] = RAGGED ? (unsigned)(min(key, p.S - 1 - 32 * (p.ntile - 1)) * p.ldx + 4 * c4) : goff[r];  // last key tile: rows clamped to S - 1
        // mfma row i supplies key 16*((i>>2)&1) + 4*(i>>3) + (i&3); its inverse places key 16a + 4b + c in row 8b + 4a + c
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
        // sum_k dP_k P_k with dP = dPd * noise, while dO . O = sum_k dPd_k P_k noise_k / keep
        if (MASKED) dot *= p.keep;
    }
    f32x16 oacc[ND];  // out^T tiles: oacc[d] holds dh 32 d .. 32 d + 31 of this lane's query
#pragma unroll
    for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[d][e] = 0.f;

    const long long rowbase = ((long long)bh * SP + (on ? q0 : 0)) * SP;  // element index of (row q0, key 0) in the (B*H, SP, SP) tensors
    const uint2 key = make_uint2((unsigned)p.seed, (unsigned)(p.seed >> 32));
    const unsigned long long ctr0 = (unsigned long long)(rowbase + (long long)q * SP) / 8 + 2 * h + p.offset;  // 8 draws per call
    float* scrw = scr[w];
    float* scrb = scrw + (BWD ? 32 * SCR_LD : 0);
    // backward: the score tile of the NEXT iteration, in the coalesced load layout (lane -> rows 8i + lane/8, 16 B each)
    float4 sn0, sn1, sn2, sn3;
    unsigned mkn = 0;  // and this row's 32 dropout bits of that tile
    // this wave's mask words: [bh][query tile][kt][q]
    unsigned* const mwave = MASKED ? p.maskbits + (((long long)bh * (SP / 32) + (on ? q0 / 32 : 0)) * p.ntile) * 32 + q : nullptr;
    const unsigned* mload = mwave;
    const float* sload = p.scores + rowbase + (long long)(lane >> 3) * SP + 4 * (lane & 7);
    // no left edge: what the tile body and the macros name of one is constant, and unused under NK_ATT_LEFT false
    constexpr int lo_w = 0, hi_w = -1, kt0 = 0, lo_row = 0;
    const int sld = SP;
    A_STAGE_LOAD(0);
    if (BWD && on) A_SCORES_LOAD(0);
    A_STAGE_STORE(0);
    if (BWD && on) A_SCORES_TO_LDS();
    // every prologue load has landed: without this the compiler's wait-count bookkeeping carries the per-query operand's
    // loads into the loop and waits for the NEXT tile's staging loads in the middle of pass 1, every iteration
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __syncthreads();

    for (int kt = 0; kt < (CAUSAL ? 4 * qb : nt); ++kt) {   // causal: the tiles left of the block's diagonal square (4 qb < nt)
#define NK_ATT_TAIL false
#include "nk_attention_tile.h"
#undef NK_ATT_TAIL
    }
    if constexpr (CAUSAL) {
        for (int kt = 4 * qb; kt < nt; ++kt) {
#define NK_ATT_TAIL true
#include "nk_attention_tile.h"
#undef NK_ATT_TAIL
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
        if (KEEP && h == 0) *reinterpret_cast<float2*>(p.stats + ((long long)bh * SP + qrow) * 2) = make_float2(m_run, inv);
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

template <bool BWD, int DH, bool CAUSAL>
int attention_launch_dh(nk_device* dev, AttnArgs& a, int B, int S, int H, double p, int train, uint64_t seed, uint64_t offset, float scale) {
    a.S = S; a.H = H; a.nqb = (S + A_QB - 1) / A_QB; a.SP = (S + 31) / 32 * 32; a.ntile = a.SP / 32;
    a.scale = scale; a.c1 = scale * 1.44269504088896341f; a.keep = (float)(1.0 - p); a.dscale = 1.f / (1.f - (float)p);  // as nk_scale_softmax_dropout_fwd
    a.seed = seed; a.offset = offset;
    a.rev = 1;   // (a kernel argument, not a template parameter: the ascending order is one word away for a sweep)
    a.keep_lt = nk_keep_threshold(1.0 - p);   // Bernoulli::new(1. - p), node/dropout/mod.rs:46
    const bool masked = train && p != 0.0;
    if (!BWD && masked)   // (the backward reads the forward's stored bits: nothing of its own to freeze)
        if (int rc = nk_refuse_capture(dev, "nk_attention_fwd: the Philox offset (every replay would draw the same mask)",
                                       "run the training-mode dropout eagerly, or capture the evaluation graph")) return rc;
    const dim3 grid((unsigned)(B * H * a.nqb)), block(A_NT);
    const bool full = S % A_QB == 0, ragged = S % 32 != 0;
    // OCC = blocks per CU the register budget is sized for.  DH = 64: three forward blocks fit by LDS (52 KB each) at <= 168
    // VGPRs - the masked forward then spills a few registers and is still faster than two blocks without spills (1.36 vs
    // 1.37 - 1.41 ms at C5, round 3) - and the backward holds 70 KB of LDS per block: two blocks per CU.  DH = 128: 85 / 103 KB
    // of LDS and ~240 / ~290 registers per lane: one block per CU (a wave may then use the whole unified register file).
    // DH = 32: the DH = 64 budgets.
    constexpr int OCC_F = DH == 128 ? 1 : 3, OCC_B = DH == 128 ? 1 : 2;   // forward / backward blocks per CU
    constexpr int OCC_DEFAULT = BWD ? OCC_B : OCC_F;
    // (the causal kernels have no two-block variant: the knob is a sweep tool and every instantiation is compile time)
    const bool occ2 = !CAUSAL && !BWD && DH != 128 && dev->tune_attn_occ == 2;   // (nk_dev_tune, NK_TUNE_ATTENTION_OCC: sweeps only)
#define NK_ATT(M, F, R)                                                                                                    \
    do {                                                                                                                   \
        /* inference forward: KEEP = false (spelled `BWD`, false on the only path that reaches this line) */             \
        if (!BWD && !a.scores) hipLaunchKernelGGL((attention_kernel<BWD, M, F, OCC_DEFAULT, BWD, DH, R, CAUSAL>), grid, block, 0, dev->compute, a); \
        else if (occ2) hipLaunchKernelGGL((attention_kernel<BWD, M, F, (DH == 128 || CAUSAL ? OCC_DEFAULT : 2), true, DH, R, CAUSAL>), grid, block, 0, dev->compute, a); \
        else hipLaunchKernelGGL((attention_kernel<BWD, M, F, OCC_DEFAULT, true, DH, R, CAUSAL>), grid, block, 0, dev->compute, a);    \
    } while (0)
    if (ragged) { if (masked) NK_ATT(true, false, true); else NK_ATT(false, false, true); }
    else if (masked && full) NK_ATT(true, true, false);
    else if (masked) NK_ATT(true, false, false);
    else if (full) NK_ATT(false, true, false);
    else NK_ATT(false, false, false);
#undef NK_ATT
    NK_LAUNCH_CHECK();
    return NK_OK;
}

template <bool BWD, bool CAUSAL>
int attention_launch_c(nk_device* dev, AttnArgs& a, int B, int S, int H, int dh, double p, int train, uint64_t seed, uint64_t offset, float scale) {
    if (dh == 32) return attention_launch_dh<BWD, 32, CAUSAL>(dev, a, B, S, H, p, train, seed, offset, scale);
    if (dh == 128) return attention_launch_dh<BWD, 128, CAUSAL>(dev, a, B, S, H, p, train, seed, offset, scale);
    return attention_launch_dh<BWD, 64, CAUSAL>(dev, a, B, S, H, p, train, seed, offset, scale);
}
template <bool BWD>
int attention_launch(nk_device* dev, AttnArgs& a, bool causal, int B, int S, int H, int dh, double p, int train, uint64_t seed, uint64_t offset,
                     float scale) {
    return causal ? attention_launch_c<BWD, true>(dev, a, B, S, H, dh, p, train, seed, offset, scale)
                  : attention_launch_c<BWD, false>(dev, a, B, S, H, dh, p, train, seed, offset, scale);
}
// algorithmic flops of one direction's two products: all S*S (query, key) pairs, or the S*(S+1)/2 on and below the diagonal
double attention_flops(bool causal, int B, int S, int H, int dh) {
    return causal ? 2.0 * B * H * dh * (double)S * (S + 1) : 4.0 * B * H * (double)S * S * dh;
}

}  // namespace

extern "C" {

int nk_attention_supported(int S, int dh, double p, int train) {
    return (dh == 32 || dh == 64 || dh == 128) && S > 0 && !(train && 1.0 - p == 0.0);
}

static int attention_fwd_impl(nk_device* dev, bool causal, const float* Q, const float* K, const float* V, int ld_qkv, float* scores, float* stats,
                              uint32_t* mask_bits, float* O, int B, int S, int H, int dh, float scale, double p, int train, uint64_t seed,
                              uint64_t offset) {
    NK_USE(dev);
    if (int rc = attention_check(B, S, H, dh, p, train, scale, (S + 31) / 32 * 32)) return rc;
    NK_CHECK(Q && K && V && O, "null pointer in nk_attention_fwd");
    NK_CHECK((scores != nullptr) == (stats != nullptr), "nk_attention_fwd: scores and stats are kept together or not at all");
    NK_CHECK(!scores || mask_bits || !(train && p != 0.0), "nk_attention_fwd: dropout is active, the mask_bits buffer is needed");
    NK_CHECK(attn_al16(Q) && attn_al16(K) && attn_al16(V) && attn_al16(scores) && attn_al16(O) && attn_al16(stats),
             "nk_attention_fwd needs 16-byte aligned buffers");
    NK_CHECK((long long)B * S * ld_qkv < (1ll << 31), "attention: the packed projection layout exceeds 2^31 elements");
    nk_prof_start(dev, NK_KERNEL_ATTENTION, attention_flops(causal, B, S, H, dh));
    AttnArgs a{};
    a.x1 = K; a.x2 = V; a.bq = Q; a.out = O; a.scores = scores; a.stats = stats; a.maskbits = mask_bits;
    a.ldx = ld_qkv; a.ldq = ld_qkv; a.ldc = H * dh; a.ldo = H * dh;
    const int rc = attention_launch<false>(dev, a, causal, B, S, H, dh, p, train, seed, offset, scale);
    nk_prof_stop(dev);
    return rc;
}
int nk_attention_fwd(nk_device* dev, const float* Q, const float* K, const float* V, float* scores, float* stats,
                     uint32_t* mask_bits, float* O, int B, int S, int H, int dh, float scale, double p, int train, uint64_t seed,
                     uint64_t offset) {
    return attention_fwd_impl(dev, false, Q, K, V, H * dh, scores, stats, mask_bits, O, B, S, H, dh, scale, p, train, seed, offset);
}
int nk_attention_causal_fwd(nk_device* dev, const float* Q, const float* K, const float* V, float* scores, float* stats,
                            uint32_t* mask_bits, float* O, int B, int S, int H, int dh, float scale, double p, int train, uint64_t seed,
                            uint64_t offset) {
    return attention_fwd_impl(dev, true, Q, K, V, H * dh, scores, stats, mask_bits, O, B, S, H, dh, scale, p, train, seed, offset);
}
static int attention_qkv_fwd_impl(nk_device* dev, bool causal, const float* QKV, float* scores, float* stats, uint32_t* mask_bits, float* O,
                                  int B, int S, int H, int dh, float scale, double p, int train, uint64_t seed, uint64_t offset) {
    NK_CHECK(QKV != nullptr, "null pointer in nk_attention_qkv_fwd");
    const int d = H * dh;
    return attention_fwd_impl(dev, causal, QKV, QKV + d, QKV + 2 * d, 3 * d, scores, stats, mask_bits, O, B, S, H, dh, scale, p, train, seed,
                              offset);
}
int nk_attention_qkv_fwd(nk_device* dev, const float* QKV, float* scores, float* stats, uint32_t* mask_bits, float* O, int B, int S,
                         int H, int dh, float scale, double p, int train, uint64_t seed, uint64_t offset) {
    return attention_qkv_fwd_impl(dev, false, QKV, scores, stats, mask_bits, O, B, S, H, dh, scale, p, train, seed, offset);
}
int nk_attention_qkv_causal_fwd(nk_device* dev, const float* QKV, float* scores, float* stats, uint32_t* mask_bits, float* O, int B, int S,
                                int H, int dh, float scale, double p, int train, uint64_t seed, uint64_t offset) {
    return attention_qkv_fwd_impl(dev, true, QKV, scores, stats, mask_bits, O, B, S, H, dh, scale, p, train, seed, offset);
}

static int attention_bwd_impl(nk_device* dev, bool causal, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO, const float* O,
                              const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q, const float* K,
                              const float* V, int ld_qkv, int B, int S, int H, int dh, float scale, double p, int train, int assign_dq,
                              int assign_dk, int assign_dv) {
    NK_USE(dev);
    if (int rc = attention_check(B, S, H, dh, p, train, scale, (S + 31) / 32 * 32)) return rc;
    NK_CHECK(dQ && dK && dV && dS && dropped && dO && O && scores && stats && Q && K && V, "null pointer in nk_attention_bwd");
    NK_CHECK(mask_bits || !(train && p != 0.0), "nk_attention_bwd: dropout is active, the forward's mask_bits are needed");
    NK_CHECK(attn_al16(dQ) && attn_al16(dK) && attn_al16(dV) && attn_al16(dS) && attn_al16(dropped) && attn_al16(dO) && attn_al16(O) &&
                 attn_al16(scores) && attn_al16(stats) && attn_al16(Q) && attn_al16(K) && attn_al16(V),
             "nk_attention_bwd needs 16-byte aligned buffers");
    NK_CHECK((long long)B * S * ld_qkv < (1ll << 31), "attention: the packed projection layout exceeds 2^31 elements");
    nk_prof_start(dev, NK_KERNEL_ATTENTION, attention_flops(causal, B, S, H, dh));
    AttnArgs a{};
    a.x1 = V; a.x2 = K; a.bq = dO; a.ctx = O; a.out = dQ; a.scores = const_cast<float*>(scores); a.ds = dS; a.dropped = dropped;
    a.stats = const_cast<float*>(stats); a.maskbits = const_cast<uint32_t*>(mask_bits); a.assign = assign_dq ? 1 : 0;
    a.ldx = ld_qkv; a.ldq = H * dh; a.ldc = H * dh; a.ldo = ld_qkv;
    int rc = attention_launch<true>(dev, a, causal, B, S, H, dh, p, train, 0, 0, scale);
    nk_prof_stop(dev);
    if (rc) return rc;
    // dK_bh (+)= dS_bh^T . Q_bh and dV_bh (+)= Pd_bh^T . dO_bh: reductions over the queries, i.e. across the blocks above.
    // (Keeping dS / Pd in the kernels' own tile order - no LDS transposition in the kernel, a k-contiguous A operand whose
    // 128 x 32 tiles are single 16 KB runs for these products - was built and measured: kernel and products unchanged.)
    const int d = H * dh, SP = (S + 31) / 32 * 32;  // row stride of the scratch tensors (== S unless S is ragged)
    const long long so = (long long)S * d, sq = (long long)S * ld_qkv, po = (long long)H * SP * SP, pi = (long long)SP * SP;
    // Causal: dS and Pd are defined on the 128 x 128 blocks that touch or lie below the diagonal and UNDEFINED above, so the key strip
    // [128 j, 128 j + 128) reduces over the queries >= 128 j only: K = S - 128 j
    if (causal) return strip_products(dev, dK, dV, dS, dropped, dO, Q, ld_qkv, B, S, H, dh, assign_dk, assign_dv, SP, pi, a.nqb);
    // (one launch for both when nk_sgemm_pair's rule says so: the two grids share their last wave of resident blocks)
    return nk_sgemm_pair_batched(dev, B, H, 1, 0, S, dh, S, dS, SP, po, pi, Q, ld_qkv, sq, dh, assign_dk ? 0.f : 1.f, dK, ld_qkv, sq, dh,
                                 1, 0, S, dh, S, dropped, SP, po, pi, dO, d, so, dh, assign_dv ? 0.f : 1.f, dV, ld_qkv, sq, dh);
}
int nk_attention_bwd(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO, const float* O,
                     const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q, const float* K,
                     const float* V, int B, int S, int H, int dh, float scale, double p, int train, int assign_dq, int assign_dk,
                     int assign_dv) {
    return attention_bwd_impl(dev, false, dQ, dK, dV, dS, dropped, dO, O, scores, stats, mask_bits, Q, K, V, H * dh, B, S, H, dh, scale, p, train,
                              assign_dq, assign_dk, assign_dv);
}
int nk_attention_causal_bwd(nk_device* dev, float* dQ, float* dK, float* dV, float* dS, float* dropped, const float* dO, const float* O,
                            const float* scores, const float* stats, const uint32_t* mask_bits, const float* Q, const float* K,
                            const float* V, int B, int S, int H, int dh, float scale, double p, int train, int assign_dq, int assign_dk,
                            int assign_dv) {
    return attention_bwd_impl(dev, true, dQ, dK, dV, dS, dropped, dO, O, scores, stats, mask_bits, Q, K, V, H * dh, B, S, H, dh, scale, p, train,
                              assign_dq, assign_dk, assign_dv);
}
static int attention_qkv_bwd_impl(nk_device* dev, bool causal, float* dQKV, float* dS, float* dropped, const float* dO, const float* O,
                                  const float* scores, const float* stats, const uint32_t* mask_bits, const float* QKV, int B, int S, int H,
                                  int dh, float scale, double p, int train, int assign) {
    NK_CHECK(dQKV && QKV, "null pointer in nk_attention_qkv_bwd");
    const int d = H * dh;
    return attention_bwd_impl(dev, causal, dQKV, dQKV + d, dQKV + 2 * d, dS, dropped, dO, O, scores, stats, mask_bits, QKV, QKV + d, QKV + 2 * d,
                              3 * d, B, S, H, dh, scale, p, train, assign, assign, assign);
}
int nk_attention_qkv_bwd(nk_device* dev, float* dQKV, float* dS, float* dropped, const float* dO, const float* O, const float* scores,
                         const float* stats, const uint32_t* mask_bits, const float* QKV, int B, int S, int H, int dh, float scale,
                         double p, int train, int assign) {
    return attention_qkv_bwd_impl(dev, false, dQKV, dS, dropped, dO, O, scores, stats, mask_bits, QKV, B, S, H, dh, scale, p, train, assign);
}
int nk_attention_qkv_causal_bwd(nk_device* dev, float* dQKV, float* dS, float* dropped, const float* dO, const float* O, const float* scores,
                                const float* stats, const uint32_t* mask_bits, const float* QKV, int B, int S, int H, int dh, float scale,
                                double p, int train, int assign) {
    return attention_qkv_bwd_impl(dev, true, dQKV, dS, dropped, dO, O, scores, stats, mask_bits, QKV, B, S, H, dh, scale, p, train, assign);
}

}  // extern "C"
