// One key tile of the walk of attention_kernel (nk_attention.hip) and attention_band_kernel (nk_attention_band.h): the loop body, included
// inside every loop of both kernels, as nk_gemm.hip does with nk_gemm_body.h and for the same reason: a body under a run-time branch
// makes the compiler wait for every outstanding vector memory operation at the join, so the tiles that are whole for all four waves get
// a copy without any predicate - and the body as a force-inlined generic lambda moved every instantiation's register allocation and
// instruction count.  Not a stand-alone header.  The including loop sets
//   NK_ATT_TAIL   false: the tile is whole for every wave of the block that has queries (the body under `on` alone)
//                 true:  an edge tile - of a causal block's diagonal square (see CAUSAL in nk_attention.hip) or of a band block's left edge
//                        (nk_attention_band.h) - per-wave predicate, element masks, zero tiles of dS / Pd where the wave computes nothing
//   NK_ATT_LEFT   false: rows start at key 0 (nk_attention.hip).  Predicate kt <= dk, element mask k > r when kt == dk.  The left-edge
//                        names below are declared all the same and never read: a `kt >= 0` the compiler cannot prove costs a compare
//                 true:  rows have a left edge.  Predicate lo_w <= kt <= dk, element mask k < lo_row where kt <= hi_w as well
// and has in scope everything the kernel declares above its loops, the loop variable `kt`, and
//   lo_w, hi_w    this wave's first tile, and its last tile that holds a key left of some row's edge (-1: none)
//   lo_row        this lane's row's first key
//   kt0           the first key tile the block stages: the mask words of a query tile are counted from it
//   sld           row stride of scores, dS and Pd
//   KEEP          (forward) scores, row statistics and dropout bits are written for a backward pass
        const int cur = kt & 1;
        const bool more = kt + 1 < nt;
        if (more) A_STAGE_LOAD(kt + 1);
        const bool next = NK_ATT_TAIL ? kt < dk : more;   // this wave computes tile kt + 1 (main part: every tile up to the diagonal exists)
        if (NK_ATT_TAIL ? on && (!NK_ATT_LEFT || kt >= lo_w) && kt <= dk : on) {
            float sv[16];
            unsigned mybits = 0;
            if (BWD) {  // score tile (put into the scratch at the end of the previous iteration) -> lane layout; fetch the next one
                if (MASKED) mybits = mkn >> (16 * h);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float4 t = *reinterpret_cast<const float4*>(&scrw[q * SCR_LD + 16 * h + 4 * c]);
                    sv[4 * c] = t.x; sv[4 * c + 1] = t.y; sv[4 * c + 2] = t.z; sv[4 * c + 3] = t.w;
                }
                if (next) A_SCORES_LOAD(kt + 1);
            }
            // ---- pass 1: C[key][query] = X1 . Bq^T  (forward: scores; backward: dPd) -------------------------------
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.f;
            {
                const float* a1 = &x1s[cur][q * X1_LD + 4 * h];
#pragma unroll
                for (int j = 0; j < DH / 8; ++j) {
                    const float4 a = *reinterpret_cast<const float4*>(a1 + 8 * j);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bq[j].x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bq[j].y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, bq[j].z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, bq[j].w, acc, 0, 0, 0);
                }
            }
            // Bernoulli(1 - p) draws of this lane's 16 keys.  Forward: 2 Philox calls (8 consecutive keys each, the draw
            // layout of nk_common.h / nk_dropout_fwd / nk_scale_softmax_dropout_fwd), packed to one bit per score for the
            // backward pass - the Philox rounds were ~2000 of the ~6500 issue cycles of a masked tile with one word per
            // score (v_mad_u64_u32 is quarter rate) and are paid once, not twice; the backward mask is the forward's by
            // construction (the reference shares the noise buffer the same way, node/dropout/mod.rs:113-128).
            bool kp[16];          // forward: the compare results stay lane masks in SGPR pairs (the masked forward is at its VGPR limit)
            int km[16];           // backward: 0 / -1 per key as AND operands (one v_bfe_i32 + one v_and per use instead of bit test + compare + select)
            if (MASKED && !BWD) {
                unsigned bits = 0;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const unsigned long long ctr = ctr0 + (unsigned long long)(kt * 4 + c);
                    const uint4 r = philox4x32_10(make_uint4((unsigned)ctr, (unsigned)(ctr >> 32), 0u, 0u), key);
                    const unsigned wv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const bool k0 = wv[k] < p.keep_lt, k1 = nk_rot16(wv[k]) < p.keep_lt;
                        kp[8 * c + 2 * k] = k0;
                        kp[8 * c + 2 * k + 1] = k1;
                        bits |= (k0 ? 1u : 0u) << (8 * c + 2 * k);
                        bits |= (k1 ? 1u : 0u) << (8 * c + 2 * k + 1);
                    }
                }
                const unsigned other = (unsigned)__shfl_xor((int)bits, 32, 64);
                if (KEEP && h == 0) mwave[(kt - kt0) * 32] = bits | (other << 16);
            }
            if (MASKED && BWD) {
#pragma unroll
                for (int e = 0; e < 16; ++e) km[e] = __builtin_amdgcn_sbfe((int)mybits, e, 1);   // v_bfe_i32: 0 / -1
            }
            float bv[16];  // B operand of pass 2
            if (!BWD) {
                float raw[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) raw[e] = acc[e];
                if (RAGGED && kt == p.ntile - 1) {  // keys beyond S: probability exactly 0, here and (through the stored score) in the backward
                    const int nvalid = p.S - 32 * kt - 16 * h;
#pragma unroll
                    for (int e = 0; e < 16; ++e) raw[e] = e < nvalid ? raw[e] : -INFINITY;
                }
                if (NK_ATT_LEFT) {
                    if (NK_ATT_TAIL && (kt <= hi_w || kt == dk)) {  // (wave-uniform) an edge of the band crosses this tile
                        // key 32 kt + 16 h + e is kept iff lo_row <= key <= qrow: e in (elo, ehi].  The left bound is the CLAMPED row's, so a
                        // padded query stays a copy of row S - 1 and no row is empty; every row keeps its diagonal
                        const int elo = kt <= hi_w ? lo_row - 1 - 32 * kt - 16 * h : -1;
                        const int ehi = kt == dk ? q - 16 * h : 15;
#pragma unroll
                        for (int e = 0; e < 16; ++e) raw[e] = (e > elo && e <= ehi) ? raw[e] : -INFINITY;
                    }
                } else if (NK_ATT_TAIL && kt == dk) {  // the diagonal tile: keys above the query (every row keeps its diagonal, no row is empty)
#pragma unroll
                    for (int e = 0; e < 16; ++e) raw[e] = 16 * h + e <= q ? raw[e] : -INFINITY;
                }
                if (KEEP) tile_write(scrw, raw, lane);
                // Online softmax in the base-2 exponent domain: exp(s*scale - m) = exp2(s*c1 - m2), c1 = scale*log2(e), one fma
                // and one v_exp_f32 per element.  f32 MFMA and VALU instructions do NOT overlap on a SIMD (measured,
                // benchmarks/native/mfma_valu_overlap.hip: both run on the f32 lanes), so every VALU instruction here is
                // paid in full on top of the 64 MFMAs of the tile.
                float rmax = raw[0];
#pragma unroll
                for (int e = 1; e < 16; ++e) rmax = fmaxf(rmax, raw[e]);   // scale > 0: max of the scaled = scaled max
                rmax = fmaxf(rmax, __shfl_xor(rmax, 32, 64));
                const float tm2 = rmax * p.c1;
                // The running max only has to bound the exponents, not equal the true max: it moves when a tile exceeds it by
                // more than 2^6 (terms stay <= 64, sums <= 2^16), i.e. after the first tile practically never, and the rescale
                // of the 32 accumulator registers is skipped (wave-uniform test).  Softmax is invariant to the shift, and the
                // backward pass recomputes the probabilities with the stored (shift, 1 / sum) pair.
                if (__any(tm2 > m_run + 6.f)) {
                    const float m_new = fmaxf(m_run, tm2);
                    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
                    l_run *= alpha;
                    m_run = m_new;
#pragma unroll
                    for (int d = 0; d < ND; ++d)
#pragma unroll
                        for (int e = 0; e < 16; ++e) oacc[d][e] *= alpha;
                }
                float ps = 0.f;
#pragma unroll
                for (int e = 0; e < 16; ++e) { sv[e] = __builtin_amdgcn_exp2f(__builtin_fmaf(raw[e], p.c1, -m_run)); ps += sv[e]; }
                ps += __shfl_xor(ps, 32, 64);
                l_run += ps;
                // Dropout: the 1 / (1 - p) factor is applied once, with the normalisation, in the epilogue
#pragma unroll
                for (int e = 0; e < 16; ++e) bv[e] = MASKED ? (kp[e] ? sv[e] : 0.f) : sv[e];
            } else {
                float pd[16];
                const float inv_s = l_run * p.scale;                      // P * scale = e * (1/sum * scale)
                const float inv_d = MASKED ? l_run * p.dscale : l_run;    // Pd = e * (1/sum * 1/(1-p)) where kept
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float ev = __builtin_amdgcn_exp2f(__builtin_fmaf(sv[e], p.c1, -m_run));  // exp(s*scale - shift), as the forward
                    const float gv = MASKED ? __int_as_float(__float_as_int(acc[e]) & km[e]) : acc[e];  // DropoutBackward: g * noise
                    bv[e] = (ev * inv_s) * (gv - dot);                           // SoftmaxBackward, MultiplicationBackwardLeft
                    pd[e] = MASKED ? __int_as_float(__float_as_int(ev * inv_d) & km[e]) : ev * inv_d;    // Dropout forward (for dV = Pd^T . dO)
                }
                tile_write(scrw, bv, lane);   // (the score tile was read out of this region at the top of the iteration)
                tile_write(scrb, pd, lane);
            }
            // ---- pass 2: out^T[dh][query] += X2^T . C ----------------------------------------------------------------
            {
                // column tile d of the output reads dh column 32 d + q of the key rows 16 h + e, stored rotated by 32 h
                const float* const a2b = &x2s[cur][(16 * h) * X2_LD];
                const int c0 = (q + 32 * h) & (DH - 1), c1 = (q + 32 + 32 * h) & (DH - 1), c2 = (q + 64 + 32 * h) & (DH - 1),
                          c3 = (q + 96 + 32 * h) & (DH - 1);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    oacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2b[e * X2_LD + c0], bv[e], oacc[0], 0, 0, 0);
                    if constexpr (ND > 1) oacc[ND > 1 ? 1 : 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2b[e * X2_LD + c1], bv[e], oacc[ND > 1 ? 1 : 0], 0, 0, 0);
                    if constexpr (ND > 2) {
                        oacc[ND > 2 ? 2 : 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2b[e * X2_LD + c2], bv[e], oacc[ND > 2 ? 2 : 0], 0, 0, 0);
                        oacc[ND > 2 ? 3 : 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a2b[e * X2_LD + c3], bv[e], oacc[ND > 2 ? 3 : 0], 0, 0, 0);
                    }
                }
                (void)c1; (void)c2; (void)c3;
            }
            // ---- the tiles written to the scratch before pass 2 go to HBM now (machine scheduler pinned: hoisting the
            //      ds_reads above the MFMAs would put the LDS round trip back on the critical path) ---------------------
            __builtin_amdgcn_sched_barrier(0);
            wave_lds_handover();
            if (!BWD) {
                if (KEEP) tile_flush(scrw, p.scores + rowbase + kt * 32, sld, lane);
            } else {
                tile_flush(scrw, p.ds + rowbase + kt * 32, sld, lane);
                tile_flush(scrb, p.dropped + rowbase + kt * 32, sld, lane);
                if (next) { wave_lds_handover(); A_SCORES_TO_LDS(); }   // next tile's scores (loaded during this iteration)
            }
        } else if (NK_ATT_TAIL && BWD && on) {   // staged by the block, left of this wave's first tile or right of its diagonal: dS = Pd = 0
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long o = rowbase + kt * 32 + (long long)(8 * i + (lane >> 3)) * sld + 4 * (lane & 7);
                nk_store_stream(reinterpret_cast<float4*>(p.ds + o), make_float4(0.f, 0.f, 0.f, 0.f));
                nk_store_stream(reinterpret_cast<float4*>(p.dropped + o), make_float4(0.f, 0.f, 0.f, 0.f));
            }
        }
        if (more) A_STAGE_STORE(cur ^ 1);
        __syncthreads();
