// The body of the vector partial kernels of single-query attention (nk_attention_decode.h says what they compute).  No kernel of its
// own and no include guard: it is included INSIDE the signatures of adec_partial_kernel<DH>, adec_gqa_partial_kernel<DH> and
// adw_partial_kernel<DH, NH> (and of the paged adp_partial_kernel / adpw_partial_kernel<DH, NH>), so they are one body by construction - the bits of a head's result are the same in all three
// whenever its keys are, and a change to the arithmetic is made once.  (A force-inlined function called from the three moved their
// register allocation; a textual body does not - profiles/attention_decode_isa_identity.md.)  The includer defines, and undefines
// after the include:
//   ADEC_GROUPED  0: one block per (b, t, h), blockIdx.x = (b*T + t)*H + h; the kernel has the argument H.
//                 1: one block per ((b, t, kv head), batch of at most ADEC_NH query heads of its group); arguments H and Hkv.
//   ADEC_NH       query heads a block serves from one read of its chunk (1 when ADEC_GROUPED is 0).
//   ADEC_WINDOW   0: positions j < n count, position j lives at slot j, blockIdx.y is the chunk; argument nchunks.
//                 1: positions lo <= j < n count, position j lives at slot s0 + (j - lo) wrapped at cap, blockIdx.y counts the chunks
//                    from lo / C; arguments W and ring, and nchunks is the number of chunks a window can touch.
//   ADEC_PAGED    0: the cache is one (B, Hkv, cap, dh) slab, slot s of the block's kv head at base + s * LPK.
//                 1: (nk_attention_decode_paged.h) pools of pages (num_pages, Hkv, page, dh) and a table: position p is in page
//                    table[b*max_pages + (p >> psh)], clamped to np1 = num_pages - 1, at slot p & (page - 1); arguments table,
//                    max_pages, psh, np1, and cap is the virtual capacity max_pages << psh.
// The forms differ in five places, marked (1) - (5); everything else - the loads, dot, xor-shuffles, chunk maximum, exp2, the groups
// in order, the write of o / ls or of the partial - is stated once.
    constexpr int LPK = DH / 4, G = ADEC_THREADS / LPK, C = G * ADEC_KPG;
    static_assert(C == adec_chunk_of(DH), "chunk");
    __shared__ float4 ro[G * LPK];
    __shared__ float rl[G];
    __shared__ float red[ADEC_THREADS / 64];
    const int tid = threadIdx.x, g = tid / LPK, sub = tid % LPK;
    // (1) how a block finds its heads: query heads h0 .. h0 + nh - 1 of row b*T + t, over kv head kvh of Hkv
#if ADEC_GROUPED
    const int R = H / Hkv, nb = (R + ADEC_NH - 1) / ADEC_NH;
    const int hb = blockIdx.x % nb, pk = blockIdx.x / nb;
    const int row = pk / Hkv, kvh = pk % Hkv, b = row / T, t = row % T;
    const int h0 = kvh * R + hb * ADEC_NH, nh = ADEC_NH == 1 ? 1 : (R - hb * ADEC_NH < ADEC_NH ? R - hb * ADEC_NH : ADEC_NH);
#else
    const int pk = blockIdx.x;
    const int row = pk / H, h0 = pk % H, b = row / T, t = row % T;
    const int Hkv = H, kvh = h0;
    constexpr int nh = 1, hq = 0;
#endif
    // (2) which positions count, (3) where a position lives - one that does not count is redirected to position n - 1, which does -
    // and (4) what "one chunk" means
#if ADEC_WINDOW
    const int n = adec_len(start, b, t, cap, ring), lo = n > W ? n - W : 0;
    const unsigned wc = blockIdx.y;  // the chunk's place among the problem's in the workspace: counted from lo / C
#define ADEC_NONE (n <= 0)
#define ADEC_IN(i) ((unsigned)(r0 + (i) * G) < wn)
#define ADEC_AT(i) adec_wrap(s0 + (ADEC_IN(i) ? r0 + (i) * G : (int)wn - 1), cap)
#define ADEC_SINGLE (cf == cl)
#else
    const int wc = blockIdx.y;  // the chunk, and its place in the workspace
    const int n = adec_len(start, b, t, cap, 0), c0 = wc * C;
#define ADEC_NONE (c0 >= n)
#define ADEC_IN(i) (c0 + (i) * G + g < n)
#define ADEC_AT(i) (ADEC_IN(i) ? c0 + (i) * G + g : n - 1)
#define ADEC_SINGLE (n <= C)
#endif
    float* __restrict__ out = O + (size_t)row * H * DH + (size_t)h0 * DH;  // the block's nh heads are contiguous columns
    if (ADEC_NONE) {  // the same decision in every thread of the block
        if (wc == 0)
            for (int e = tid; e < nh * DH; e += ADEC_THREADS) out[e] = 0.f;
        return;
    }
#if ADEC_WINDOW
    const int cf = lo / C, cl = (n - 1) / C, chunk = cf + (int)wc;
    if (chunk > cl) return;
    const int s0 = ring ? lo % cap : lo;  // the slot of position lo
    // positions relative to lo: key i of this lane group is r0 + i * G, inside the window iff 0 <= r < wn - ONE unsigned compare,
    // the cost of "position < n"
    const int r0 = chunk * C + g - lo;
    const unsigned wn = (unsigned)(n - lo);
#endif
    // a block of one head asks for its query before its keys and has no head loop; a batch of heads asks head by head, after the keys.
    // (Where the forms keep an order of their own - here, and in wc's signedness - the order is part of their machine code: one place
    // for the query moved each one-head kernel by an instruction, a head loop of one trip by up to 5.)
#define ADEC_Q(h)                                                                      \
    const float* __restrict__ qp = Q + (size_t)row * ldq + (size_t)(h) * DH + sub * 4; \
    const float4 q = make_float4(qp[0], qp[1], qp[2], qp[3])
#if !ADEC_GROUPED
    ADEC_Q(h0);
#endif
    // (5) where a position's row is in memory: at base + slot * LPK of one slab, or in the page the sample's table row names
#if !ADEC_PAGED
    const size_t base = ((size_t)b * Hkv + kvh) * cap * LPK + sub;
#endif
    float4 kk[ADEC_KPG], vv[ADEC_KPG];
#if ADEC_PAGED
    // the 16 table entries first, then the 16 + 16 loads they address: one dependent-load latency per chunk.  Only positions that
    // count (or n - 1) are looked up; the entry is clamped into the pool
    const int* __restrict__ trow = table + (size_t)b * max_pages;
    unsigned at[ADEC_KPG];
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i) at[i] = (unsigned)trow[ADEC_AT(i) >> psh];
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i)
        at[i] = ((((at[i] < np1 ? at[i] : np1) * Hkv + kvh) << psh) + (ADEC_AT(i) & ((1 << psh) - 1))) * LPK + sub;
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i) kk[i] = Kc[at[i]];
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i) vv[i] = Vc[at[i]];
#else
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i) kk[i] = Kc[base + (size_t)ADEC_AT(i) * LPK];
#pragma unroll
    for (int i = 0; i < ADEC_KPG; ++i) vv[i] = Vc[base + (size_t)ADEC_AT(i) * LPK];
#endif
#if ADEC_GROUPED
#pragma unroll 1
    for (int hq = 0; hq < nh; ++hq)  // head by head over the registers above
#endif
    {
#if ADEC_GROUPED
        ADEC_Q(h0 + hq);
#endif
        float s[ADEC_KPG], m = -INFINITY;
#pragma unroll
        for (int i = 0; i < ADEC_KPG; ++i) {
            float d = q.x * kk[i].x;
            d = __builtin_fmaf(q.y, kk[i].y, d);
            d = __builtin_fmaf(q.z, kk[i].z, d);
            d = __builtin_fmaf(q.w, kk[i].w, d);
#pragma unroll
            for (int off = LPK / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
            s[i] = ADEC_IN(i) ? d * c1 : -INFINITY;
            m = fmaxf(m, s[i]);
        }
        m = nk_wave_max(m);
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));  // finite: a visited chunk holds a key that counts
        float l = 0.f;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < ADEC_KPG; ++i) {
            const float p = ADEC_IN(i) ? __builtin_amdgcn_exp2f(s[i] - m) : 0.f;
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
            if (ADEC_SINGLE) {
                out[hq * DH + tid] = o / ls;
            } else {
                const size_t prob = ADEC_GROUPED ? (size_t)row * H + h0 + hq : (size_t)pk;  // (b*T + t)*H + h
                float* __restrict__ part = ws + (prob * nchunks + wc) * (DH + 2);
                part[tid] = o;
                if (tid == 0) {
                    part[DH] = m;
                    part[DH + 1] = ls;
                }
            }
        }
    }
#undef ADEC_Q
#undef ADEC_NONE
#undef ADEC_IN
#undef ADEC_AT
#undef ADEC_SINGLE
