// The body of the generic kernels of single-query attention (any dh but 32 / 64 / 128; nk_attention_decode.h says what they compute).
// No kernel of its own and no include guard: it is included INSIDE the signatures of adec_generic_kernel, adec_gqa_generic_kernel and
// adw_generic_kernel (and of the paged adp_generic_kernel / adpw_generic_kernel), as nk_attention_decode_body.h is inside the vector kernels'.  One block per (b, t, h) in all three; nothing is
// shared between the heads of a group.  The includer defines, and undefines after the include:
//   ADEC_GROUPED  1: the cache has Hkv heads and query head h reads head h / (H / Hkv); argument Hkv.  0: head h.
//   ADEC_WINDOW   as in nk_attention_decode_body.h: arguments W and ring, and nchunks counts the chunks a window can touch.
//   ADEC_PAGED    as in nk_attention_decode_body.h: 0 one slab, 1 pages behind a table (arguments table, max_pages, psh, np1).
    constexpr int C = ADEC_CHUNK_GENERIC;
    static_assert(C == ADEC_THREADS, "one key per thread");
    __shared__ float sc[C];
    __shared__ float ro[ADEC_THREADS];
    __shared__ float red[ADEC_THREADS / 64];
    const int tid = threadIdx.x, G = ADEC_THREADS / lpk, g = tid / lpk, sub = tid & (lpk - 1);  // lpk keys per group: C / G
    const int prob = blockIdx.x;
#if !ADEC_WINDOW
    const int chunk = blockIdx.y;
#endif
    const int row = prob / H, h = prob % H, b = row / T, t = row % T;
    // which positions count, where a position lives - one that does not count is redirected to position n - 1, which does - and what
    // "one chunk" means
#if ADEC_WINDOW
    const int n = adec_len(start, b, t, cap, ring), lo = n > W ? n - W : 0;
#define ADEC_WC blockIdx.y  // the chunk's place among the problem's in the workspace: counted from lo / C
#define ADEC_NONE (n <= 0)
#define ADEC_IN(j) ((j) >= lo && (j) < n)
#define ADEC_REL(j) (s0 + (ADEC_IN(j) ? (j) : n - 1) - lo)  // the slot before the wrap
#define ADEC_AT(r) adec_wrap(r, cap)
#define ADEC_SINGLE (cf == cl)
#else
    const int n = adec_len(start, b, t, cap, 0), c0 = chunk * C;
#define ADEC_WC chunk  // the chunk is its place in the workspace
#define ADEC_NONE (c0 >= n)
#define ADEC_IN(j) ((j) < n)
#define ADEC_REL(j) (j)
#define ADEC_AT(r) ((r) < n ? (r) : n - 1)
#define ADEC_SINGLE (n <= C)
#endif
    float* __restrict__ out = O + (size_t)row * H * dh + (size_t)h * dh;
    if (ADEC_NONE) {
        if (ADEC_WC == 0)
            for (int e = tid; e < dh; e += ADEC_THREADS) out[e] = 0.f;
        return;
    }
#if ADEC_WINDOW
    const int cf = lo / C, cl = (n - 1) / C, chunk = cf + (int)ADEC_WC;
    if (chunk > cl) return;
    const int c0 = chunk * C;
    const int s0 = ring ? lo % cap : lo;  // the slot of position lo
#endif
    const float* __restrict__ qp = Q + (size_t)row * ldq + (size_t)h * dh;
    // where slot s of the block's kv head starts: in one slab, or in the page the sample's table row names (the entry clamped into
    // the pool; only slots of positions that count, or of n - 1, are looked up)
#if ADEC_PAGED
    const int* __restrict__ trow = table + (size_t)b * max_pages;
    const unsigned kvh = h / (H / Hkv);
#define ADEC_ROW(s) \
    (((((size_t)((unsigned)trow[(s) >> psh] < np1 ? (unsigned)trow[(s) >> psh] : np1) * Hkv + kvh) << psh) + ((s) & ((1 << psh) - 1))) * dh)
#else
#define ADEC_ROW(s) base + (size_t)(s) * dh  // unparenthesised: Kc + base + ..., the association the three kernels were compiled with
#if ADEC_GROUPED
    const size_t base = ((size_t)b * Hkv + h / (H / Hkv)) * cap * dh;
#else
    const size_t base = ((size_t)b * H + h) * cap * dh;
#endif
#endif
    for (int i = 0; i < lpk; ++i) {
        const int j = c0 + i * G + g, r = ADEC_REL(j);
        const float* __restrict__ kr = Kc + ADEC_ROW(ADEC_AT(r));
        float d = 0.f;
        for (int e = sub; e < dh; e += lpk) d = __builtin_fmaf(qp[e], kr[e], d);
        for (int off = lpk >> 1; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
        if (sub == 0) sc[i * G + g] = ADEC_IN(j) ? d * c1 : -INFINITY;
    }
    __syncthreads();
    const float sv = sc[tid];
    const float m = nk_block_max<ADEC_THREADS>(sv, red);
    const float p = ADEC_IN(c0 + tid) ? __builtin_amdgcn_exp2f(sv - m) : 0.f;
    const float l = nk_block_sum<ADEC_THREADS>(p, red);
    sc[tid] = p;  // a thread's own slot
    __syncthreads();
    const bool single = ADEC_SINGLE;
    float* __restrict__ part = ws + ((size_t)prob * nchunks + ADEC_WC) * ((size_t)dh + 2);
    for (int e0 = 0; e0 < dh; e0 += lpk) {
        const int e = e0 + sub;
        float acc = 0.f;
        if (e < dh)
            for (int i = 0; i < lpk; ++i) {
                const int jl = i * G + g, j = c0 + jl, r = ADEC_REL(j);
                acc = __builtin_fmaf(sc[jl], Vc[ADEC_ROW(ADEC_AT(r)) + e], acc);
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
#undef ADEC_WC
#undef ADEC_NONE
#undef ADEC_IN
#undef ADEC_REL
#undef ADEC_AT
#undef ADEC_ROW
#undef ADEC_SINGLE
