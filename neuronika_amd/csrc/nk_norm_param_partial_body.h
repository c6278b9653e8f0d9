// The body of stage 1 of the parameter gradients of nk_norm.hip, included INSIDE the signatures of
// layer_norm_param_partial_kernel<VEC> and rms_norm_gamma_partial_kernel<VEC> (no kernel of its own, no include guard; the includer
// defines and undefines NORM_CENTRED).  Block (tile, split) owns the 64 * VEC columns of its tile and the rows
// [split * rpb, (split + 1) * rpb): wave w takes rows w, w + 4, ... of them, a lane VEC adjacent columns (a wave reads 1 KB of a row
// at VEC = 4), the loads of PARAM_U rows in flight.  The four waves' sums are added in wave order and stored as
// part[split][0 = dgamma, 1 = dbeta][D] when centred, as part[split][D] (dgamma alone: there is no beta) when not.
    constexpr int NP = NORM_CENTRED ? 2 : 1;  // planes of sums: dgamma and, centred only, dbeta
    __shared__ float sm[4][NP][64 * VEC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * VEC;
    const bool on = col < D;  // VEC = 4 only with D % 4 == 0: a quad is inside the row or outside it
    const int cc = on ? col : 0;
    const long long r0 = blockIdx.y * rpb, r1 = r0 + rpb < rows ? r0 + rpb : rows;
    float dg[VEC];
#if NORM_CENTRED
    float db[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) dg[k] = db[k] = 0.f;
#else
#pragma unroll
    for (int k = 0; k < VEC; ++k) dg[k] = 0.f;
#endif
    struct Ld { float g[VEC], x[VEC]; };
    auto load = [&](long long r) {
        Ld l;
        if constexpr (VEC == 4) {
            const float4 a = nk_load_stream(reinterpret_cast<const float4*>(g + r * D + cc), nt);
            const float4 b = nk_load_stream(reinterpret_cast<const float4*>(x + r * D + cc), nt);
            l.g[0] = a.x; l.g[1] = a.y; l.g[2] = a.z; l.g[3] = a.w;
            l.x[0] = b.x; l.x[1] = b.y; l.x[2] = b.z; l.x[3] = b.w;
        } else {
            l.g[0] = g[r * D + cc];
            l.x[0] = x[r * D + cc];
        }
        return l;
    };
#if NORM_CENTRED
#define NORM_STATS(a, i) a[(i) * 2], a[(i) * 2 + 1]  // mean, rstd
    auto add = [&](const Ld& l, float mean, float rstd) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            dg[k] += l.g[k] * ((l.x[k] - mean) * rstd);
            db[k] += l.g[k];
        }
    };
#else
#define NORM_STATS(a, i) a[i]  // rstd
    auto add = [&](const Ld& l, float rstd) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) dg[k] += l.g[k] * (l.x[k] * rstd);
    };
#endif
    long long r = r0 + w;
    for (; r + 4 * (PARAM_U - 1) < r1; r += 4 * PARAM_U) {
        Ld l[PARAM_U];
        float st[PARAM_U * NP];
#pragma unroll
        for (int u = 0; u < PARAM_U; ++u) {
            l[u] = load(r + 4 * u);
            for (int p = 0; p < NP; ++p) st[u * NP + p] = stats[(r + 4 * u) * NP + p];
        }
#pragma unroll
        for (int u = 0; u < PARAM_U; ++u) add(l[u], NORM_STATS(st, u));
    }
    for (; r < r1; r += 4) add(load(r), NORM_STATS(stats, r));
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        sm[w][0][lane * VEC + k] = dg[k];
#if NORM_CENTRED
        sm[w][1][lane * VEC + k] = db[k];
#endif
    }
    __syncthreads();
    // NP * 64 * VEC sums for 256 threads
    for (int i = threadIdx.x; i < NP * 64 * VEC; i += 256) {
        const int which = i / (64 * VEC), j = i % (64 * VEC), c = blockIdx.x * 64 * VEC + j;
        if (c < D) part[((size_t)blockIdx.y * NP + which) * D + c] = (sm[0][which][j] + sm[1][which][j]) + (sm[2][which][j] + sm[3][which][j]);
    }
#undef NORM_STATS
