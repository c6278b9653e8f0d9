// Group normalisation (instance normalisation at G == C) of a contiguous row-major tensor read as (N, C, L): the kernels and entry
// points of nk_group_norm_*.  Included ONCE, by nk_norm.hip, behind that unit's helpers (al16, quads_load, row_stats, owner_sum,
// sum4 .. dot4, row_grid, the layer_norm_param_final_kernel), which it builds on.  Semantics: include/neuronika_hip.h.
// Group row r = n * G + j is the D = Cg * L contiguous floats at x + r * D; its element at offset o belongs to channel
// j * Cg + o / L.  Three classes, chosen from (Cg, L, 16-byte alignment) ALONE, so that a row's bits do not depend on N, G or the device:
//   registers  D % 4 == 0, D <= 16384, aligned: the LayerNorm family's shape (a wave per row up to 2048, a 256-thread block beyond),
//              statistics by the unit's row_stats, so at G == 1 `stats` is nk_layer_norm_fwd's bit for bit
//   chunked    D % 4 == 0, D > 16384, aligned: the row is cut into chunks of GN_CHUNK floats, grid = rows x chunks, two launches per
//              direction.  Launch 1 leaves per chunk (count, mean, M2) - or (sum gh, sum gh * xhat) - in the workspace; in launch 2
//              every block re-merges its row's few records in chunk order (Chan's formula) and finishes its own chunk.  No block
//              waits on another, and one sample at G == 1 still fills the machine.  x (and g) are read twice.
//   generic    everything else: a block per row, scalar strided passes, the same chunk-and-merge statistics (chunks of 2048)
// Chunk means are taken relative to an anchor, the row's first value, for the reason given in nk_batchnorm.hip.
// No division in any inner loop: a (channel, offset in plane) pair is formed once per thread and stepped by a fixed stride.
// dgamma / dbeta: stage 1 sums g and g * xhat over each (n, c) plane (a wave or a block per plane) into [N][2][C] of the workspace,
// stage 2 is the unit's layer_norm_param_final_kernel with the samples as its splits.  No atomics anywhere.
// Plain loads and stores throughout: the launch-time streaming switch of the LayerNorm family is not wired in here.

namespace {

constexpr int GN_CHUNK_V = 8;                   // quads per thread of a chunk: 32 data VGPRs forward, 96 in dx with accumulation
constexpr int GN_CHUNK = 256 * GN_CHUNK_V * 4;  // 8192 floats: a constant of the library, the same on every device
constexpr int GN_GEN_V = 8;                     // generic class: scalars per thread of a chunk
constexpr int GN_GEN_CHUNK = 256 * GN_GEN_V;    // 2048 floats
constexpr int GN_PLANE_BLOCK_L = 2048;          // parameter gradients: planes longer than this take a block, shorter ones a wave

struct GnTriple { float n, mean, m2; };
// Chan et al.: the triple of the union of two disjoint sets
__device__ __forceinline__ GnTriple gn_chan(const GnTriple& a, const GnTriple& b) {
    if (b.n == 0.f) return a;
    if (a.n == 0.f) return b;
    const float n = a.n + b.n, d = b.mean - a.mean, f = b.n / n;
    return GnTriple{n, a.mean + d * f, a.m2 + b.m2 + d * d * a.n * f};
}

// Where an offset of a group row lies: channel (relative to the group's first) and offset in that channel's plane.  Formed by one
// division per thread, then stepped: by a fixed stride (gn_advance, the stride given as quotient and remainder by L) or by one.
struct GnPos { unsigned ch, rem; };
__device__ __forceinline__ GnPos gn_pos(unsigned o, unsigned L) { const unsigned ch = o / L; return GnPos{ch, o - ch * L}; }
__device__ __forceinline__ void gn_advance(GnPos& p, unsigned dq, unsigned dr, unsigned L) {
    p.ch += dq;
    p.rem += dr;
    if (p.rem >= L) { p.rem -= L; ++p.ch; }
}
// the per-channel parameter of the four elements from position q on; LQ: L % 4 == 0, a quad lies in one plane
template <bool LQ>
__device__ __forceinline__ float4 gn_quad(const float* __restrict__ p, GnPos q, unsigned L) {
    if (LQ) { const float w = p[q.ch]; return make_float4(w, w, w, w); }
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r[k] = p[q.ch];
        if (++q.rem == L) { q.rem = 0; ++q.ch; }
    }
    return make_float4(r[0], r[1], r[2], r[3]);
}
__device__ __forceinline__ float4 mul4(const float4& a, const float4& b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 scale4(const float4& a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }

// y of V quads that hold the CENTRED values; `p` is the position of the thread's first quad, stepped T quads at a time
template <int V, int T, bool LQ>
__device__ __forceinline__ void gn_store_y(const float4 (&v)[V], float* __restrict__ yr, const float* __restrict__ gm,
                                           const float* __restrict__ bt, int t, int len, float rstd, GnPos p, unsigned L) {
    const unsigned dq = (T * 4u) / L, dr = (T * 4u) % L;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = (i * T + t) * 4;
        if (c < len) {
            float4 o = scale4(v[i], rstd);
            if (gm) o = mul4(o, gn_quad<LQ>(gm, p, L));
            if (bt) o = add4(o, gn_quad<LQ>(bt, p, L));
            *reinterpret_cast<float4*>(yr + c) = o;
        }
        gn_advance(p, dq, dr, L);
    }
}

// gh = g * gamma and xhat in place, and the thread's share of sum(gh) and sum(gh * xhat)
template <int V, int T, bool LQ>
__device__ __forceinline__ void gn_dx_terms(float4 (&gv)[V], float4 (&xv)[V], const float* __restrict__ gm, int t, int len, float mean,
                                            float rstd, GnPos p, unsigned L, float* s1, float* s2) {
    const unsigned dq = (T * 4u) / L, dr = (T * 4u) % L;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        if ((i * T + t) * 4 < len) {
            if (gm) gv[i] = mul4(gv[i], gn_quad<LQ>(gm, p, L));
            xv[i] = scale4(sub4(xv[i], mean), rstd);
            a += sum4(gv[i]);
            b += dot4(gv[i], xv[i]);
        }
        gn_advance(p, dq, dr, L);
    }
    *s1 = a;
    *s2 = b;
}

template <int V, int T>
__device__ __forceinline__ void gn_store_dx(const float4 (&gv)[V], const float4 (&xv)[V], const float4 (&dv)[V], float* __restrict__ dr_,
                                            int t, int len, float rstd, float c1, float c2, bool assign) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = (i * T + t) * 4;
        if (c < len) {
            float4 d = make_float4(rstd * (gv[i].x - c1 - xv[i].x * c2), rstd * (gv[i].y - c1 - xv[i].y * c2),
                                   rstd * (gv[i].z - c1 - xv[i].z * c2), rstd * (gv[i].w - c1 - xv[i].w * c2));
            if (!assign) d = add4(d, dv[i]);
            *reinterpret_cast<float4*>(dr_ + c) = d;
        }
    }
}

// ---- the row in registers -----------------------------------------------------------------------------------------------------------
// BLOCK = false: blocks of four waves, a wave per row.  BLOCK = true: a 256-thread block per row.  (rows, D) as in the LayerNorm kernels.
// LQ: L % 4 == 0, one parameter per quad; a template argument because the four gathers per quad of the other form, as a runtime
// branch, cost every kernel 30 - 90 VGPRs.
template <int V, bool BLOCK, bool LQ>
__global__ __launch_bounds__(256) void group_norm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ y,
                                                             float* __restrict__ stats, long long rows, int D, unsigned G, unsigned Cg,
                                                             unsigned L, float eps) {
    constexpr int T = BLOCK ? 256 : 64;
    __shared__ float red[4];
    const int t = BLOCK ? threadIdx.x : threadIdx.x & 63;
    const long long first = BLOCK ? blockIdx.x : blockIdx.x * 4ll + (threadIdx.x >> 6), step = BLOCK ? gridDim.x : gridDim.x * 4ll;
    const GnPos p0 = gn_pos(t * 4u, L);
    for (long long row = first; row < rows; row += step) {
        float4 v[V];
        quads_load<V, T>(v, x + row * D, t, D, false);
        float mean, rstd;
        row_stats<V, T>(v, t, D, eps, red, &mean, &rstd);
        if (stats && t == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
        const unsigned cb = ((unsigned)row % G) * Cg;
        gn_store_y<V, T, LQ>(v, y + row * D, gamma ? gamma + cb : nullptr, beta ? beta + cb : nullptr, t, D, rstd, p0, L);
    }
}

template <int V, bool BLOCK, bool LQ>
__global__ __launch_bounds__(256) void group_norm_bwd_kernel(int assign, float* __restrict__ dx, const float* __restrict__ g,
                                                             const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ stats, long long rows, int D, unsigned G,
                                                             unsigned Cg, unsigned L) {
    constexpr int T = BLOCK ? 256 : 64;
    __shared__ float red[4];
    const int t = BLOCK ? threadIdx.x : threadIdx.x & 63;
    const long long first = BLOCK ? blockIdx.x : blockIdx.x * 4ll + (threadIdx.x >> 6), step = BLOCK ? gridDim.x : gridDim.x * 4ll;
    const GnPos p0 = gn_pos(t * 4u, L);
    for (long long row = first; row < rows; row += step) {
        float4 gv[V], xv[V], dv[V];
        quads_load<V, T>(gv, g + row * D, t, D, false);
        quads_load<V, T>(xv, x + row * D, t, D, false);
        if (!assign) quads_load<V, T>(dv, dx + row * D, t, D, false);
        const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
        const unsigned cb = ((unsigned)row % G) * Cg;
        float s1, s2;
        gn_dx_terms<V, T, LQ>(gv, xv, gamma ? gamma + cb : nullptr, t, D, mean, rstd, p0, L, &s1, &s2);
        const float c1 = owner_sum<BLOCK>(s1, red) / (float)D;
        const float c2 = owner_sum<BLOCK>(s2, red) / (float)D;
        gn_store_dx<V, T>(gv, xv, dv, dx + row * D, t, D, rstd, c1, c2, assign);
    }
}

// ---- chunked ------------------------------------------------------------------------------------------------------------------------
// Work item w = row * chunks + k: chunk k of the row, the floats [k * GN_CHUNK, k * GN_CHUNK + len) of it.
struct GnChunk { long long row; int base, len; };
__device__ __forceinline__ GnChunk gn_chunk(long long w, int chunks, int D) {
    const long long row = w / chunks;
    const int base = (int)(w - row * chunks) * GN_CHUNK;
    return GnChunk{row, base, D - base < GN_CHUNK ? D - base : GN_CHUNK};
}

// part[w][3] = {count, mean - anchor, M2} of the chunk
__global__ __launch_bounds__(256) void group_norm_chunk_stats_kernel(const float* __restrict__ x, float* __restrict__ part, long long work,
                                                                     int chunks, int D) {
    constexpr int V = GN_CHUNK_V;
    __shared__ float red[4];
    const int t = threadIdx.x;
    for (long long w = blockIdx.x; w < work; w += gridDim.x) {
        const GnChunk ck = gn_chunk(w, chunks, D);
        const float* xr = x + ck.row * D;
        float4 v[V];
        quads_load<V, 256>(v, xr + ck.base, t, ck.len, false);
        const float anchor = xr[0];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i)
            if ((i * 256 + t) * 4 < ck.len) {
                v[i] = sub4(v[i], anchor);
                s += sum4(v[i]);
            }
        const float m = owner_sum<true>(s, red) / (float)ck.len;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i)
            if ((i * 256 + t) * 4 < ck.len) q += sq4(sub4(v[i], m));
        const float m2 = owner_sum<true>(q, red);
        if (t == 0) {
            float* p = part + w * 3;
            p[0] = (float)ck.len; p[1] = m; p[2] = m2;
        }
    }
}

// the row's records merged in chunk order, by every thread alike
__device__ __forceinline__ void gn_merge_row(const float* __restrict__ p, int chunks, float anchor, int D, float eps, float* mean,
                                             float* rstd) {
    GnTriple a{0.f, 0.f, 0.f};
    for (int k = 0; k < chunks; ++k) a = gn_chan(a, GnTriple{p[k * 3ll], p[k * 3ll + 1], p[k * 3ll + 2]});
    *mean = a.mean + anchor;
    *rstd = 1.f / sqrtf(a.m2 / (float)D + eps);
}

template <bool LQ>
__global__ __launch_bounds__(256) void group_norm_chunk_apply_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, float* __restrict__ y,
                                                                     float* __restrict__ stats, const float* __restrict__ part,
                                                                     long long work, int chunks, int D, unsigned G, unsigned Cg, unsigned L,
                                                                     float eps) {
    constexpr int V = GN_CHUNK_V;
    const int t = threadIdx.x;
    for (long long w = blockIdx.x; w < work; w += gridDim.x) {
        const GnChunk ck = gn_chunk(w, chunks, D);
        const float* xr = x + ck.row * D;
        float4 v[V];
        quads_load<V, 256>(v, xr + ck.base, t, ck.len, false);
        float mean, rstd;
        gn_merge_row(part + ck.row * chunks * 3, chunks, xr[0], D, eps, &mean, &rstd);
        if (stats && ck.base == 0 && t == 0) { stats[ck.row * 2] = mean; stats[ck.row * 2 + 1] = rstd; }
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = sub4(v[i], mean);
        const unsigned cb = ((unsigned)ck.row % G) * Cg;
        gn_store_y<V, 256, LQ>(v, y + ck.row * D + ck.base, gamma ? gamma + cb : nullptr, beta ? beta + cb : nullptr, t, ck.len, rstd,
                           gn_pos((unsigned)ck.base + t * 4u, L), L);
    }
}

// part[w][2] = {sum gh, sum gh * xhat} of the chunk
template <bool LQ>
__global__ __launch_bounds__(256) void group_norm_chunk_bwd_sums_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                        const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                        float* __restrict__ part, long long work, int chunks, int D,
                                                                        unsigned G, unsigned Cg, unsigned L) {
    constexpr int V = GN_CHUNK_V;
    __shared__ float red[4];
    const int t = threadIdx.x;
    for (long long w = blockIdx.x; w < work; w += gridDim.x) {
        const GnChunk ck = gn_chunk(w, chunks, D);
        float4 gv[V], xv[V];
        quads_load<V, 256>(gv, g + ck.row * D + ck.base, t, ck.len, false);
        quads_load<V, 256>(xv, x + ck.row * D + ck.base, t, ck.len, false);
        const unsigned cb = ((unsigned)ck.row % G) * Cg;
        float s1, s2;
        gn_dx_terms<V, 256, LQ>(gv, xv, gamma ? gamma + cb : nullptr, t, ck.len, stats[ck.row * 2], stats[ck.row * 2 + 1],
                            gn_pos((unsigned)ck.base + t * 4u, L), L, &s1, &s2);
        s1 = owner_sum<true>(s1, red);
        s2 = owner_sum<true>(s2, red);
        if (t == 0) { part[w * 2] = s1; part[w * 2 + 1] = s2; }
    }
}

template <bool LQ>
__global__ __launch_bounds__(256) void group_norm_chunk_bwd_kernel(int assign, float* __restrict__ dx, const float* __restrict__ g,
                                                                   const float* __restrict__ x, const float* __restrict__ gamma,
                                                                   const float* __restrict__ stats, const float* __restrict__ part,
                                                                   long long work, int chunks, int D, unsigned G, unsigned Cg, unsigned L) {
    constexpr int V = GN_CHUNK_V;
    const int t = threadIdx.x;
    for (long long w = blockIdx.x; w < work; w += gridDim.x) {
        const GnChunk ck = gn_chunk(w, chunks, D);
        float4 gv[V], xv[V], dv[V];
        quads_load<V, 256>(gv, g + ck.row * D + ck.base, t, ck.len, false);
        quads_load<V, 256>(xv, x + ck.row * D + ck.base, t, ck.len, false);
        if (!assign) quads_load<V, 256>(dv, dx + ck.row * D + ck.base, t, ck.len, false);
        const float* p = part + ck.row * chunks * 2;
        float s1 = 0.f, s2 = 0.f;
        for (int k = 0; k < chunks; ++k) { s1 += p[k * 2ll]; s2 += p[k * 2ll + 1]; }
        const float rstd = stats[ck.row * 2 + 1];
        const unsigned cb = ((unsigned)ck.row % G) * Cg;
        float u1, u2;  // the chunk's own sums again: not needed, the terms are
        gn_dx_terms<V, 256, LQ>(gv, xv, gamma ? gamma + cb : nullptr, t, ck.len, stats[ck.row * 2], rstd, gn_pos((unsigned)ck.base + t * 4u, L), L,
                            &u1, &u2);
        gn_store_dx<V, 256>(gv, xv, dv, dx + ck.row * D + ck.base, t, ck.len, rstd, s1 / (float)D, s2 / (float)D, assign);
    }
}

// ---- generic ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void group_norm_fwd_generic_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, float* __restrict__ y,
                                                                     float* __restrict__ stats, long long rows, int D, unsigned G,
                                                                     unsigned Cg, unsigned L, float eps) {
    constexpr int V = GN_GEN_V;
    __shared__ float red[4];
    const int t = threadIdx.x;
    const GnPos p0 = gn_pos(t, L);
    const unsigned dq = 256u / L, dr = 256u % L;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* xr = x + row * D;
        float* yr = y + row * D;
        const float anchor = xr[0];
        GnTriple acc{0.f, 0.f, 0.f};
        for (long long base = 0; base < D; base += GN_GEN_CHUNK) {
            const int len = D - base < GN_GEN_CHUNK ? (int)(D - base) : GN_GEN_CHUNK;
            float v[V], s = 0.f;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int c = i * 256 + t;
                v[i] = c < len ? xr[base + c] - anchor : 0.f;
                if (c < len) s += v[i];
            }
            const float m = owner_sum<true>(s, red) / (float)len;
            float q = 0.f;
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (i * 256 + t < len) { const float d = v[i] - m; q += d * d; }
            acc = gn_chan(acc, GnTriple{(float)len, m, owner_sum<true>(q, red)});
        }
        const float mean = acc.mean + anchor, rstd = 1.f / sqrtf(acc.m2 / (float)D + eps);
        if (stats && t == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
        const unsigned cb = ((unsigned)row % G) * Cg;
        const float* gm = gamma ? gamma + cb : nullptr;
        const float* bt = beta ? beta + cb : nullptr;
        GnPos p = p0;
        for (long long c = t; c < D; c += 256) {
            float o = (xr[c] - mean) * rstd;
            if (gm) o *= gm[p.ch];
            if (bt) o += bt[p.ch];
            yr[c] = o;
            gn_advance(p, dq, dr, L);
        }
    }
}

__global__ __launch_bounds__(256) void group_norm_bwd_generic_kernel(int assign, float* __restrict__ dx, const float* __restrict__ g,
                                                                     const float* __restrict__ x, const float* __restrict__ gamma,
                                                                     const float* __restrict__ stats, long long rows, int D, unsigned G,
                                                                     unsigned Cg, unsigned L) {
    __shared__ float red[4];
    const int t = threadIdx.x;
    const GnPos p0 = gn_pos(t, L);
    const unsigned dq = 256u / L, dr = 256u % L;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* gr = g + row * D;
        const float* xr = x + row * D;
        float* dr_ = dx + row * D;
        const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
        const unsigned cb = ((unsigned)row % G) * Cg;
        const float* gm = gamma ? gamma + cb : nullptr;
        float s1 = 0.f, s2 = 0.f;
        GnPos p = p0;
        for (long long c = t; c < D; c += 256) {
            const float gh = gm ? gr[c] * gm[p.ch] : gr[c], xh = (xr[c] - mean) * rstd;
            s1 += gh;
            s2 += gh * xh;
            gn_advance(p, dq, dr, L);
        }
        const float c1 = owner_sum<true>(s1, red) / (float)D;
        const float c2 = owner_sum<true>(s2, red) / (float)D;
        p = p0;
        for (long long c = t; c < D; c += 256) {
            const float gh = gm ? gr[c] * gm[p.ch] : gr[c], xh = (xr[c] - mean) * rstd;
            const float d = rstd * (gh - c1 - xh * c2);
            dr_[c] = assign ? d : dr_[c] + d;
            gn_advance(p, dq, dr, L);
        }
    }
}

// ---- parameter gradients, stage 1 ---------------------------------------------------------------------------------------------------
// Plane p = n * C + c, the L contiguous values of channel c of sample n: part[n][0][c] = sum g * xhat, part[n][1][c] = sum g - the
// layout layer_norm_param_final_kernel sums over its splits.  BLOCK = false: a wave per plane, four planes a block.
template <int VEC, bool BLOCK>
__global__ __launch_bounds__(256) void group_norm_param_plane_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                     const float* __restrict__ stats, float* __restrict__ part,
                                                                     long long planes, unsigned C, unsigned Cg, unsigned L) {
    constexpr unsigned T = BLOCK ? 256 : 64;
    __shared__ float red[4];
    const unsigned t = BLOCK ? threadIdx.x : threadIdx.x & 63;
    const long long first = BLOCK ? blockIdx.x : blockIdx.x * 4ll + (threadIdx.x >> 6), step = BLOCK ? gridDim.x : gridDim.x * 4ll;
    const unsigned G = C / Cg;
    for (long long p = first; p < planes; p += step) {
        const long long n = p / C;
        const unsigned c = (unsigned)(p - n * C);
        const long long r = n * G + c / Cg;
        const float mean = stats[r * 2], rstd = stats[r * 2 + 1];
        const float* gp = g + p * L;
        const float* xp = x + p * L;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll 4
        for (unsigned i = t * VEC; i < L; i += T * VEC) {
            if constexpr (VEC == 4) {
                const float4 gv = *reinterpret_cast<const float4*>(gp + i);
                const float4 xh = scale4(sub4(*reinterpret_cast<const float4*>(xp + i), mean), rstd);
                s0 += sum4(gv);
                s1 += dot4(gv, xh);
            } else {
                const float gv = gp[i];
                s0 += gv;
                s1 += gv * ((xp[i] - mean) * rstd);
            }
        }
        s0 = owner_sum<BLOCK>(s0, red);
        s1 = owner_sum<BLOCK>(s1, red);
        if (t == 0) {
            part[(n * 2) * C + c] = s1;
            part[(n * 2 + 1) * C + c] = s0;
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
struct GnGeom { long long rows; int D, Cg, chunks; };
enum GnClass { GN_REGISTERS, GN_CHUNKED, GN_GENERIC };

// The refusals every entry point shares; `go` is false where there is nothing to do (N == 0 or L == 0)
int gn_geometry(const char* who, long long N, int C, long long L, int G, GnGeom* out, bool* go) {
    NK_CHECK(G > 0 && C > 0 && C % G == 0, "%s: C = %d channels in G = %d groups (both must be positive, C a multiple of G)", who, C, G);
    NK_CHECK(N >= 0 && L >= 0, "%s: N = %lld, L = %lld", who, N, L);
    const long long Cg = C / G;
    NK_CHECK(L <= 0x7fffffffll / Cg, "%s: a group row of %lld x %lld elements does not fit in 31 bits", who, Cg, L);
    NK_CHECK(N <= 0x7fffffffll / G, "%s: N * G = %lld x %d does not fit in 31 bits", who, N, G);
    out->rows = N * G;
    out->D = (int)(Cg * L);
    out->Cg = (int)Cg;
    out->chunks = (out->D + GN_CHUNK - 1) / GN_CHUNK;
    *go = N > 0 && L > 0;
    return NK_OK;
}

// (Cg, L, alignment) alone
GnClass gn_class(int D, std::initializer_list<const void*> operands) {
    bool vec = D % 4 == 0;
    for (const void* p : operands) vec = vec && al16(p);
    return !vec ? GN_GENERIC : D <= BLOCK_MAX_D ? GN_REGISTERS : GN_CHUNKED;
}

unsigned gn_chunk_grid(long long work) { return (unsigned)(work < (long long)MAX_GRID ? work : (long long)MAX_GRID); }

// the LayerNorm ladder's thresholds: the same (V, owner) for the same D, which is what makes `stats` agree bit for bit at G == 1
// KERNEL... is a kernel's name with its leading template arguments; the last one, LQ, is chosen here from L
#define NK_GN_LAUNCH(GRID, ARGS, ...)                                                                                          \
    do {                                                                                                                       \
        if (L % 4 == 0) hipLaunchKernelGGL((__VA_ARGS__ true>), dim3(GRID), dim3(256), 0, dev->compute, NK_GN_UNPACK ARGS);    \
        else hipLaunchKernelGGL((__VA_ARGS__ false>), dim3(GRID), dim3(256), 0, dev->compute, NK_GN_UNPACK ARGS);              \
    } while (0)
#define NK_GN_UNPACK(...) __VA_ARGS__
#define NK_GN_ROWS(KERNEL, V, BLOCK, ...) NK_GN_LAUNCH(row_grid(rows, BLOCK ? 1 : 4), (__VA_ARGS__), KERNEL<V, BLOCK,)
#define NK_GN_LADDER(KERNEL, ...)                                             \
    do {                                                                      \
        if (D <= 256) NK_GN_ROWS(KERNEL, 1, false, __VA_ARGS__);              \
        else if (D <= 512) NK_GN_ROWS(KERNEL, 2, false, __VA_ARGS__);         \
        else if (D <= 1024) NK_GN_ROWS(KERNEL, 4, false, __VA_ARGS__);        \
        else if (D <= WAVE_MAX_D) NK_GN_ROWS(KERNEL, 8, false, __VA_ARGS__);  \
        else if (D <= 4096) NK_GN_ROWS(KERNEL, 4, true, __VA_ARGS__);         \
        else if (D <= 8192) NK_GN_ROWS(KERNEL, 8, true, __VA_ARGS__);         \
        else NK_GN_ROWS(KERNEL, 16, true, __VA_ARGS__);                       \
    } while (0)

int group_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, long long N, int C,
                   long long L_, int G, int assign) {
    NK_USE(dev);
    const char* who = assign ? "nk_group_norm_bwd_assign" : "nk_group_norm_bwd";
    GnGeom gm;
    bool go;
    if (int rc = gn_geometry(who, N, C, L_, G, &gm, &go)) return rc;
    NK_CHECK(dx && g && x && stats, "null pointer in %s (only gamma may be NULL)", who);
    if (!go) return NK_OK;
    const long long rows = gm.rows;
    const int D = gm.D;
    const unsigned uG = (unsigned)G, Cg = (unsigned)gm.Cg, L = (unsigned)L_;
    switch (gn_class(D, {dx, g, x, gamma})) {
    case GN_REGISTERS:
        NK_GN_LADDER(group_norm_bwd_kernel, assign, dx, g, x, gamma, stats, rows, D, uG, Cg, L);
        break;
    case GN_CHUNKED: {
        const long long work = rows * gm.chunks;
        void* ws = nullptr;
        if (int rc = nk_workspace(dev, (size_t)work * 2 * sizeof(float), &ws)) return rc;
        NK_GN_LAUNCH(gn_chunk_grid(work), (g, x, gamma, stats, (float*)ws, work, gm.chunks, D, uG, Cg, L), group_norm_chunk_bwd_sums_kernel<);
        NK_LAUNCH_CHECK();
        NK_GN_LAUNCH(gn_chunk_grid(work), (assign, dx, g, x, gamma, stats, (const float*)ws, work, gm.chunks, D, uG, Cg, L), group_norm_chunk_bwd_kernel<);
        break;
    }
    case GN_GENERIC:
        hipLaunchKernelGGL(group_norm_bwd_generic_kernel, dim3(row_grid(rows, 1)), dim3(256), 0, dev->compute, assign, dx, g, x, gamma, stats, rows, D, uG, Cg, L);
        break;
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int group_norm_bwd_params(nk_device* dev, float* dgamma, float* dbeta, const float* g, const float* x, const float* stats, long long N,
                          int C, long long L_, int G, int assign) {
    NK_USE(dev);
    const char* who = assign ? "nk_group_norm_bwd_params_assign" : "nk_group_norm_bwd_params";
    GnGeom gm;
    bool go;
    if (int rc = gn_geometry(who, N, C, L_, G, &gm, &go)) return rc;
    NK_CHECK(dgamma || dbeta, "%s: dgamma and dbeta are both NULL", who);
    NK_CHECK(g && x && stats, "null pointer in %s", who);
    if (!go) return NK_OK;
    const long long planes = N * C;
    const unsigned uC = (unsigned)C, Cg = (unsigned)gm.Cg, L = (unsigned)L_;
    void* ws = nullptr;
    if (int rc = nk_workspace(dev, (size_t)planes * 2 * sizeof(float), &ws)) return rc;
    const bool vec = L % 4 == 0 && al16(g) && al16(x), block = L > (unsigned)GN_PLANE_BLOCK_L;
    const dim3 grid(row_grid(planes, block ? 1 : 4));
#define NK_GN_PLANES(VEC, BLOCK) \
    hipLaunchKernelGGL((group_norm_param_plane_kernel<VEC, BLOCK>), grid, dim3(256), 0, dev->compute, g, x, stats, (float*)ws, planes, uC, Cg, L)
    if (vec && block) NK_GN_PLANES(4, true);
    else if (vec) NK_GN_PLANES(4, false);
    else if (block) NK_GN_PLANES(1, true);
    else NK_GN_PLANES(1, false);
#undef NK_GN_PLANES
    NK_LAUNCH_CHECK();
    // stage 2: the samples are the splits; the four waves of a block take a quarter of them each, ascending
    hipLaunchKernelGGL(layer_norm_param_final_kernel, dim3((C + 63) / 64, 2), dim3(256), 0, dev->compute, (const float*)ws, dgamma, dbeta, C, (int)N, assign);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_group_norm_fwd(nk_device* dev, const float* x, const float* gamma, const float* beta, float* y, float* stats, long long N, int C,
                      long long L_, int G, double eps) {
    NK_USE(dev);
    GnGeom gm;
    bool go;
    if (int rc = gn_geometry("nk_group_norm_fwd", N, C, L_, G, &gm, &go)) return rc;
    NK_CHECK(eps >= 0.0 && eps <= 3.0e38, "nk_group_norm_fwd: eps = %g (must be finite and not negative)", eps);  // NaN fails both
    NK_CHECK(x && y, "null pointer in nk_group_norm_fwd (gamma, beta and stats may be NULL)");
    if (!go) return NK_OK;
    const long long rows = gm.rows;
    const int D = gm.D;
    const unsigned uG = (unsigned)G, Cg = (unsigned)gm.Cg, L = (unsigned)L_;
    switch (gn_class(D, {x, y, gamma, beta})) {
    case GN_REGISTERS:
        NK_GN_LADDER(group_norm_fwd_kernel, x, gamma, beta, y, stats, rows, D, uG, Cg, L, (float)eps);
        break;
    case GN_CHUNKED: {
        const long long work = rows * gm.chunks;
        void* ws = nullptr;
        if (int rc = nk_workspace(dev, (size_t)work * 3 * sizeof(float), &ws)) return rc;
        hipLaunchKernelGGL(group_norm_chunk_stats_kernel, dim3(gn_chunk_grid(work)), dim3(256), 0, dev->compute, x, (float*)ws, work, gm.chunks, D);
        NK_LAUNCH_CHECK();
        NK_GN_LAUNCH(gn_chunk_grid(work), (x, gamma, beta, y, stats, (const float*)ws, work, gm.chunks, D, uG, Cg, L, (float)eps), group_norm_chunk_apply_kernel<);
        break;
    }
    case GN_GENERIC:
        hipLaunchKernelGGL(group_norm_fwd_generic_kernel, dim3(row_grid(rows, 1)), dim3(256), 0, dev->compute, x, gamma, beta, y, stats, rows, D, uG, Cg, L, (float)eps);
        break;
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int nk_group_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, long long N, int C,
                      long long L, int G) {
    return group_norm_bwd(dev, dx, g, x, gamma, stats, N, C, L, G, 0);
}
int nk_group_norm_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, long long N,
                             int C, long long L, int G) {
    return group_norm_bwd(dev, dx, g, x, gamma, stats, N, C, L, G, 1);
}
int nk_group_norm_bwd_params(nk_device* dev, float* dgamma, float* dbeta, const float* g, const float* x, const float* stats, long long N,
                             int C, long long L, int G) {
    return group_norm_bwd_params(dev, dgamma, dbeta, g, x, stats, N, C, L, G, 0);
}
int nk_group_norm_bwd_params_assign(nk_device* dev, float* dgamma, float* dbeta, const float* g, const float* x, const float* stats,
                                    long long N, int C, long long L, int G) {
    return group_norm_bwd_params(dev, dgamma, dbeta, g, x, stats, N, C, L, G, 1);
}

}  // extern "C"
