// Batch normalisation of a contiguous row-major tensor read as (N, C, L): per channel c the statistic runs over the M = N * L
// values x[n][c][l] - a strided set far too large for registers.  The reference has no such layer; the semantics are fixed in
// include/neuronika_hip.h (mean, then the CENTRED sum of squares; chunks merged with Chan's formula; all in f32).
//   statistics   a wave holds one chunk of a channel in registers (the LayerNorm idiom: mean, then the centred squares of the same
//                registers), merges the chunk's (count, mean, M2) into its running triple, the four waves of a block merge in wave
//                order and leave one partial triple in the workspace; a second kernel merges the partials of a channel (four waves a
//                quarter each in ascending order, then the four in wave order) and writes {mean, rstd} and the running statistics.
//   backward     s0 = sum g, s1 = sum g * xhat per channel through the same partial / final pair (plain sums); dx is elementwise
//                in the channel's scalars.
// Three layout classes, chosen at launch from (N, C, L) and the pointers' alignment:
//   planes   L % 4 == 0, L >= 256, 16-byte aligned: float4 traffic, channel scalars block-uniform
//   columns  L == 1 (an (N, C) matrix): a lane owns adjacent columns and walks the rows, the tiling of layer_norm_bwd_params
//   generic  everything else: scalar loads, flat indices, correct for every shape
// No atomics, no block waits on another block: every order of summation is a function of (N, C, L) alone.
#include "nk_common.h"

#include <climits>

namespace {

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

constexpr unsigned MAX_GRID = 1u << 20;  // blocks per launch of the elementwise kernels; they stride over the work beyond it
constexpr int PLANE_MIN_L = 256;         // a plane segment feeds a whole wave with one quad per lane (guessed, not measured)
constexpr int V = 4;                     // slots per lane of a wave's chunk: 4 quads (planes) or 4 scalars (generic)
constexpr int COL_U = 8;                 // rows a lane of the column kernels holds per trip

struct Triple { float n, mean, m2; };
// Chan et al.: the triple of the union of two disjoint sets
__device__ __forceinline__ Triple chan(const Triple& a, const Triple& b) {
    if (b.n == 0.f) return a;
    if (a.n == 0.f) return b;
    const float n = a.n + b.n, d = b.mean - a.mean, f = b.n / n;
    return Triple{n, a.mean + d * f, a.m2 + b.m2 + d * d * a.n * f};
}

// How a channel's M values are cut into the units a wave holds at once.  VEC = 4 (planes): plane n is cut into `cp` units of at
// most `qpu` <= 64 V quads, unit u = (n, k).  VEC = 1 (generic): unit u is the 64 V consecutive values from j = u * 64 V on of the
// channel's flattened (n, l) index.  Block `split` of a channel owns the units [split * upb, (split + 1) * upb), wave w every
// fourth of them from w on.
struct Units {
    int C, L, cp, qpu;
    long long M, units, upb;
};

// offsets (in floats) of the lane's V slots of unit u and whether each is inside the unit; returns the unit's element count
template <int VEC>
__device__ __forceinline__ int unit_slots(const Units& g, int c, long long u, int lane, size_t (&off)[V], bool (&on)[V]) {
    if (VEC == 4) {
        const long long n = u / g.cp;
        const int k = (int)(u - n * g.cp), Q = g.L >> 2, q0 = k * g.qpu;
        const int qn = Q - q0 < g.qpu ? Q - q0 : g.qpu;
        if (qn <= 0) return 0;
        const size_t base = ((size_t)n * g.C + c) * g.L + (size_t)q0 * 4;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int q = i * 64 + lane;
            on[i] = q < qn;
            off[i] = base + (size_t)(on[i] ? q : 0) * 4;
        }
        return qn * 4;
    } else {
        const long long j0 = u * (64 * V), j1 = j0 + 64 * V < g.M ? j0 + 64 * V : g.M;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const long long j = j0 + i * 64 + lane;
            on[i] = j < j1;
            const long long jj = on[i] ? j : j0, n = jj / g.L;
            off[i] = ((size_t)n * g.C + c) * g.L + (size_t)(jj - n * g.L);
        }
        return (int)(j1 - j0);
    }
}

template <int VEC>
__device__ __forceinline__ void slot_load(float (&v)[VEC], const float* __restrict__ p, size_t off, bool nt) {
    if constexpr (VEC == 4) {
        const float4 t = nk_load_stream(reinterpret_cast<const float4*>(p + off), nt);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[off];
    }
}

// ---- statistics -----------------------------------------------------------------------------------------------------------------
// part[(split * 3 + {0 count, 1 mean, 2 M2}) * C + c]
template <int VEC>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* __restrict__ x, float* __restrict__ part, Units g) {
    __shared__ Triple sm[4];
    const int c = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long lo = blockIdx.y * g.upb, hi = lo + g.upb < g.units ? lo + g.upb : g.units;
    // The wave's means are kept RELATIVE to an anchor, the first value the wave reads: next to a large common offset the f32 grid
    // is coarse against the spread, sums of such values round at the size of the sum, and a running mean that is moved by
    // delta * nb / n stops moving at all.  Differences of nearby values are exact, so Chan's formula runs on them unharmed.
    Triple acc{0.f, 0.f, 0.f};
    float anchor = 0.f;
    for (long long u = lo + w; u < hi; u += 4) {
        size_t off[V];
        bool on[V];
        const int cnt = unit_slots<VEC>(g, c, u, lane, off, on);
        if (cnt <= 0) continue;  // wave-uniform
        float v[V][VEC];
#pragma unroll
        for (int i = 0; i < V; ++i) slot_load<VEC>(v[i], x, off[i], false);
        if (acc.n == 0.f) anchor = __shfl(v[0][0], 0, 64);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i)
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                v[i][k] -= anchor;
                if (on[i]) s += v[i][k];
            }
        const float mean = nk_wave_sum(s) / (float)cnt;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (on[i]) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) { const float d = v[i][k] - mean; q += d * d; }
            }
        acc = chan(acc, Triple{(float)cnt, mean, nk_wave_sum(q)});
    }
    acc.mean += anchor;
    if (lane == 0) sm[w] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const Triple t = chan(chan(chan(sm[0], sm[1]), sm[2]), sm[3]);
        float* p = part + (size_t)blockIdx.y * 3 * g.C + c;
        p[0] = t.n; p[g.C] = t.mean; p[2 * (size_t)g.C] = t.m2;
    }
}

// Columns: block (tile, split) owns 64 VEC columns and the rows [split * rpb, (split + 1) * rpb); wave w takes rows w, w + 4, ... of
// them, COL_U rows per trip: a lane forms the triple of its COL_U values of each of its VEC columns and merges it.
template <int VEC>
__global__ __launch_bounds__(256) void bn_col_stats_partial_kernel(const float* __restrict__ x, float* __restrict__ part, int N, int C,
                                                                   int rpb) {
    __shared__ float sm[4][3][64 * VEC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * VEC;
    const int cc = col < C ? col : 0;  // VEC = 4 only with C % 4 == 0: a quad is inside the row or outside it
    const long long r0 = (long long)blockIdx.y * rpb, r1 = r0 + rpb < N ? r0 + rpb : N;
    float na = 0.f, mean[VEC], m2[VEC], anchor[VEC];  // means relative to the lane's first value of the column (see above)
#pragma unroll
    for (int k = 0; k < VEC; ++k) mean[k] = m2[k] = anchor[k] = 0.f;
    for (long long r = r0 + w; r < r1; r += 4 * COL_U) {
        float v[COL_U][VEC];
        int cnt = 0;
#pragma unroll
        for (int u = 0; u < COL_U; ++u) {
            const long long rr = r + 4 * u;
            const bool in = rr < r1;
            cnt += in;
            slot_load<VEC>(v[u], x, (size_t)(in ? rr : r) * C + cc, false);
        }
        const float nb = (float)cnt, n = na + nb, f = nb / n;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (na == 0.f) anchor[k] = v[0][k];
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int u = 0; u < COL_U; ++u) {
                v[u][k] -= anchor[k];
                if (r + 4 * u < r1) s += v[u][k];
            }
            const float mb = s / nb;
#pragma unroll
            for (int u = 0; u < COL_U; ++u)
                if (r + 4 * u < r1) { const float d = v[u][k] - mb; q += d * d; }
            const float d = mb - mean[k];
            if (na == 0.f) { mean[k] = mb; m2[k] = q; }
            else { mean[k] += d * f; m2[k] += q + d * d * na * f; }
        }
        na = n;
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) mean[k] += anchor[k];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        sm[w][0][lane * VEC + k] = na;
        sm[w][1][lane * VEC + k] = mean[k];
        sm[w][2][lane * VEC + k] = m2[k];
    }
    __syncthreads();
    const int j = threadIdx.x, c = blockIdx.x * 64 * VEC + j;
    if (j < 64 * VEC && c < C) {
        Triple t{sm[0][0][j], sm[0][1][j], sm[0][2][j]};
#pragma unroll
        for (int i = 1; i < 4; ++i) t = chan(t, Triple{sm[i][0][j], sm[i][1][j], sm[i][2][j]});
        float* p = part + (size_t)blockIdx.y * 3 * C + c;
        p[0] = t.n; p[C] = t.mean; p[2 * (size_t)C] = t.m2;
    }
}

// Block `tile` finishes 64 channels: wave w merges the partial triples [w * per, (w + 1) * per) of a lane's channel in ascending
// order (eight loads in flight), the four waves' triples merge in wave order, and the lane of wave 0 writes {mean, rstd} and updates
// the running statistics (unbias = M / (M - 1)).  Every mean is taken relative to the first partial's (see above).
constexpr int FINAL_U = 8;
__global__ __launch_bounds__(256) void bn_stats_final_kernel(const float* __restrict__ part, int splits, int C, float M, float eps,
                                                             float momentum, float unbias, float* __restrict__ stats,
                                                             float* __restrict__ running_mean, float* __restrict__ running_var) {
    __shared__ float sm[4][3][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    const int cc = c < C ? c : 0;
    const int per = (splits + 3) / 4, lo = w * per, hi = lo + per < splits ? lo + per : splits;
    const float anchor = part[(size_t)C + cc];
    Triple t{0.f, 0.f, 0.f};
    int s = lo;
    for (; s + FINAL_U <= hi; s += FINAL_U) {
        Triple b[FINAL_U];
#pragma unroll
        for (int u = 0; u < FINAL_U; ++u) {
            const float* p = part + (size_t)(s + u) * 3 * C + cc;
            b[u] = Triple{p[0], p[C] - anchor, p[2 * (size_t)C]};
        }
#pragma unroll
        for (int u = 0; u < FINAL_U; ++u) t = chan(t, b[u]);
    }
    for (; s < hi; ++s) {
        const float* p = part + (size_t)s * 3 * C + cc;
        t = chan(t, Triple{p[0], p[C] - anchor, p[2 * (size_t)C]});
    }
    sm[w][0][lane] = t.n; sm[w][1][lane] = t.mean; sm[w][2][lane] = t.m2;
    __syncthreads();
    if (w != 0 || c >= C) return;
#pragma unroll
    for (int i = 1; i < 4; ++i) t = chan(t, Triple{sm[i][0][lane], sm[i][1][lane], sm[i][2][lane]});
    t.mean += anchor;
    const float var = t.m2 / M;
    stats[2 * (size_t)c] = t.mean;
    stats[2 * (size_t)c + 1] = 1.f / sqrtf(var + eps);
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * t.mean;
    if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (var * unbias);
}

// inference: {mean, rstd} out of the running statistics
__global__ __launch_bounds__(256) void bn_infer_stats_kernel(const float* __restrict__ running_mean, const float* __restrict__ running_var,
                                                             float eps, int C, float* __restrict__ stats) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    stats[2 * (size_t)c] = running_mean[c];
    stats[2 * (size_t)c + 1] = 1.f / sqrtf(running_var[c] + eps);
}

// ---- backward sums --------------------------------------------------------------------------------------------------------------
// part[(split * 2 + {0: s0, 1: s1}) * C + c]
template <int VEC>
__global__ __launch_bounds__(256) void bn_sums_partial_kernel(const float* __restrict__ gr, const float* __restrict__ x,
                                                              const float* __restrict__ stats, float* __restrict__ part, Units g, bool nt) {
    __shared__ float sm[4][2];
    const int c = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float mean = stats[2 * (size_t)c], rstd = stats[2 * (size_t)c + 1];
    const long long lo = blockIdx.y * g.upb, hi = lo + g.upb < g.units ? lo + g.upb : g.units;
    float s0 = 0.f, s1 = 0.f;
    for (long long u = lo + w; u < hi; u += 4) {
        size_t off[V];
        bool on[V];
        if (unit_slots<VEC>(g, c, u, lane, off, on) <= 0) continue;
        float gv[V][VEC], xv[V][VEC];
#pragma unroll
        for (int i = 0; i < V; ++i) { slot_load<VEC>(gv[i], gr, off[i], nt); slot_load<VEC>(xv[i], x, off[i], nt); }
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (on[i]) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) { s0 += gv[i][k]; s1 += gv[i][k] * ((xv[i][k] - mean) * rstd); }
            }
    }
    s0 = nk_wave_sum(s0);
    s1 = nk_wave_sum(s1);
    if (lane == 0) { sm[w][0] = s0; sm[w][1] = s1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        part[((size_t)blockIdx.y * 2 + k) * g.C + c] = (sm[0][k] + sm[1][k]) + (sm[2][k] + sm[3][k]);
    }
}

template <int VEC>
__global__ __launch_bounds__(256) void bn_col_sums_partial_kernel(const float* __restrict__ gr, const float* __restrict__ x,
                                                                  const float* __restrict__ stats, float* __restrict__ part, int N, int C,
                                                                  int rpb, bool nt) {
    __shared__ float sm[4][2][64 * VEC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * VEC;
    const int cc = col < C ? col : 0;
    const long long r0 = (long long)blockIdx.y * rpb, r1 = r0 + rpb < N ? r0 + rpb : N;
    float mean[VEC], rstd[VEC], s0[VEC], s1[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        mean[k] = stats[2 * (size_t)(cc + k)];
        rstd[k] = stats[2 * (size_t)(cc + k) + 1];
        s0[k] = s1[k] = 0.f;
    }
    for (long long r = r0 + w; r < r1; r += 4 * COL_U) {
        float gv[COL_U][VEC], xv[COL_U][VEC];
#pragma unroll
        for (int u = 0; u < COL_U; ++u) {
            const size_t off = (size_t)(r + 4 * u < r1 ? r + 4 * u : r) * C + cc;
            slot_load<VEC>(gv[u], gr, off, nt);
            slot_load<VEC>(xv[u], x, off, nt);
        }
#pragma unroll
        for (int u = 0; u < COL_U; ++u)
            if (r + 4 * u < r1) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) { s0[k] += gv[u][k]; s1[k] += gv[u][k] * ((xv[u][k] - mean[k]) * rstd[k]); }
            }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) { sm[w][0][lane * VEC + k] = s0[k]; sm[w][1][lane * VEC + k] = s1[k]; }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * 64 * VEC; i += 256) {
        const int which = i / (64 * VEC), j = i % (64 * VEC), c = blockIdx.x * 64 * VEC + j;
        if (c < C) part[((size_t)blockIdx.y * 2 + which) * C + c] = (sm[0][which][j] + sm[1][which][j]) + (sm[2][which][j] + sm[3][which][j]);
    }
}

// the same shape for the plain sums: wave w adds its quarter of the splits in ascending order, the four waves in wave order
__global__ __launch_bounds__(256) void bn_sums_final_kernel(const float* __restrict__ part, int splits, int C, float* __restrict__ sums) {
    __shared__ float sm[4][2][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    const int cc = c < C ? c : 0;
    const int per = (splits + 3) / 4, lo = w * per, hi = lo + per < splits ? lo + per : splits;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 8
    for (int s = lo; s < hi; ++s) {
        s0 += part[(size_t)s * 2 * C + cc];
        s1 += part[((size_t)s * 2 + 1) * C + cc];
    }
    sm[w][0][lane] = s0; sm[w][1][lane] = s1;
    __syncthreads();
    if (w != 0 || c >= C) return;
    sums[2 * (size_t)c] = (sm[0][0][lane] + sm[1][0][lane]) + (sm[2][0][lane] + sm[3][0][lane]);
    sums[2 * (size_t)c + 1] = (sm[0][1][lane] + sm[1][1][lane]) + (sm[2][1][lane] + sm[3][1][lane]);
}

__global__ __launch_bounds__(256) void bn_params_kernel(const float* __restrict__ sums, float* __restrict__ dgamma,
                                                        float* __restrict__ dbeta, int C, int assign) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float s0 = sums[2 * (size_t)c], s1 = sums[2 * (size_t)c + 1];
    if (dgamma) dgamma[c] = assign ? s1 : dgamma[c] + s1;
    if (dbeta) dbeta[c] = assign ? s0 : dbeta[c] + s0;
}

// ---- elementwise: normalise, dx -------------------------------------------------------------------------------------------------
// An Op names its NIN input streams, its output, the scalars P of a channel and the value of one element.
struct NormOp {  // y = (x - mean) * rstd * gamma + beta
    static constexpr int NIN = 1;
    const float* in[1];
    float* out;
    const float *stats, *gamma, *beta;
    struct P { float mean, rstd, w, b; };
    __device__ __forceinline__ P params(int c) const {
        return P{stats[2 * (size_t)c], stats[2 * (size_t)c + 1], gamma ? gamma[c] : 1.f, beta ? beta[c] : 0.f};
    }
    __device__ __forceinline__ float f(const P& p, const float (&v)[1]) const { return (v[0] - p.mean) * p.rstd * p.w + p.b; }
};
// dx (+)= gamma * rstd * (g - s0 / M - xhat * s1 / M), or gamma * rstd * g in the inference form.  Streams: g, x unless INFER, dx
// unless ASSIGN.
template <bool ASSIGN, bool INFER>
struct DxOp {
    static constexpr int NIN = 1 + !INFER + !ASSIGN;
    const float* in[NIN];
    float* out;
    const float *stats, *gamma, *sums;
    float inv_m;
    struct P { float mean, rstd, gr, c0, c1; };
    __device__ __forceinline__ P params(int c) const {
        const float rstd = stats[2 * (size_t)c + 1];
        P p{stats[2 * (size_t)c], rstd, (gamma ? gamma[c] : 1.f) * rstd, 0.f, 0.f};
        if (!INFER) { p.c0 = sums[2 * (size_t)c] * inv_m; p.c1 = sums[2 * (size_t)c + 1] * inv_m; }
        return p;
    }
    __device__ __forceinline__ float f(const P& p, const float (&v)[NIN]) const {
        float d;
        if (INFER) d = p.gr * v[0];
        else d = p.gr * (v[0] - p.c0 - (v[1] - p.mean) * p.rstd * p.c1);
        return ASSIGN ? d : v[NIN - 1] + d;
    }
};

// Planes: an item is one segment of at most 1024 quads of one (n, c) plane; the channel's scalars are block-uniform, the loads of
// the four trips are issued before the first use, the stores stream.
template <class Op>
__global__ __launch_bounds__(256) void bn_plane_map_kernel(Op op, int C, int Q, int segs, long long items, bool nt) {
    constexpr int U = 4;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long plane = item / segs;
        const int seg = (int)(item - plane * segs), c = (int)(plane % C);
        const typename Op::P p = op.params(c);
        const size_t base = (size_t)plane * Q;
        const int q0 = seg * (256 * U), q1 = q0 + 256 * U < Q ? q0 + 256 * U : Q;
        float4 v[U][Op::NIN];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * 256 + threadIdx.x;
#pragma unroll
            for (int s = 0; s < Op::NIN; ++s) v[u][s] = nk_load_stream(reinterpret_cast<const float4*>(op.in[s]) + base + (q < q1 ? q : q0), nt);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int q = q0 + u * 256 + threadIdx.x;
            if (q < q1) {
                float a[Op::NIN], b[Op::NIN], cc[Op::NIN], d[Op::NIN];
#pragma unroll
                for (int s = 0; s < Op::NIN; ++s) { a[s] = v[u][s].x; b[s] = v[u][s].y; cc[s] = v[u][s].z; d[s] = v[u][s].w; }
                nk_store_stream(reinterpret_cast<float4*>(op.out) + base + q, make_float4(op.f(p, a), op.f(p, b), op.f(p, cc), op.f(p, d)));
            }
        }
    }
}

// Columns: the tiling of the column reductions; a lane keeps the scalars of its VEC columns and walks the rows.
template <class Op, int VEC>
__global__ __launch_bounds__(256) void bn_col_map_kernel(Op op, int N, int C, int rpb, bool nt) {
    constexpr int U = 4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * VEC;
    const bool on = col < C;
    const int cc = on ? col : 0;
    typename Op::P p[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) p[k] = op.params(cc + k);
    const long long r0 = (long long)blockIdx.y * rpb, r1 = r0 + rpb < N ? r0 + rpb : N;
    for (long long r = r0 + w; r < r1; r += 4 * U) {
        float v[U][Op::NIN][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t off = (size_t)(r + 4 * u < r1 ? r + 4 * u : r) * C + cc;
#pragma unroll
            for (int s = 0; s < Op::NIN; ++s) slot_load<VEC>(v[u][s], op.in[s], off, nt);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!on || r + 4 * u >= r1) continue;
            float o[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                float a[Op::NIN];
#pragma unroll
                for (int s = 0; s < Op::NIN; ++s) a[s] = v[u][s][k];
                o[k] = op.f(p[k], a);
            }
            float* dst = op.out + (size_t)(r + 4 * u) * C + col;
            if constexpr (VEC == 4) nk_store_stream(reinterpret_cast<float4*>(dst), make_float4(o[0], o[1], o[2], o[3]));
            else dst[0] = o[0];
        }
    }
}

// Generic: flat indices, scalar traffic, the channel's scalars read per element.
template <class Op>
__global__ __launch_bounds__(256) void bn_generic_map_kernel(Op op, int C, int L, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int c = (int)((i / (size_t)L) % (size_t)C);
        float a[Op::NIN];
#pragma unroll
        for (int s = 0; s < Op::NIN; ++s) a[s] = op.in[s][i];
        op.out[i] = op.f(op.params(c), a);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
enum Layout { PLANES, COLUMNS4, COLUMNS1, GENERIC };

Layout layout_of(int C, int L, bool aligned) {
    if (L == 1) return aligned && C % 4 == 0 ? COLUMNS4 : COLUMNS1;
    return aligned && L % 4 == 0 && L >= PLANE_MIN_L ? PLANES : GENERIC;
}

int check_geometry(const char* who, int N, int C, int L) {
    NK_CHECK(C > 0, "%s: C = %d (the channel count must be positive)", who, C);
    NK_CHECK(N >= 0 && L >= 0, "%s: N = %d, L = %d", who, N, L);
    NK_CHECK((long long)N * L <= INT_MAX, "%s: N * L = %lld values per channel (at most 2^31 - 1)", who, (long long)N * L);
    return NK_OK;
}

// the cut of a channel into units and of the units into blocks: about 2048 blocks in all, at least one unit per wave; a function of
// (N, C, L) and the layout alone
Units units_of(Layout lay, int N, int C, int L, int* splits) {
    Units g{};
    g.C = C; g.L = L; g.M = (long long)N * L;
    if (lay == PLANES) {
        const int Q = L / 4;
        g.cp = (Q + 64 * V - 1) / (64 * V);
        g.qpu = (Q + g.cp - 1) / g.cp;
        g.units = (long long)N * g.cp;
    } else {
        g.cp = g.qpu = 0;
        g.units = (g.M + 64 * V - 1) / (64 * V);
    }
    const long long want = (2048 + C - 1) / C;
    long long upb = (g.units + want - 1) / want;
    upb = upb < 4 ? 4 : (upb + 3) / 4 * 4;
    g.upb = upb;
    *splits = (int)((g.units + upb - 1) / upb);
    return g;
}

// rows per block of the column kernels (nk_norm.hip: layer_norm_bwd_params)
int col_rows_per_block(int N, int C, int vec, int* tiles, int* splits) {
    *tiles = (C + 64 * vec - 1) / (64 * vec);
    const long long want = (2048 + *tiles - 1) / *tiles;
    long long rpb = ((long long)N + want - 1) / want;
    rpb = rpb < 4 * COL_U ? 4 * COL_U : (rpb + 3) / 4 * 4;
    long long sp = (N + rpb - 1) / rpb;
    if (sp > 65535) { rpb = (((long long)N + 65534) / 65535 + 3) / 4 * 4; sp = (N + rpb - 1) / rpb; }
    *splits = (int)sp;
    return (int)rpb;
}

template <class Op>
int launch_map(nk_device* dev, const Op& op, Layout lay, int N, int C, int L, bool nt) {
    if (lay == PLANES) {
        const int Q = L / 4, segs = (Q + 1023) / 1024;
        const long long items = (long long)N * C * segs;
        hipLaunchKernelGGL((bn_plane_map_kernel<Op>), dim3((unsigned)(items < (long long)MAX_GRID ? items : (long long)MAX_GRID)), dim3(256), 0,
                           dev->compute, op, C, Q, segs, items, nt);
    } else if (lay == GENERIC) {
        const size_t n = (size_t)N * C * L;
        hipLaunchKernelGGL((bn_generic_map_kernel<Op>), dim3(nk_stream_grid(n, 256)), dim3(256), 0, dev->compute, op, C, L, n);
    } else {
        int tiles, splits;
        const int rpb = col_rows_per_block(N, C, lay == COLUMNS4 ? 4 : 1, &tiles, &splits);
        if (lay == COLUMNS4) hipLaunchKernelGGL((bn_col_map_kernel<Op, 4>), dim3(tiles, splits), dim3(256), 0, dev->compute, op, N, C, rpb, nt);
        else hipLaunchKernelGGL((bn_col_map_kernel<Op, 1>), dim3(tiles, splits), dim3(256), 0, dev->compute, op, N, C, rpb, nt);
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int normalise(nk_device* dev, const float* x, const float* gamma, const float* beta, const float* stats, float* y, int N, int C, int L) {
    NormOp op{{x}, y, stats, gamma, beta};
    return launch_map(dev, op, layout_of(C, L, al16(x) && al16(y)), N, C, L, false);
}

template <bool ASSIGN, bool INFER>
int dx_launch(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, const float* sums, int N,
              int C, int L) {
    DxOp<ASSIGN, INFER> op{};
    int s = 0;
    op.in[s++] = g;
    if (!INFER) op.in[s++] = x;
    if (!ASSIGN) op.in[s++] = dx;
    op.out = dx; op.stats = stats; op.gamma = gamma; op.sums = sums;
    op.inv_m = (float)(1.0 / ((double)N * L));
    const bool nt = nk_streams_past_cache((size_t)N * C * L * 4 * (DxOp<ASSIGN, INFER>::NIN + 1));
    return launch_map(dev, op, layout_of(C, L, al16(dx) && al16(g) && (INFER || al16(x))), N, C, L, nt);
}

int batch_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, const float* sums,
                   int N, int C, int L, bool assign) {
    NK_USE(dev);
    if (int rc = check_geometry("nk_batch_norm_bwd", N, C, L)) return rc;
    NK_CHECK(dx && g && stats && (x || !sums), "null pointer in nk_batch_norm_bwd (gamma may be NULL; sums NULL selects the inference form, which does not read x)");
    if (N == 0 || L == 0) return NK_OK;
    if (sums) return assign ? dx_launch<true, false>(dev, dx, g, x, gamma, stats, sums, N, C, L) : dx_launch<false, false>(dev, dx, g, x, gamma, stats, sums, N, C, L);
    return assign ? dx_launch<true, true>(dev, dx, g, x, gamma, stats, sums, N, C, L) : dx_launch<false, true>(dev, dx, g, x, gamma, stats, sums, N, C, L);
}

int batch_norm_bwd_params(nk_device* dev, float* dgamma, float* dbeta, const float* sums, int C, int assign) {
    NK_USE(dev);
    NK_CHECK(C > 0, "nk_batch_norm_bwd_params: C = %d (the channel count must be positive)", C);
    NK_CHECK(dgamma || dbeta, "nk_batch_norm_bwd_params: dgamma and dbeta are both NULL");
    NK_CHECK(sums, "null pointer in nk_batch_norm_bwd_params");
    hipLaunchKernelGGL(bn_params_kernel, dim3((C + 255) / 256), dim3(256), 0, dev->compute, sums, dgamma, dbeta, C, assign);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_batch_norm_fwd(nk_device* dev, const float* x, const float* gamma, const float* beta, float* y, float* stats, float* running_mean,
                      float* running_var, int N, int C, int L, double eps, double momentum) {
    NK_USE(dev);
    if (int rc = check_geometry("nk_batch_norm_fwd", N, C, L)) return rc;
    NK_CHECK(eps >= 0.0 && eps <= 3.0e38, "nk_batch_norm_fwd: eps = %g (must be finite and not negative)", eps);  // NaN fails both
    NK_CHECK(momentum >= 0.0 && momentum <= 1.0, "nk_batch_norm_fwd: momentum = %g (must be in [0, 1])", momentum);
    NK_CHECK(x && y, "null pointer in nk_batch_norm_fwd (gamma, beta, stats and the running statistics may be NULL)");
    if (N == 0 || L == 0) return NK_OK;
    const long long M = (long long)N * L;
    NK_CHECK(M > 1, "nk_batch_norm_fwd: one value per channel (N = %d, L = %d) has no variance; training needs N * L > 1", N, L);
    const Layout lay = layout_of(C, L, al16(x));
    int splits = 0, tiles = 0, rpb = 0;
    Units g{};
    if (lay == PLANES || lay == GENERIC) g = units_of(lay, N, C, L, &splits);
    else rpb = col_rows_per_block(N, C, lay == COLUMNS4 ? 4 : 1, &tiles, &splits);
    void* ws = nullptr;
    if (int rc = nk_workspace(dev, ((size_t)splits * 3 + 2) * C * sizeof(float), &ws)) return rc;
    float* part = (float*)ws;
    if (!stats) stats = part + (size_t)splits * 3 * C;  // nothing kept for a backward pass: the normalisation still needs them
    if (lay == PLANES) hipLaunchKernelGGL((bn_stats_partial_kernel<4>), dim3(C, splits), dim3(256), 0, dev->compute, x, part, g);
    else if (lay == GENERIC) hipLaunchKernelGGL((bn_stats_partial_kernel<1>), dim3(C, splits), dim3(256), 0, dev->compute, x, part, g);
    else if (lay == COLUMNS4) hipLaunchKernelGGL((bn_col_stats_partial_kernel<4>), dim3(tiles, splits), dim3(256), 0, dev->compute, x, part, N, C, rpb);
    else hipLaunchKernelGGL((bn_col_stats_partial_kernel<1>), dim3(tiles, splits), dim3(256), 0, dev->compute, x, part, N, C, rpb);
    NK_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3((C + 63) / 64), dim3(256), 0, dev->compute, (const float*)part, splits, C, (float)M, (float)eps,
                       (float)momentum, (float)((double)M / (double)(M - 1)), stats, running_mean, running_var);
    NK_LAUNCH_CHECK();
    return normalise(dev, x, gamma, beta, stats, y, N, C, L);
}

int nk_batch_norm_infer_fwd(nk_device* dev, const float* x, const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float* y, float* stats, int N, int C, int L, double eps) {
    NK_USE(dev);
    if (int rc = check_geometry("nk_batch_norm_infer_fwd", N, C, L)) return rc;
    NK_CHECK(eps >= 0.0 && eps <= 3.0e38, "nk_batch_norm_infer_fwd: eps = %g (must be finite and not negative)", eps);
    NK_CHECK(x && y && running_mean && running_var, "null pointer in nk_batch_norm_infer_fwd (gamma, beta and stats may be NULL)");
    if (N == 0 || L == 0) return NK_OK;
    if (!stats) {
        void* ws = nullptr;
        if (int rc = nk_workspace(dev, (size_t)2 * C * sizeof(float), &ws)) return rc;
        stats = (float*)ws;
    }
    hipLaunchKernelGGL(bn_infer_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, dev->compute, running_mean, running_var, (float)eps, C, stats);
    NK_LAUNCH_CHECK();
    return normalise(dev, x, gamma, beta, stats, y, N, C, L);
}

int nk_batch_norm_bwd_sums(nk_device* dev, float* sums, const float* g, const float* x, const float* stats, int N, int C, int L) {
    NK_USE(dev);
    if (int rc = check_geometry("nk_batch_norm_bwd_sums", N, C, L)) return rc;
    NK_CHECK(sums && g && x && stats, "null pointer in nk_batch_norm_bwd_sums");
    if (N == 0 || L == 0) return NK_OK;
    const Layout lay = layout_of(C, L, al16(g) && al16(x));
    int splits = 0, tiles = 0, rpb = 0;
    Units u{};
    if (lay == PLANES || lay == GENERIC) u = units_of(lay, N, C, L, &splits);
    else rpb = col_rows_per_block(N, C, lay == COLUMNS4 ? 4 : 1, &tiles, &splits);
    void* ws = nullptr;
    if (int rc = nk_workspace(dev, (size_t)splits * 2 * C * sizeof(float), &ws)) return rc;
    float* part = (float*)ws;
    const bool nt = nk_streams_past_cache((size_t)N * C * L * 8);
    if (lay == PLANES) hipLaunchKernelGGL((bn_sums_partial_kernel<4>), dim3(C, splits), dim3(256), 0, dev->compute, g, x, stats, part, u, nt);
    else if (lay == GENERIC) hipLaunchKernelGGL((bn_sums_partial_kernel<1>), dim3(C, splits), dim3(256), 0, dev->compute, g, x, stats, part, u, nt);
    else if (lay == COLUMNS4) hipLaunchKernelGGL((bn_col_sums_partial_kernel<4>), dim3(tiles, splits), dim3(256), 0, dev->compute, g, x, stats, part, N, C, rpb, nt);
    else hipLaunchKernelGGL((bn_col_sums_partial_kernel<1>), dim3(tiles, splits), dim3(256), 0, dev->compute, g, x, stats, part, N, C, rpb, nt);
    NK_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_sums_final_kernel, dim3((C + 63) / 64), dim3(256), 0, dev->compute, (const float*)part, splits, C, sums);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int nk_batch_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, const float* sums,
                      int N, int C, int L) {
    return batch_norm_bwd(dev, dx, g, x, gamma, stats, sums, N, C, L, false);
}
int nk_batch_norm_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats,
                             const float* sums, int N, int C, int L) {
    return batch_norm_bwd(dev, dx, g, x, gamma, stats, sums, N, C, L, true);
}
int nk_batch_norm_bwd_params(nk_device* dev, float* dgamma, float* dbeta, const float* sums, int C) {
    return batch_norm_bwd_params(dev, dgamma, dbeta, sums, C, 0);
}
int nk_batch_norm_bwd_params_assign(nk_device* dev, float* dgamma, float* dbeta, const float* sums, int C) {
    return batch_norm_bwd_params(dev, dgamma, dbeta, sums, C, 1);
}

}  // extern "C"
