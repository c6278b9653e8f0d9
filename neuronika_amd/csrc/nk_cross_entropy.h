// Cross entropy over class logits with integer targets (ours; semantics in include/neuronika_hip.h): log-softmax and NLL in one
// pass.  Forward reads the logits ONCE and keeps one `lse` per position; backward recomputes softmax = exp(x - lse) from the logits
// and writes their gradient: nothing of size (N, C) is saved or zero-filled.  Included by nk_norm.hip, the row-kernel unit.
//   row      class axis contiguous, C <= CE_ROW_MAX: ONE WAVE PER ROW, the row in registers (V float4 per lane, all issued before
//            any is used), max and sum by wave64 xor-shuffles, as softmax_fwd_row_kernel does
//   block    class axis contiguous, larger C: ONE BLOCK PER ROW (256 / 512 / 1024 threads by C), one pass with a running
//            (max, sum, sum of x) per lane over four float4s in flight, merged by wave shuffles and one LDS step
//   A row starts wherever row * C falls (C = 50257 is odd: three rows in four start off a 16-byte boundary), so every row is walked
//   as a scalar HEAD up to the boundary, a float4 BODY and a scalar TAIL: both families take any C and any row start.  The backward
//   kernels store through the same walk, so they need dx and x to share their offset from a 16-byte boundary; a pair that does
//   not (offset views) goes to the generic kernels.
//   generic  class axis strided (inner > 1): a thread per position, lanes along `inner` (coalesced), looping over C
// Per-position losses go to the workspace and are summed by per-block partials over fixed spans and a single-block final sum; the
// active count is an integer sum.  No float atomics: bits are a function of shape, arguments and data.
#pragma once
#include "nk_common.h"

namespace {

constexpr float CE_F32_MIN = -3.40282347e+38f;  // the max fold starts from f32::MIN, as the softmax kernels' does
constexpr int CE_ROW_MAX = 2048;                // row-in-registers up to here (8 float4 per lane)
constexpr int CE_BLOCK_512 = 16384;             // one block per row: 256 threads up to this C, 512 up to CE_BLOCK_1024, 1024 beyond
constexpr int CE_BLOCK_1024 = 65536;
constexpr int CE_MAX_PART = 1024;
constexpr long long CE_MAX_POSITIONS = 0x7fffffffLL;

// `target as usize` (nll/mod.rs:57), identical to nk_loss.hip's: Rust's saturating cast - NaN and negatives become 0, the fraction
// is dropped
__device__ __forceinline__ long long rust_f32_as_usize(float t) {
    if (!(t > 0.f)) return 0;                       // NaN, -x, 0
    if (t >= 9.2233720368547758e18f) return 0x7fffffffffffffffLL;
    return (long long)t;                            // trunc toward zero
}
// the class of position p, or -1 when the position is inactive (an id >= C selects nothing; `ignore` < 0: none)
__device__ __forceinline__ int ce_class(float t, int C, long long ignore) {
    const long long id = rust_f32_as_usize(t);
    return id < C && id != ignore ? (int)id : -1;
}
__device__ __forceinline__ float ce_loss_of(float lse, float xt, float sx, int C, float eps) {
    return eps == 0.f ? lse - xt : (1.f - eps) * (lse - xt) + eps * (lse - sx / (float)C);
}

// How a row of C floats starting at `row` splits into head scalars, float4s and tail scalars.
struct ce_walk {
    int head, nb, tail;
};
__device__ __forceinline__ ce_walk ce_walk_of(const float* row, int C) {
    ce_walk w;
    w.head = (int)((4 - ((reinterpret_cast<uintptr_t>(row) >> 2) & 3)) & 3);
    if (w.head > C) w.head = C;
    w.nb = (C - w.head) >> 2;
    w.tail = C - w.head - 4 * w.nb;
    return w;
}
// The one edge element a thread may own: thread j < head the head's j-th, thread EDGE_TAIL + j the tail's j-th.  -1: none.
constexpr int CE_EDGE_TAIL = 32;
__device__ __forceinline__ int ce_edge_col(const ce_walk& w, int tid) {
    if (tid < w.head) return tid;
    if (tid >= CE_EDGE_TAIL && tid - CE_EDGE_TAIL < w.tail) return w.head + 4 * w.nb + tid - CE_EDGE_TAIL;
    return -1;
}

__device__ __forceinline__ float ce_max4(const float4& v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }
__device__ __forceinline__ float ce_sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float ce_expsum4(const float4& v, float m) {
    return (expf(v.x - m) + expf(v.y - m)) + (expf(v.z - m) + expf(v.w - m));
}
// d (+)= scale * (exp(x - lse) - sm - on [c == t]) for the four columns from c0
template <bool ASSIGN>
__device__ __forceinline__ float4 ce_grad4(const float4& v, const float4& d, float lse, float sm, float on, float scale, int c0, int t) {
    float4 o;
    o.x = scale * (expf(v.x - lse) - sm - (c0 == t ? on : 0.f));
    o.y = scale * (expf(v.y - lse) - sm - (c0 + 1 == t ? on : 0.f));
    o.z = scale * (expf(v.z - lse) - sm - (c0 + 2 == t ? on : 0.f));
    o.w = scale * (expf(v.w - lse) - sm - (c0 + 3 == t ? on : 0.f));
    if (!ASSIGN) { o.x += d.x; o.y += d.y; o.z += d.z; o.w += d.w; }
    return o;
}

// ------------------------------------------------------------------------------------------------ row in registers
template <int V>
__global__ __launch_bounds__(256) void ce_fwd_row_kernel(const float* __restrict__ x, const float* __restrict__ target, long long rows, int C,
                                                          long long ignore, float eps, float* __restrict__ lse, float* __restrict__ loss) {
    const int lane = threadIdx.x & 63;
    const long long row = blockIdx.x * (long long)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * C;
    const ce_walk w = ce_walk_of(xr, C);
    const float4* body = reinterpret_cast<const float4*>(xr + w.head);
    float4 v[V];
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = i * 64 + lane < w.nb ? body[i * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int ec = ce_edge_col(w, lane);
    const float e = ec >= 0 ? xr[ec] : 0.f;
    const int t = ce_class(target[row], C, ignore);
    const float xt = t >= 0 ? xr[t] : 0.f;
    float m = ec >= 0 ? fmaxf(CE_F32_MIN, e) : CE_F32_MIN;
#pragma unroll
    for (int i = 0; i < V; ++i)
        if (i * 64 + lane < w.nb) m = fmaxf(m, ce_max4(v[i]));
    m = nk_wave_max(m);
    float s = ec >= 0 ? expf(e - m) : 0.f, sx = e;
#pragma unroll
    for (int i = 0; i < V; ++i)
        if (i * 64 + lane < w.nb) {
            s += ce_expsum4(v[i], m);
            sx += ce_sum4(v[i]);
        }
    s = nk_wave_sum(s);
    sx = nk_wave_sum(sx);
    if (lane == 0) {
        const float l = m + logf(s);
        lse[row] = l;
        loss[row] = t >= 0 ? ce_loss_of(l, xt, sx, C, eps) : 0.f;
    }
}

// flags: bit 0 Mean (scale by 1 / *count), bit 1 `nt` loads (operands beyond the Infinity Cache)
template <int V, bool ASSIGN>
__global__ __launch_bounds__(256) void ce_bwd_row_kernel(float* __restrict__ dx, const float* __restrict__ gs, const float* __restrict__ x,
                                                          const float* __restrict__ target, const float* __restrict__ lse,
                                                          const int* __restrict__ count, long long rows, int C, long long ignore, float eps,
                                                          int flags) {
    const int lane = threadIdx.x & 63;
    const long long row = blockIdx.x * (long long)(blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * C;
    float* dr = dx + row * C;
    const ce_walk w = ce_walk_of(xr, C);  // dr shares xr's offset from a 16-byte boundary (checked at launch)
    const int ec = ce_edge_col(w, lane);
    float4* dbody = reinterpret_cast<float4*>(dr + w.head);
    const int t = ce_class(target[row], C, ignore);
    if (t < 0) {  // an inactive position: a zero gradient row
        if (ASSIGN) {
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (i * 64 + lane < w.nb) nk_store_stream(dbody + i * 64 + lane, make_float4(0.f, 0.f, 0.f, 0.f));
            if (ec >= 0) dr[ec] = 0.f;
        }
        return;
    }
    const bool nt = flags & 2;
    const float4* body = reinterpret_cast<const float4*>(xr + w.head);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v[V], d[V];
#pragma unroll
    for (int i = 0; i < V; ++i) v[i] = i * 64 + lane < w.nb ? nk_load_stream(body + i * 64 + lane, nt) : zero;
    if (!ASSIGN) {
#pragma unroll
        for (int i = 0; i < V; ++i) d[i] = i * 64 + lane < w.nb ? nk_load_stream(dbody + i * 64 + lane, nt) : zero;
    }
    const float e = ec >= 0 ? xr[ec] : 0.f, de = !ASSIGN && ec >= 0 ? dr[ec] : 0.f;
    const float l = lse[row], sm = eps / (float)C, on = 1.f - eps;
    const float scale = flags & 1 ? gs[0] * (1.f / (float)count[0]) : gs[0];
#pragma unroll
    for (int i = 0; i < V; ++i)
        if (i * 64 + lane < w.nb)
            nk_store_stream(dbody + i * 64 + lane, ce_grad4<ASSIGN>(v[i], ASSIGN ? zero : d[i], l, sm, on, scale, w.head + 4 * (i * 64 + lane), t));
    if (ec >= 0) {
        const float o = scale * (expf(e - l) - sm - (ec == t ? on : 0.f));
        dr[ec] = ASSIGN ? o : o + de;
    }
}

// ------------------------------------------------------------------------------------------------ one block per row
// running (max, sum of exp(x - max), sum of x) of a lane, advanced by a group of quads
__device__ __forceinline__ void ce_online(float& m, float& s, float cm) {
    const float mn = fmaxf(m, cm);
    s *= expf(m - mn);
    m = mn;
}

template <int NT>
__global__ __launch_bounds__(NT) void ce_fwd_block_kernel(const float* __restrict__ x, const float* __restrict__ target, int C, long long ignore,
                                                          float eps, float* __restrict__ lse, float* __restrict__ loss) {
    __shared__ float red[3][NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const long long row = blockIdx.x;
    const float* xr = x + row * C;
    const ce_walk w = ce_walk_of(xr, C);
    const float4* body = reinterpret_cast<const float4*>(xr + w.head);
    const int ec = ce_edge_col(w, tid);
    const float e = ec >= 0 ? xr[ec] : 0.f;
    float m = CE_F32_MIN, s = 0.f, sx = 0.f;
    int q = tid;
    for (; q + 3 * NT < w.nb; q += 4 * NT) {
        float4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = body[q + u * NT];
        ce_online(m, s, fmaxf(fmaxf(ce_max4(r[0]), ce_max4(r[1])), fmaxf(ce_max4(r[2]), ce_max4(r[3]))));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s += ce_expsum4(r[u], m);
            sx += ce_sum4(r[u]);
        }
    }
    {  // the last, partial trip
        float4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = q + u * NT < w.nb ? body[q + u * NT] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q + u * NT < w.nb) {
                ce_online(m, s, ce_max4(r[u]));
                s += ce_expsum4(r[u], m);
                sx += ce_sum4(r[u]);
            }
    }
    if (ec >= 0) {
        ce_online(m, s, e);
        s += expf(e - m);
        sx += e;
    }
    const float wm = nk_wave_max(m);
    s = nk_wave_sum(s * expf(m - wm));
    sx = nk_wave_sum(sx);
    if (lane == 0) {
        red[0][wid] = wm;
        red[1][wid] = s;
        red[2][wid] = sx;
    }
    __syncthreads();
    if (tid == 0) {
        float bm = red[0][0];
#pragma unroll
        for (int i = 1; i < NT / 64; ++i) bm = fmaxf(bm, red[0][i]);
        float bs = 0.f, bx = 0.f;
#pragma unroll
        for (int i = 0; i < NT / 64; ++i) {
            bs += red[1][i] * expf(red[0][i] - bm);
            bx += red[2][i];
        }
        const float l = bm + logf(bs);
        const int t = ce_class(target[row], C, ignore);
        lse[row] = l;
        loss[row] = t >= 0 ? ce_loss_of(l, xr[t], bx, C, eps) : 0.f;
    }
}

template <int NT, bool ASSIGN>
__global__ __launch_bounds__(NT) void ce_bwd_block_kernel(float* __restrict__ dx, const float* __restrict__ gs, const float* __restrict__ x,
                                                          const float* __restrict__ target, const float* __restrict__ lse,
                                                          const int* __restrict__ count, int C, long long ignore, float eps, int flags) {
    const int tid = threadIdx.x;
    const long long row = blockIdx.x;
    const float* xr = x + row * C;
    float* dr = dx + row * C;
    const ce_walk w = ce_walk_of(xr, C);  // dr shares xr's offset from a 16-byte boundary (checked at launch)
    const int ec = ce_edge_col(w, tid);
    float4* dbody = reinterpret_cast<float4*>(dr + w.head);
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const int t = ce_class(target[row], C, ignore);
    if (t < 0) {  // an inactive position: a zero gradient row
        if (ASSIGN) {
            for (int q = tid; q < w.nb; q += NT) nk_store_stream(dbody + q, zero);
            if (ec >= 0) dr[ec] = 0.f;
        }
        return;
    }
    const bool nt = flags & 2;
    const float4* body = reinterpret_cast<const float4*>(xr + w.head);
    const float l = lse[row], sm = eps / (float)C, on = 1.f - eps;
    const float scale = flags & 1 ? gs[0] * (1.f / (float)count[0]) : gs[0];
    if (ec >= 0) {
        const float o = scale * (expf(xr[ec] - l) - sm - (ec == t ? on : 0.f));
        dr[ec] = ASSIGN ? o : o + dr[ec];
    }
    int q = tid;
    for (; q + 3 * NT < w.nb; q += 4 * NT) {
        float4 r[4], d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = nk_load_stream(body + q + u * NT, nt);
        if (!ASSIGN) {
#pragma unroll
            for (int u = 0; u < 4; ++u) d[u] = nk_load_stream(dbody + q + u * NT, nt);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            nk_store_stream(dbody + q + u * NT, ce_grad4<ASSIGN>(r[u], ASSIGN ? zero : d[u], l, sm, on, scale, w.head + 4 * (q + u * NT), t));
    }
    {  // the last, partial trip
        float4 r[4], d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = q + u * NT < w.nb ? nk_load_stream(body + q + u * NT, nt) : zero;
        if (!ASSIGN) {
#pragma unroll
            for (int u = 0; u < 4; ++u) d[u] = q + u * NT < w.nb ? nk_load_stream(dbody + q + u * NT, nt) : zero;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (q + u * NT < w.nb)
                nk_store_stream(dbody + q + u * NT, ce_grad4<ASSIGN>(r[u], ASSIGN ? zero : d[u], l, sm, on, scale, w.head + 4 * (q + u * NT), t));
    }
}

// ------------------------------------------------------------------------------------------------ generic (class axis strided)
// A thread per position, lanes along `inner`; x[(n C + c) inner + r].  Two passes over the classes forward (max; sum), one backward.
__global__ void ce_fwd_generic_kernel(const float* __restrict__ x, const float* __restrict__ target, long long positions, int C, long long inner,
                                      long long ignore, float eps, float* __restrict__ lse, float* __restrict__ loss) {
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < positions; p += (long long)gridDim.x * blockDim.x) {
        const float* xp = x + (p / inner) * C * inner + p % inner;
        float m = CE_F32_MIN;
#pragma unroll 4
        for (int c = 0; c < C; ++c) m = fmaxf(m, xp[c * inner]);
        float s = 0.f, sx = 0.f;
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            const float v = xp[c * inner];
            s += expf(v - m);
            sx += v;
        }
        const float l = m + logf(s);
        const int t = ce_class(target[p], C, ignore);
        lse[p] = l;
        loss[p] = t >= 0 ? ce_loss_of(l, xp[t * inner], sx, C, eps) : 0.f;
    }
}

template <bool ASSIGN>
__global__ void ce_bwd_generic_kernel(float* __restrict__ dx, const float* __restrict__ gs, const float* __restrict__ x,
                                      const float* __restrict__ target, const float* __restrict__ lse, const int* __restrict__ count,
                                      long long positions, int C, long long inner, long long ignore, float eps, int flags) {
    const float sm = eps / (float)C, on = 1.f - eps;
    for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < positions; p += (long long)gridDim.x * blockDim.x) {
        const long long base = (p / inner) * C * inner + p % inner;
        const int t = ce_class(target[p], C, ignore);
        if (t < 0) {
            if (ASSIGN)
                for (int c = 0; c < C; ++c) dx[base + c * inner] = 0.f;
            continue;
        }
        const float l = lse[p];
        const float scale = flags & 1 ? gs[0] * (1.f / (float)count[0]) : gs[0];
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            const long long o = base + c * inner;
            const float v = scale * (expf(x[o] - l) - sm - (c == t ? on : 0.f));
            dx[o] = ASSIGN ? v : v + dx[o];
        }
    }
}

// ------------------------------------------------------------------------------------------------ loss sum and active count
// Block b owns the contiguous span [b per, (b + 1) per) of the positions: lpart[b] = the sum of its losses (`loss` may be null),
// cpart[b] = the number of its active positions.
__global__ __launch_bounds__(256) void ce_partial_kernel(const float* __restrict__ loss, const float* __restrict__ target, long long positions,
                                                          int C, long long ignore, float* __restrict__ lpart, int* __restrict__ cpart) {
    __shared__ float red[4];
    __shared__ int cred[4];
    const long long per = (positions + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, end = lo + per < positions ? lo + per : positions;
    float a = 0.f;
    int n = 0;
    for (long long p = lo + threadIdx.x; p < end; p += 256) {
        if (loss) a += loss[p];
        n += ce_class(target[p], C, ignore) >= 0;
    }
    const float s = nk_block_sum<256>(a, red);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        if (lpart) lpart[blockIdx.x] = s;
        cpart[blockIdx.x] = (cred[0] + cred[1]) + (cred[2] + cred[3]);
    }
}
// out[0] = the sum of the partials, divided by the active count under Mean (0 when nothing is active); count[0] = the active count
__global__ __launch_bounds__(256) void ce_final_kernel(const float* __restrict__ lpart, const int* __restrict__ cpart, int nparts, int mean,
                                                        float* __restrict__ out, int* __restrict__ count) {
    __shared__ float red[4];
    __shared__ int cred[4];
    float a = 0.f;
    int n = 0;
    for (int i = threadIdx.x; i < nparts; i += 256) {
        if (lpart) a += lpart[i];
        n += cpart[i];
    }
    const float s = nk_block_sum<256>(a, red);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = (cred[0] + cred[1]) + (cred[2] + cred[3]);
        if (out) out[0] = mean ? (total > 0 ? s / (float)total : 0.f) : s;
        count[0] = total;
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct ce_geom {
    long long N, inner, positions;
    int C;
};
int ce_check(nk_device* dev, const int* shape, int nd, int reduction, double eps, const char* what, ce_geom* g) {
    NK_CHECK(reduction == NK_REDUCTION_SUM || reduction == NK_REDUCTION_MEAN, "%s: unknown reduction %d", what, reduction);
    NK_CHECK(nd >= 2 && nd <= NK_MAX_DIMS && shape, "%s: input must be (minibatch, C, d1..dk), got %d dims", what, nd);
    NK_CHECK(eps >= 0.0 && eps < 1.0, "%s: label_smoothing must be in [0, 1), got %g", what, eps);  // NaN fails both tests
    g->N = shape[0];
    g->C = shape[1];
    g->inner = 1;
    for (int i = 0; i < nd; ++i) NK_CHECK(shape[i] >= 0, "%s: negative extent", what);
    for (int i = 2; i < nd; ++i) {
        g->inner *= shape[i];
        NK_CHECK(g->inner <= CE_MAX_POSITIONS, "%s: more than 2^31 - 1 positions", what);
    }
    NK_CHECK((double)g->N * (double)g->inner <= (double)CE_MAX_POSITIONS, "%s: more than 2^31 - 1 positions", what);
    g->positions = g->N * g->inner;
    NK_CHECK(dev != nullptr, "%s: null device handle", what);
    return NK_OK;
}
size_t ce_round256(size_t b) { return (b + 255) & ~(size_t)255; }
int ce_parts(long long positions) {
    const long long b = (positions + 255) / 256;
    return (int)(b < 1 ? 1 : (b > CE_MAX_PART ? CE_MAX_PART : b));
}
// workspace: lpart[CE_MAX_PART] | cpart[CE_MAX_PART] | count | loss[positions]
struct ce_ws {
    float* lpart;
    int* cpart;
    int* count;
    float* loss;
};
int ce_workspace(nk_device* dev, long long positions, ce_ws* w) {
    const size_t head = ce_round256(CE_MAX_PART * 4);
    void* ws = nullptr;
    if (int rc = nk_workspace(dev, 2 * head + 256 + ce_round256((size_t)positions * 4), &ws)) return rc;
    char* base = static_cast<char*>(ws);
    w->lpart = reinterpret_cast<float*>(base);
    w->cpart = reinterpret_cast<int*>(base + head);
    w->count = reinterpret_cast<int*>(base + 2 * head);
    w->loss = reinterpret_cast<float*>(base + 2 * head + 256);
    return NK_OK;
}

template <bool ASSIGN>
int ce_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* target, const float* lse, const int* shape, int nd,
           int reduction, long long ignore_index, double label_smoothing) {
    const char* what = ASSIGN ? "nk_cross_entropy_bwd_assign" : "nk_cross_entropy_bwd";
    ce_geom s;
    if (int rc = ce_check(dev, shape, nd, reduction, label_smoothing, what, &s)) return rc;
    if (s.positions == 0 || s.C == 0) return NK_OK;
    NK_CHECK(dx && g && x && target && lse, "%s: null pointer", what);
    NK_USE(dev);
    const long long ignore = ignore_index < 0 ? -1 : ignore_index;
    const float eps = (float)label_smoothing;
    const int C = s.C;
    const bool mean = reduction == NK_REDUCTION_MEAN;
    ce_ws w;
    if (int rc = ce_workspace(dev, 0, &w)) return rc;
    if (mean) {  // the active count, from the targets alone
        const int parts = ce_parts(s.positions);
        hipLaunchKernelGGL(ce_partial_kernel, dim3(parts), dim3(256), 0, dev->compute, (const float*)nullptr, target, s.positions, C, ignore,
                           (float*)nullptr, w.cpart);
        NK_LAUNCH_CHECK();
        hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(256), 0, dev->compute, (const float*)nullptr, w.cpart, parts, 0, (float*)nullptr, w.count);
        NK_LAUNCH_CHECK();
    }
    // x read, dx written (and read by `+=`), each once
    const int flags = (mean ? 1 : 0) | (nk_streams_past_cache((size_t)s.positions * C * (ASSIGN ? 8 : 12)) ? 2 : 0);
    const bool together = ((reinterpret_cast<uintptr_t>(x) ^ reinterpret_cast<uintptr_t>(dx)) & 15) == 0;
    if (s.inner > 1 || !together) {
        hipLaunchKernelGGL((ce_bwd_generic_kernel<ASSIGN>), dim3(nk_stream_grid((size_t)s.positions, 256)), dim3(256), 0, dev->compute, dx, g, x,
                           target, lse, w.count, s.positions, C, s.inner, ignore, eps, flags);
    } else if (C <= CE_ROW_MAX) {
        const dim3 grid((unsigned)((s.positions + 3) / 4)), block(256);
#define CE_ROW(V) hipLaunchKernelGGL((ce_bwd_row_kernel<V, ASSIGN>), grid, block, 0, dev->compute, dx, g, x, target, lse, w.count, s.positions, C, ignore, eps, flags)
        if (C <= 256) CE_ROW(1);
        else if (C <= 512) CE_ROW(2);
        else if (C <= 1024) CE_ROW(4);
        else CE_ROW(8);
#undef CE_ROW
    } else {
        const dim3 grid((unsigned)s.positions);
#define CE_BLOCK(NT) hipLaunchKernelGGL((ce_bwd_block_kernel<NT, ASSIGN>), grid, dim3(NT), 0, dev->compute, dx, g, x, target, lse, w.count, C, ignore, eps, flags)
        if (C <= CE_BLOCK_512) CE_BLOCK(256);
        else if (C <= CE_BLOCK_1024) CE_BLOCK(512);
        else CE_BLOCK(1024);
#undef CE_BLOCK
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_cross_entropy_fwd(nk_device* dev, const float* x, const float* target, const int* shape, int nd, int reduction, long long ignore_index,
                         double label_smoothing, float* lse, float* out) {
    const char* what = "nk_cross_entropy_fwd";
    ce_geom s;
    if (int rc = ce_check(dev, shape, nd, reduction, label_smoothing, what, &s)) return rc;
    NK_CHECK(out != nullptr, "%s: null output scalar", what);
    const bool empty = s.positions == 0 || s.C == 0;
    NK_CHECK(empty || (x && target && lse), "%s: null pointer", what);
    NK_USE(dev);
    if (empty) {  // no class or no position: loss 0, lse not written
        NK_HIP(hipMemsetAsync(out, 0, sizeof(float), dev->compute));
        return NK_OK;
    }
    const long long ignore = ignore_index < 0 ? -1 : ignore_index;
    const float eps = (float)label_smoothing;
    const int C = s.C;
    ce_ws w;
    if (int rc = ce_workspace(dev, s.positions, &w)) return rc;
    if (s.inner > 1) {
        hipLaunchKernelGGL(ce_fwd_generic_kernel, dim3(nk_stream_grid((size_t)s.positions, 256)), dim3(256), 0, dev->compute, x, target, s.positions,
                           C, s.inner, ignore, eps, lse, w.loss);
    } else if (C <= CE_ROW_MAX) {
        const dim3 grid((unsigned)((s.positions + 3) / 4)), block(256);
#define CE_ROW(V) hipLaunchKernelGGL((ce_fwd_row_kernel<V>), grid, block, 0, dev->compute, x, target, s.positions, C, ignore, eps, lse, w.loss)
        if (C <= 256) CE_ROW(1);
        else if (C <= 512) CE_ROW(2);
        else if (C <= 1024) CE_ROW(4);
        else CE_ROW(8);
#undef CE_ROW
    } else {
        const dim3 grid((unsigned)s.positions);
#define CE_BLOCK(NT) hipLaunchKernelGGL((ce_fwd_block_kernel<NT>), grid, dim3(NT), 0, dev->compute, x, target, C, ignore, eps, lse, w.loss)
        if (C <= CE_BLOCK_512) CE_BLOCK(256);
        else if (C <= CE_BLOCK_1024) CE_BLOCK(512);
        else CE_BLOCK(1024);
#undef CE_BLOCK
    }
    NK_LAUNCH_CHECK();
    const int parts = ce_parts(s.positions);
    hipLaunchKernelGGL(ce_partial_kernel, dim3(parts), dim3(256), 0, dev->compute, (const float*)w.loss, target, s.positions, C, ignore, w.lpart,
                       w.cpart);
    NK_LAUNCH_CHECK();
    hipLaunchKernelGGL(ce_final_kernel, dim3(1), dim3(256), 0, dev->compute, (const float*)w.lpart, (const int*)w.cpart, parts,
                       reduction == NK_REDUCTION_MEAN ? 1 : 0, out, w.count);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int nk_cross_entropy_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* target, const float* lse, const int* shape, int nd,
                         int reduction, long long ignore_index, double label_smoothing) {
    return ce_bwd<false>(dev, dx, g, x, target, lse, shape, nd, reduction, ignore_index, label_smoothing);
}

int nk_cross_entropy_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, const float* target, const float* lse, const int* shape,
                                int nd, int reduction, long long ignore_index, double label_smoothing) {
    return ce_bwd<true>(dev, dx, g, x, target, lse, shape, nd, reduction, ignore_index, label_smoothing);
}

}  // extern "C"
