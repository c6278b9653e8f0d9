// Max and average pooling over 1, 2 or 3 spatial axes of an (N, C, spatial...) tensor: forward (values, and for max pooling the
// int32 offset of the selected element inside its own plane), and both backward passes in GATHER form - a thread owns input
// elements and walks the outputs whose windows cover them in a fixed order - so there is no atomic anywhere and every output
// repeats bit for bit.  Semantics: include/neuronika_hip.h.  Every geometry is normalised to three axes (D, H, W): a 1-d call is
// (1, 1, W), a 2-d call (1, H, W), the missing axes with window 1, stride 1, padding 0.
//
// Three classes, chosen by `pool_class` from the geometry and the pointers' alignment:
//   WINDOWED  D trivial, (k, s, p) along W one of 2/2/0, 3/2/0, 3/2/1, 3/1/0, 3/1/1 (compile time), any window along H, in_W % 4 == 0
//             and 16-byte aligned pointers.  Forward: a lane makes four adjacent outputs of one output row; per input row it
//             reads an aligned run of 4 s floats as 16-byte loads and the k - s + p columns beside it as scalars, border columns
//             and rows masked; y and idx leave as 16-byte stores when out_W % 4 == 0 (3/2/0 never has that: scalar stores).
//             Items are walked in row-major order, so the rows two neighbouring output rows share are read by neighbouring waves
//             within a few hundred cycles of each other and come from L2.  Backward: a lane owns 16 bytes of dx and gathers from
//             the covering outputs, compile-time bounds along W.
//   PLANE     every out_i == 1, k_i == in_i, no padding: G = 16 / 64 / 256 lanes own one contiguous plane of L floats (L <= 128 /
//             <= 16384 / beyond) and reduce it with wave shuffles (G = 256: through LDS); 16-byte loads when L % 4 == 0 and x is
//             aligned.  Max pooling reduces (value, offset) pairs.  Backward: g[plane] / L (or g[plane] at idx[plane]) broadcast in
//             16-byte stores when L % 4 == 0 and dx is aligned, the generic gather otherwise.
//   GENERIC   everything else inside the contract: runtime loops, scalar accesses, one thread per output (forward) or per input
//             element (backward), lanes along the innermost axis.
#include "nk_common.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace {

struct PoolGeom {
    int in[3], out[3], k[3], s[3], p[3];
    int in_plane, out_plane;
    long long planes;  // N * C
};

// first / last output index along one axis whose window holds input index i
__device__ __forceinline__ int pool_cover_lo(int i, int k, int s, int p) {
    const int a = i + p - k + 1;  // ceil(a / s), clamped at 0
    return a <= 0 ? 0 : (a + s - 1) / s;
}
__device__ __forceinline__ int pool_cover_hi(int i, int s, int p, int out) {
    const int h = (i + p) / s;
    return h < out - 1 ? h : out - 1;
}
// in-range positions of window o along one axis
__device__ __forceinline__ int pool_count(int o, int k, int s, int p, int in) {
    const int a = o * s - p, b = a + k;
    return (b < in ? b : in) - (a > 0 ? a : 0);
}
// selection rule of max pooling, in scan order: a larger value, or the first NaN
__device__ __forceinline__ bool pool_takes(float v, float best) { return v > best || (v != v && best == best); }
// merge of two (value, offset) candidates that were each found by that rule over disjoint offset sets: the smallest NaN offset if any
// NaN, else the largest value at its smallest offset.  Associative and commutative.
__device__ __forceinline__ void pool_pair_merge(float& v, int& i, float ov, int oi) {
    const bool vn = v != v, on = ov != ov;
    const bool take = (vn || on) ? (on && (!vn || oi < i)) : (ov > v || (ov == v && oi < i));
    if (take) { v = ov; i = oi; }
}

__device__ __forceinline__ void pool_store4(float4* p, const float4& v, bool nt) {
    if (nt) nk_store_stream(p, v);
    else *p = v;
}

// ------------------------------------------------------------------------------------------------ generic class
template <bool MAX>
__global__ __launch_bounds__(256) void pool_generic_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int* __restrict__ idx,
                                                               PoolGeom q, int count_include_pad) {
    const long long total = q.planes * q.out_plane;
    for (long long o = blockIdx.x * 256ll + threadIdx.x; o < total; o += (long long)gridDim.x * 256) {
        const long long plane = o / q.out_plane;
        int r = (int)(o - plane * q.out_plane);
        const int ow = r % q.out[2]; r /= q.out[2];
        const int oh = r % q.out[1], od = r / q.out[1];
        const int d0 = od * q.s[0] - q.p[0], h0 = oh * q.s[1] - q.p[1], w0 = ow * q.s[2] - q.p[2];
        const int d_lo = max(d0, 0), d_hi = min(d0 + q.k[0], q.in[0]);
        const int h_lo = max(h0, 0), h_hi = min(h0 + q.k[1], q.in[1]);
        const int w_lo = max(w0, 0), w_hi = min(w0 + q.k[2], q.in[2]);
        const float* xp = x + plane * q.in_plane;
        if (MAX) {
            float best = -INFINITY;
            int bi = (d_lo * q.in[1] + h_lo) * q.in[2] + w_lo;
            for (int d = d_lo; d < d_hi; ++d)
                for (int h = h_lo; h < h_hi; ++h) {
                    const int base = (d * q.in[1] + h) * q.in[2];
                    for (int w = w_lo; w < w_hi; ++w) {
                        const float v = xp[base + w];
                        if (pool_takes(v, best)) { best = v; bi = base + w; }
                    }
                }
            y[o] = best;
            if (idx) idx[o] = bi;
        } else {
            float acc = 0.f;
            for (int d = d_lo; d < d_hi; ++d)
                for (int h = h_lo; h < h_hi; ++h) {
                    const float* row = xp + (d * q.in[1] + h) * q.in[2];
                    for (int w = w_lo; w < w_hi; ++w) acc += row[w];
                }
            const int div = count_include_pad ? q.k[0] * q.k[1] * q.k[2] : (d_hi - d_lo) * (h_hi - h_lo) * (w_hi - w_lo);
            y[o] = acc / (float)div;
        }
    }
}

template <bool MAX>
__global__ __launch_bounds__(256) void pool_generic_bwd_kernel(float* __restrict__ dx, const float* __restrict__ g, const int* __restrict__ idx,
                                                               PoolGeom q, int count_include_pad, int assign) {
    const long long total = q.planes * q.in_plane;
    const int full = q.k[0] * q.k[1] * q.k[2];
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long plane = i / q.in_plane;
        const int off = (int)(i - plane * q.in_plane);
        int r = off;
        const int w = r % q.in[2]; r /= q.in[2];
        const int h = r % q.in[1], d = r / q.in[1];
        const int od_lo = pool_cover_lo(d, q.k[0], q.s[0], q.p[0]), od_hi = pool_cover_hi(d, q.s[0], q.p[0], q.out[0]);
        const int oh_lo = pool_cover_lo(h, q.k[1], q.s[1], q.p[1]), oh_hi = pool_cover_hi(h, q.s[1], q.p[1], q.out[1]);
        const int ow_lo = pool_cover_lo(w, q.k[2], q.s[2], q.p[2]), ow_hi = pool_cover_hi(w, q.s[2], q.p[2], q.out[2]);
        const float* gp = g + plane * q.out_plane;
        const int* ip = MAX ? idx + plane * q.out_plane : nullptr;
        float acc = 0.f;
        for (int od = od_lo; od <= od_hi; ++od)
            for (int oh = oh_lo; oh <= oh_hi; ++oh) {
                const int base = (od * q.out[1] + oh) * q.out[2];
                int dh = full;
                if (!MAX && !count_include_pad)
                    dh = pool_count(od, q.k[0], q.s[0], q.p[0], q.in[0]) * pool_count(oh, q.k[1], q.s[1], q.p[1], q.in[1]);
                for (int ow = ow_lo; ow <= ow_hi; ++ow) {
                    const float gv = gp[base + ow];
                    if (MAX) {
                        acc += ip[base + ow] == off ? gv : 0.f;
                    } else {
                        const int div = count_include_pad ? full : dh * pool_count(ow, q.k[2], q.s[2], q.p[2], q.in[2]);
                        acc += gv / (float)div;
                    }
                }
            }
        dx[i] = assign ? acc : dx[i] + acc;
    }
}

// ------------------------------------------------------------------------------------------------ windowed class
struct PoolWin {
    int IH, IW, OH, OW;
    int kh, sh, ph;
    int groups;       // lane items per row: ceil(OW / 4) forward, IW / 4 backward
    long long items;  // planes * rows * groups
    int count_include_pad, vector_store, nt, assign;
};
struct PoolItem {
    long long plane;
    int row, j;
};
// (plane, row, group) of a flat item; one division chain per item, 32-bit when the launch's item count allows
__device__ __forceinline__ PoolItem pool_item(size_t item, int rows, int groups, bool narrow) {
    PoolItem it;
    if (narrow) {
        const unsigned t = (unsigned)item, r = t / (unsigned)groups;
        it.j = (int)(t - r * (unsigned)groups);
        const unsigned pl = r / (unsigned)rows;
        it.row = (int)(r - pl * (unsigned)rows);
        it.plane = pl;
    } else {
        const size_t r = item / (size_t)groups;
        it.j = (int)(item - r * (size_t)groups);
        it.plane = (long long)(r / (size_t)rows);
        it.row = (int)(r - (size_t)it.plane * (size_t)rows);
    }
    return it;
}
struct PoolOut4 {
    float4 y;
    int4 i;
    size_t o;  // flat index of the first of the four outputs
    int ow;
};

template <int KW, int SW, int PW, bool MAX>
__global__ __launch_bounds__(256) void pool_win_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int* __restrict__ idx, PoolWin q) {
    constexpr int SPAN = 3 * SW + KW;  // input columns behind four adjacent outputs
    constexpr int CORE = 4 * SW;       // of which the aligned run [a, a + CORE) comes as 16-byte loads
    const bool narrow = q.items < (1ll << 31);
    const float pad = MAX ? -INFINITY : 0.f;
    auto compute = [&](size_t item) {
        const PoolItem it = pool_item(item, q.OH, q.groups, narrow);
        const int oh = it.row, h0 = oh * q.sh - q.ph;
        const int h_lo = max(h0, 0), h_hi = min(h0 + q.kh, q.IH);
        const int a = CORE * it.j;
        const float* xp = x + (size_t)it.plane * q.IH * q.IW;
        float best[4], acc[4];
        int bi[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int w0 = (4 * it.j + e) * SW - PW;
            best[e] = -INFINITY;
            acc[e] = 0.f;
            bi[e] = h_lo * q.IW + max(w0, 0);
        }
        for (int ih = h_lo; ih < h_hi; ++ih) {
            const float* row = xp + (size_t)ih * q.IW;
            float v[SPAN];  // v[t] = column a - PW + t, `pad` outside the row
#pragma unroll
            for (int c = 0; c < SW; ++c) {
                float4 f = make_float4(pad, pad, pad, pad);
                if (a + 4 * c < q.IW) f = *reinterpret_cast<const float4*>(row + a + 4 * c);  // IW % 4 == 0: the whole group is inside
                const float fe[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (PW + 4 * c + e < SPAN) v[PW + 4 * c + e] = fe[e];
            }
#pragma unroll
            for (int t = 0; t < SPAN; ++t) {
                const int u = t - PW;
                if (u < 0 || u >= CORE) {
                    const int col = a + u;
                    v[t] = (col >= 0 && col < q.IW) ? row[col] : pad;
                }
            }
            const int rowoff = ih * q.IW + a - PW;
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < KW; ++t) {
                    const float val = v[e * SW + t];
                    if (MAX) {
                        if (pool_takes(val, best[e])) { best[e] = val; bi[e] = rowoff + e * SW + t; }
                    } else {
                        acc[e] += val;
                    }
                }
        }
        PoolOut4 r;
        r.ow = 4 * it.j;
        r.o = ((size_t)it.plane * q.OH + oh) * q.OW + r.ow;
        if (MAX) {
            r.y = make_float4(best[0], best[1], best[2], best[3]);
            r.i = make_int4(bi[0], bi[1], bi[2], bi[3]);
        } else {
            float d[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                d[e] = (float)(q.count_include_pad ? q.kh * KW : (h_hi - h_lo) * pool_count(4 * it.j + e, KW, SW, PW, q.IW));
            r.y = make_float4(acc[0] / d[0], acc[1] / d[1], acc[2] / d[2], acc[3] / d[3]);
            r.i = make_int4(0, 0, 0, 0);
        }
        return r;
    };
    auto store = [&](size_t, const PoolOut4& r) {
        if (q.vector_store) {
            pool_store4(reinterpret_cast<float4*>(y + r.o), r.y, q.nt);
            if (MAX && idx)
                pool_store4(reinterpret_cast<float4*>(idx + r.o),
                            make_float4(__int_as_float(r.i.x), __int_as_float(r.i.y), __int_as_float(r.i.z), __int_as_float(r.i.w)), q.nt);
        } else {
            const float ye[4] = {r.y.x, r.y.y, r.y.z, r.y.w};
            const int ie[4] = {r.i.x, r.i.y, r.i.z, r.i.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (r.ow + e < q.OW) {
                    y[r.o + e] = ye[e];
                    if (MAX && idx) idx[r.o + e] = ie[e];
                }
        }
    };
    nk_span_walk<2>((size_t)q.items, compute, store);
}

constexpr int pool_ceil_div(int a, int b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }

template <int KW, int SW, int PW, bool MAX>
__global__ __launch_bounds__(256) void pool_win_bwd_kernel(float* __restrict__ dx, const float* __restrict__ g, const int* __restrict__ idx, PoolWin q) {
    // input column 4 j + e lies in the window of output column (4 / SW) j + c  iff  0 <= e + PW - c SW < KW
    constexpr int CLO = pool_ceil_div(PW - KW + 1, SW), CHI = (3 + PW) / SW, NC = CHI - CLO + 1;
    const bool narrow = q.items < (1ll << 31);
    struct Acc { float4 v; size_t at; };
    auto compute = [&](size_t item) {
        const PoolItem it = pool_item(item, q.IH, q.groups, narrow);
        const int ih = it.row, own = ih * q.IW + 4 * it.j;
        const int oh_lo = pool_cover_lo(ih, q.kh, q.sh, q.ph), oh_hi = pool_cover_hi(ih, q.sh, q.ph, q.OH);
        const int ow_b = (4 / SW) * it.j + CLO;
        const float* gp = g + (size_t)it.plane * q.OH * q.OW;
        const int* ip = MAX ? idx + (size_t)it.plane * q.OH * q.OW : nullptr;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int oh = oh_lo; oh <= oh_hi; ++oh) {
            const int base = oh * q.OW;
            const int dh = (!MAX && !q.count_include_pad) ? pool_count(oh, q.kh, q.sh, q.ph, q.IH) : q.kh;
            float gv[NC];
            int iv[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int ow = ow_b + c;
                const bool ok = ow >= 0 && ow < q.OW;
                gv[c] = ok ? gp[base + ow] : 0.f;
                if (MAX) {
                    iv[c] = ok ? ip[base + ow] : -1;
                } else {
                    const int div = q.count_include_pad ? q.kh * KW : dh * pool_count(ok ? ow : 0, KW, SW, PW, q.IW);
                    gv[c] = gv[c] / (float)div;
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int t = e + PW - (CLO + c) * SW;
                    if (t >= 0 && t < KW) acc[e] += MAX ? (iv[c] == own + e ? gv[c] : 0.f) : gv[c];
                }
        }
        Acc r;
        r.at = (size_t)it.plane * q.IH * q.IW + own;
        r.v = make_float4(acc[0], acc[1], acc[2], acc[3]);
        if (!q.assign) {
            const float4 o = *reinterpret_cast<const float4*>(dx + r.at);
            r.v = make_float4(o.x + r.v.x, o.y + r.v.y, o.z + r.v.z, o.w + r.v.w);
        }
        return r;
    };
    auto store = [&](size_t, const Acc& r) { pool_store4(reinterpret_cast<float4*>(dx + r.at), r.v, q.nt); };
    nk_span_walk<2>((size_t)q.items, compute, store);
}

// ------------------------------------------------------------------------------------------------ plane class
// G lanes own a plane.  Lane l takes the elements (VEC: 16-byte groups) l, l + G, l + 2 G, ... in that order, then the G partial
// results are merged by a butterfly over lane distances G / 2 .. 1 (G = 256: per wave, then the four wave results in wave order).
template <int G, bool VEC, bool MAX>
__global__ __launch_bounds__(256) void pool_plane_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int* __restrict__ idx,
                                                             long long planes, int L) {
    constexpr int PER_BLOCK = 256 / G, W = G < 64 ? G : 64;
    __shared__ float sv[4];
    __shared__ int si[4];
    const int lane = threadIdx.x % G, group = threadIdx.x / G;
    for (long long p = (long long)blockIdx.x * PER_BLOCK + group; p < planes; p += (long long)gridDim.x * PER_BLOCK) {
        const float* xp = x + p * L;
        float acc = MAX ? -INFINITY : 0.f;
        int bi = INT_MAX;
        if (VEC) {
            const float4* x4 = reinterpret_cast<const float4*>(xp);
            const int n4 = L / 4;
#pragma unroll 4
            for (int t = lane; t < n4; t += G) {
                const float4 f = x4[t];
                const float fe[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (MAX) {
                        if (bi == INT_MAX || pool_takes(fe[e], acc)) { acc = fe[e]; bi = 4 * t + e; }
                    } else {
                        acc += fe[e];
                    }
                }
            }
        } else {
#pragma unroll 4
            for (int t = lane; t < L; t += G) {
                const float v = xp[t];
                if (MAX) {
                    if (bi == INT_MAX || pool_takes(v, acc)) { acc = v; bi = t; }
                } else {
                    acc += v;
                }
            }
        }
#pragma unroll
        for (int off = W / 2; off > 0; off >>= 1) {
            const float ov = __shfl_xor(acc, off, 64);
            if (MAX) {
                const int oi = __shfl_xor(bi, off, 64);
                pool_pair_merge(acc, bi, ov, oi);
            } else {
                acc += ov;
            }
        }
        if (G == 256) {  // p is the same for the whole block: every thread reaches the barriers
            __syncthreads();
            if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = acc; si[threadIdx.x >> 6] = bi; }
            __syncthreads();
            acc = sv[0]; bi = si[0];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                if (MAX) pool_pair_merge(acc, bi, sv[w], si[w]);
                else acc += sv[w];
            }
        }
        if (lane == 0) {
            y[p] = MAX ? acc : acc / (float)L;
            if (MAX && idx) idx[p] = bi;
        }
    }
}

template <bool MAX>
__global__ __launch_bounds__(256) void pool_plane_bwd_kernel(float* __restrict__ dx, const float* __restrict__ g, const int* __restrict__ idx,
                                                             long long n4, int L, int assign, int nt) {
    const int L4 = L / 4;
    const bool narrow = n4 < (1ll << 31);
    auto compute = [&](size_t i) {
        size_t plane;
        int off;
        if (narrow) {
            const unsigned pl = (unsigned)i / (unsigned)L4;
            plane = pl;
            off = 4 * (int)((unsigned)i - pl * (unsigned)L4);
        } else {
            plane = i / (size_t)L4;
            off = 4 * (int)(i - plane * (size_t)L4);
        }
        const float gv = g[plane];
        float4 v;
        if (MAX) {
            const int at = idx[plane] - off;
            v = make_float4(at == 0 ? gv : 0.f, at == 1 ? gv : 0.f, at == 2 ? gv : 0.f, at == 3 ? gv : 0.f);
        } else {
            const float a = gv / (float)L;
            v = make_float4(a, a, a, a);
        }
        if (!assign) {
            const float4 o = reinterpret_cast<const float4*>(dx)[i];
            v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
        }
        return v;
    };
    auto store = [&](size_t i, const float4& v) { pool_store4(reinterpret_cast<float4*>(dx) + i, v, nt); };
    nk_span_walk<2>((size_t)n4, compute, store);
}

// ------------------------------------------------------------------------------------------------ host side
inline bool pool_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// blocks of 256 threads for `items` thread-items: about eight per CU at most, the kernels walk the rest
inline int pool_grid(long long items) {
    long long b = (items + 255) / 256;
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return (int)b;
}

// The validity rules of the header, the one place they live.  y_shape (2 + nd entries) may be NULL.
int pool_geometry(const char* who, int nd, const int* x_shape, const int* kernel, const int* stride, const int* padding, PoolGeom* q,
                  int* y_shape) {
    NK_CHECK(nd >= 1 && nd <= 3, "%s: nd = %d (1, 2 or 3 spatial axes)", who, nd);
    NK_CHECK(x_shape && kernel && stride && padding, "null pointer in %s", who);
    NK_CHECK(x_shape[0] >= 0 && x_shape[1] >= 0, "%s: negative extent (N = %d, C = %d)", who, x_shape[0], x_shape[1]);
    PoolGeom t;
    for (int a = 0; a < 3; ++a) { t.in[a] = t.out[a] = t.k[a] = t.s[a] = 1; t.p[a] = 0; }
    long long in_plane = 1, out_plane = 1;
    for (int i = 0; i < nd; ++i) {
        const int a = 3 - nd + i, in = x_shape[2 + i], k = kernel[i], s = stride[i], p = padding[i];
        NK_CHECK(in >= 1, "%s: spatial extent %d of axis %d", who, in, i);
        NK_CHECK(k >= 1, "%s: window %d of axis %d (must be >= 1)", who, k, i);
        NK_CHECK(s >= 1, "%s: stride %d of axis %d (must be >= 1)", who, s, i);
        NK_CHECK(p >= 0 && p <= k / 2, "%s: padding %d of axis %d (must be in [0, window / 2] = [0, %d])", who, p, i, k / 2);
        const long long span = (long long)in + 2ll * p - k;
        NK_CHECK(span >= 0, "%s: window %d exceeds the padded extent %d + 2 * %d of axis %d: no output", who, k, in, p, i);
        const long long out = span / s + 1;
        t.in[a] = in; t.k[a] = k; t.s[a] = s; t.p[a] = p; t.out[a] = (int)out;
        in_plane *= in;
        out_plane *= out;
        NK_CHECK(in_plane <= INT_MAX && out_plane <= INT_MAX, "%s: a plane of more than 2^31 - 1 elements", who);
    }
    t.in_plane = (int)in_plane;
    t.out_plane = (int)out_plane;
    t.planes = (long long)x_shape[0] * x_shape[1];
    if (y_shape) {
        y_shape[0] = x_shape[0];
        y_shape[1] = x_shape[1];
        for (int i = 0; i < nd; ++i) y_shape[2 + i] = t.out[3 - nd + i];
    }
    if (q) *q = t;
    return NK_OK;
}

enum PoolClass { POOL_GENERIC, POOL_WINDOWED, POOL_PLANE };

bool pool_is_plane(const PoolGeom& q) {
    for (int a = 0; a < 3; ++a)
        if (q.out[a] != 1 || q.p[a] != 0 || q.k[a] != q.in[a]) return false;
    return true;
}
bool pool_is_windowed(const PoolGeom& q) {
    if (q.in[0] != 1 || q.k[0] != 1 || q.s[0] != 1 || q.p[0] != 0 || q.in[2] % 4 != 0) return false;
    const int k = q.k[2], s = q.s[2], p = q.p[2];
    return (k == 2 && s == 2 && p == 0) || (k == 3 && s == 2 && p <= 1) || (k == 3 && s == 1 && p <= 1);
}
// `aligned`: the pointers the class reads or writes in 16-byte pieces (forward: x; backward: dx)
PoolClass pool_class(const PoolGeom& q, bool aligned) {
    if (pool_is_plane(q)) return POOL_PLANE;
    return aligned && pool_is_windowed(q) ? POOL_WINDOWED : POOL_GENERIC;
}

#define POOL_WIN_CASES(X) X(2, 2, 0) X(3, 2, 0) X(3, 2, 1) X(3, 1, 0) X(3, 1, 1)

template <bool MAX>
int pool_fwd(nk_device* dev, const char* who, int nd, const float* x, const int* x_shape, float* y, int* idx, const int* kernel, const int* stride,
             const int* padding, int count_include_pad) {
    NK_USE(dev);
    PoolGeom q;
    if (int rc = pool_geometry(who, nd, x_shape, kernel, stride, padding, &q, nullptr)) return rc;
    NK_CHECK(x && y, "null pointer in %s", who);
    if (q.planes == 0) return NK_OK;
    const size_t bytes = ((size_t)q.planes * q.in_plane + (size_t)q.planes * q.out_plane * (MAX && idx ? 2 : 1)) * sizeof(float);
    const PoolClass cls = pool_class(q, pool_al16(x));
    if (cls == POOL_PLANE) {
        const int L = q.in_plane;
        const bool vec = L % 4 == 0 && pool_al16(x);
        const int G = L <= 128 ? 16 : (L <= 16384 ? 64 : 256);
        const int grid = (int)std::min<long long>((q.planes + 256 / G - 1) / (256 / G), 2048);
#define POOL_PLANE_LAUNCH(GG, VV) \
    hipLaunchKernelGGL((pool_plane_fwd_kernel<GG, VV, MAX>), dim3(grid), dim3(256), 0, dev->compute, x, y, idx, q.planes, L)
        if (G == 16) { if (vec) POOL_PLANE_LAUNCH(16, true); else POOL_PLANE_LAUNCH(16, false); }
        else if (G == 64) { if (vec) POOL_PLANE_LAUNCH(64, true); else POOL_PLANE_LAUNCH(64, false); }
        else { if (vec) POOL_PLANE_LAUNCH(256, true); else POOL_PLANE_LAUNCH(256, false); }
#undef POOL_PLANE_LAUNCH
    } else if (cls == POOL_WINDOWED) {
        PoolWin w{};
        w.IH = q.in[1]; w.IW = q.in[2]; w.OH = q.out[1]; w.OW = q.out[2];
        w.kh = q.k[1]; w.sh = q.s[1]; w.ph = q.p[1];
        w.groups = (w.OW + 3) / 4;
        w.items = q.planes * w.OH * w.groups;
        w.count_include_pad = count_include_pad;
        w.vector_store = w.OW % 4 == 0 && pool_al16(y) && (!idx || pool_al16(idx));
        w.nt = nk_streams_past_cache(bytes);
        const int grid = pool_grid(w.items);
#define X(K, S, P) \
    if (q.k[2] == K && q.s[2] == S && q.p[2] == P) \
        hipLaunchKernelGGL((pool_win_fwd_kernel<K, S, P, MAX>), dim3(grid), dim3(256), 0, dev->compute, x, y, idx, w);
        POOL_WIN_CASES(X)
#undef X
    } else {
        hipLaunchKernelGGL((pool_generic_fwd_kernel<MAX>), dim3(pool_grid(q.planes * q.out_plane)), dim3(256), 0, dev->compute, x, y, idx, q,
                           count_include_pad);
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}

template <bool MAX>
int pool_bwd(nk_device* dev, const char* who, int nd, float* dx, const int* x_shape, const float* g, const int* idx, const int* kernel,
             const int* stride, const int* padding, int count_include_pad, int assign) {
    NK_USE(dev);
    PoolGeom q;
    if (int rc = pool_geometry(who, nd, x_shape, kernel, stride, padding, &q, nullptr)) return rc;
    NK_CHECK(dx && g && (!MAX || idx), "null pointer in %s", who);
    if (q.planes == 0) return NK_OK;
    const size_t bytes = ((size_t)q.planes * q.in_plane * (assign ? 1 : 2) + (size_t)q.planes * q.out_plane * (MAX ? 2 : 1)) * sizeof(float);
    const int nt = nk_streams_past_cache(bytes);
    PoolClass cls = pool_class(q, pool_al16(dx));
    if (cls == POOL_PLANE && !(q.in_plane % 4 == 0 && pool_al16(dx))) cls = POOL_GENERIC;
    if (cls == POOL_PLANE) {
        const long long n4 = q.planes * (q.in_plane / 4);
        hipLaunchKernelGGL((pool_plane_bwd_kernel<MAX>), dim3(pool_grid(n4)), dim3(256), 0, dev->compute, dx, g, idx, n4, q.in_plane, assign, nt);
    } else if (cls == POOL_WINDOWED) {
        PoolWin w{};
        w.IH = q.in[1]; w.IW = q.in[2]; w.OH = q.out[1]; w.OW = q.out[2];
        w.kh = q.k[1]; w.sh = q.s[1]; w.ph = q.p[1];
        w.groups = w.IW / 4;
        w.items = q.planes * w.IH * w.groups;
        w.count_include_pad = count_include_pad;
        w.nt = nt;
        w.assign = assign;
        const int grid = pool_grid(w.items);
#define X(K, S, P) \
    if (q.k[2] == K && q.s[2] == S && q.p[2] == P) \
        hipLaunchKernelGGL((pool_win_bwd_kernel<K, S, P, MAX>), dim3(grid), dim3(256), 0, dev->compute, dx, g, idx, w);
        POOL_WIN_CASES(X)
#undef X
    } else {
        hipLaunchKernelGGL((pool_generic_bwd_kernel<MAX>), dim3(pool_grid(q.planes * q.in_plane)), dim3(256), 0, dev->compute, dx, g, idx, q,
                           count_include_pad, assign);
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_pool_out_shape(int nd, const int* x_shape, const int* kernel, const int* stride, const int* padding, int* y_shape) {
    NK_CHECK(y_shape, "null pointer in nk_pool_out_shape");
    return pool_geometry("nk_pool_out_shape", nd, x_shape, kernel, stride, padding, nullptr, y_shape);
}

int nk_max_pool_fwd(nk_device* dev, int nd, const float* x, const int* x_shape, float* y, int* idx, const int* kernel, const int* stride,
                    const int* padding) {
    return pool_fwd<true>(dev, "nk_max_pool_fwd", nd, x, x_shape, y, idx, kernel, stride, padding, 1);
}
int nk_max_pool_bwd(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g, const int* idx, const int* kernel, const int* stride,
                    const int* padding) {
    return pool_bwd<true>(dev, "nk_max_pool_bwd", nd, dx, x_shape, g, idx, kernel, stride, padding, 1, 0);
}
int nk_max_pool_bwd_assign(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g, const int* idx, const int* kernel,
                           const int* stride, const int* padding) {
    return pool_bwd<true>(dev, "nk_max_pool_bwd_assign", nd, dx, x_shape, g, idx, kernel, stride, padding, 1, 1);
}
int nk_avg_pool_fwd(nk_device* dev, int nd, const float* x, const int* x_shape, float* y, const int* kernel, const int* stride,
                    const int* padding, int count_include_pad) {
    return pool_fwd<false>(dev, "nk_avg_pool_fwd", nd, x, x_shape, y, nullptr, kernel, stride, padding, count_include_pad != 0);
}
int nk_avg_pool_bwd(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g, const int* kernel, const int* stride,
                    const int* padding, int count_include_pad) {
    return pool_bwd<false>(dev, "nk_avg_pool_bwd", nd, dx, x_shape, g, nullptr, kernel, stride, padding, count_include_pad != 0, 0);
}
int nk_avg_pool_bwd_assign(nk_device* dev, int nd, float* dx, const int* x_shape, const float* g, const int* kernel, const int* stride,
                           const int* padding, int count_include_pad) {
    return pool_bwd<false>(dev, "nk_avg_pool_bwd_assign", nd, dx, x_shape, g, nullptr, kernel, stride, padding, count_include_pad != 0, 1);
}

}  // extern "C"

// nn::Upsample: its kernels, host code and entry points (this unit's pool_al16 / pool_grid serve it)
#include "nk_upsample.h"
