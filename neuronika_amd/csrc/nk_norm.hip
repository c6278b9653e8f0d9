// Layer normalisation over the trailing extent of a contiguous row-major tensor read as (rows, D): HBM-bound row kernels in the
// style of the softmax rows of nk_reduce.hip - the row lives in registers between the passes, so x is read from memory once.
// The reference has no such layer; the semantics are fixed in include/neuronika_hip.h (biased variance as a SECOND pass over the
// centred values, all in f32).
//   forward / dx   D % 4 == 0, 16-byte aligned:  D <= 2048   one wave per row, V float4 per lane
//                                                D <= 16384  one 256-thread block per row, V float4 per thread, sums through LDS
//                  anything else (ragged D, unaligned pointers, longer rows): one block per row, scalar passes over memory
//   dgamma / dbeta one pass over g, x, stats: a block owns a tile of columns and a SPLIT of the rows and leaves one partial row
//                  pair in the workspace; a second kernel sums the splits in a fixed order.  No atomics: results repeat bit for bit.
#include "nk_common.h"
#include "nk_embedding.h"
#include "nk_cross_entropy.h"
#include "nk_activation.h"
#include "nk_optim_multi.h"
#include "nk_attention_decode.h"
#include "nk_attention_decode_paged.h"
#include "nk_attention_band.h"
#include "nk_repeat_kv.h"
#include "nk_rope.h"
#include "nk_sampling.h"

namespace {

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

constexpr int WAVE_MAX_D = 2048;    // V = 8 float4 per lane: forward 32 data VGPRs, dx with accumulation 96
constexpr int BLOCK_MAX_D = 16384;  // V = 16 float4 per thread of a 256-thread block
constexpr unsigned MAX_GRID = 1u << 20;  // blocks per launch; the kernels stride over the rows beyond it

__device__ __forceinline__ float sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float4 sub4(const float4& v, float m) { return make_float4(v.x - m, v.y - m, v.z - m, v.w - m); }

// Sum over the row's owner: a wave (xor-shuffles) or a 256-thread block (wave sums combined through LDS in wave order).  Result
// in every thread of the owner.
template <bool BLOCK>
__device__ __forceinline__ float owner_sum(float v, float* red) {
    v = nk_wave_sum(v);
    if (!BLOCK) return v;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wid] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// The V quads of a thread's row slice, ALL issued before any is used (nk_reduce.hip: row_load).  T threads own the row (64 or
// 256); threads beyond the row re-read its first quad and are masked by the `c < D` tests of the compute loops.
template <int V, int T>
__device__ __forceinline__ void quads_load(float4 (&v)[V], const float* __restrict__ row, int t, int D, bool stream) {
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int c = (i * T + t) * 4;
        v[i] = nk_load_stream(reinterpret_cast<const float4*>(row + (c < D ? c : 0)), stream);
    }
}

// mean, then the biased variance of the centred values (which replace v), then rstd
template <int V, int T>
__device__ __forceinline__ void row_stats(float4 (&v)[V], int t, int D, float eps, float* red, float* mean, float* rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i)
        if ((i * T + t) * 4 < D) s += sum4(v[i]);
    const float m = owner_sum<T == 256>(s, red) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i)
        if ((i * T + t) * 4 < D) {
            v[i] = sub4(v[i], m);
            q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
        }
    *mean = m;
    *rstd = 1.f / sqrtf(owner_sum<T == 256>(q, red) / (float)D + eps);
}

// BLOCK = false: blocks of four waves, a wave per row.  BLOCK = true: a 256-thread block per row.
template <int V, bool BLOCK>
__global__ __launch_bounds__(256) void layer_norm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ y,
                                                             float* __restrict__ stats, long long rows, int D, float eps) {
    constexpr int T = BLOCK ? 256 : 64;
    __shared__ float red[4];
    const int t = BLOCK ? threadIdx.x : threadIdx.x & 63;
    const long long first = BLOCK ? blockIdx.x : blockIdx.x * 4ll + (threadIdx.x >> 6), step = BLOCK ? gridDim.x : gridDim.x * 4ll;
    for (long long row = first; row < rows; row += step) {
        float4 v[V];
        quads_load<V, T>(v, x + row * D, t, D, false);
        float mean, rstd;
        row_stats<V, T>(v, t, D, eps, red, &mean, &rstd);
        if (stats && t == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
        float* yr = y + row * D;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = (i * T + t) * 4;
            if (c < D) {
                float4 o = make_float4(v[i].x * rstd, v[i].y * rstd, v[i].z * rstd, v[i].w * rstd);
                if (gamma) { const float4 w = *reinterpret_cast<const float4*>(gamma + c); o.x *= w.x; o.y *= w.y; o.z *= w.z; o.w *= w.w; }
                if (beta) { const float4 b = *reinterpret_cast<const float4*>(beta + c); o.x += b.x; o.y += b.y; o.z += b.z; o.w += b.w; }
                nk_store_stream(reinterpret_cast<float4*>(yr + c), o);
            }
        }
    }
}

// dx (+)= rstd * (gh - mean_D(gh) - xhat * mean_D(gh * xhat)),  gh = g * gamma,  xhat = (x - mean) * rstd as the forward formed it
// flags: bit 0 assign, bit 1 operands beyond the Infinity Cache (launch-time choice, nk_common.h)
template <int V, bool BLOCK>
__global__ __launch_bounds__(256) void layer_norm_bwd_kernel(int flags, float* __restrict__ dx, const float* __restrict__ g,
                                                             const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ stats, long long rows, int D) {
    constexpr int T = BLOCK ? 256 : 64;
    __shared__ float red[4];
    const int t = BLOCK ? threadIdx.x : threadIdx.x & 63;
    const long long first = BLOCK ? blockIdx.x : blockIdx.x * 4ll + (threadIdx.x >> 6), step = BLOCK ? gridDim.x : gridDim.x * 4ll;
    const bool assign = flags & 1, nt = flags & 2;
    for (long long row = first; row < rows; row += step) {
        float4 gv[V], xv[V], dv[V];
        quads_load<V, T>(gv, g + row * D, t, D, nt);
        quads_load<V, T>(xv, x + row * D, t, D, nt);
        if (!assign) quads_load<V, T>(dv, dx + row * D, t, D, nt);
        const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = (i * T + t) * 4;
            if (c < D) {
                if (gamma) { const float4 w = *reinterpret_cast<const float4*>(gamma + c); gv[i].x *= w.x; gv[i].y *= w.y; gv[i].z *= w.z; gv[i].w *= w.w; }
                xv[i] = sub4(xv[i], mean);
                xv[i].x *= rstd; xv[i].y *= rstd; xv[i].z *= rstd; xv[i].w *= rstd;
                s1 += sum4(gv[i]);
                s2 += (gv[i].x * xv[i].x + gv[i].y * xv[i].y) + (gv[i].z * xv[i].z + gv[i].w * xv[i].w);
            }
        }
        const float c1 = owner_sum<BLOCK>(s1, red) / (float)D, c2 = owner_sum<BLOCK>(s2, red) / (float)D;
        float* dr = dx + row * D;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = (i * T + t) * 4;
            if (c < D) {
                float4 d = make_float4(rstd * (gv[i].x - c1 - xv[i].x * c2), rstd * (gv[i].y - c1 - xv[i].y * c2),
                                       rstd * (gv[i].z - c1 - xv[i].z * c2), rstd * (gv[i].w - c1 - xv[i].w * c2));
                if (!assign) { d.x += dv[i].x; d.y += dv[i].y; d.z += dv[i].z; d.w += dv[i].w; }
                nk_store_stream(reinterpret_cast<float4*>(dr + c), d);
            }
        }
    }
}

// General kernels: any D, any alignment; a 256-thread block per row, scalar passes over memory (the row is re-read from cache).
__global__ __launch_bounds__(256) void layer_norm_fwd_general_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, float* __restrict__ y,
                                                                     float* __restrict__ stats, long long rows, int D, float eps) {
    __shared__ float red[4];
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* xr = x + row * D;
        float* yr = y + row * D;
        float s = 0.f;
        for (int c = threadIdx.x; c < D; c += 256) s += xr[c];
        const float mean = owner_sum<true>(s, red) / (float)D;
        float q = 0.f;
        for (int c = threadIdx.x; c < D; c += 256) { const float d = xr[c] - mean; q += d * d; }
        const float rstd = 1.f / sqrtf(owner_sum<true>(q, red) / (float)D + eps);
        if (stats && threadIdx.x == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
        for (int c = threadIdx.x; c < D; c += 256) {
            float o = (xr[c] - mean) * rstd;
            if (gamma) o *= gamma[c];
            if (beta) o += beta[c];
            yr[c] = o;
        }
    }
}

__global__ __launch_bounds__(256) void layer_norm_bwd_general_kernel(int assign, float* __restrict__ dx, const float* __restrict__ g,
                                                                     const float* __restrict__ x, const float* __restrict__ gamma,
                                                                     const float* __restrict__ stats, long long rows, int D) {
    __shared__ float red[4];
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* gr = g + row * D;
        const float* xr = x + row * D;
        float* dr = dx + row * D;
        const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
        float s1 = 0.f, s2 = 0.f;
        for (int c = threadIdx.x; c < D; c += 256) {
            const float gh = gamma ? gr[c] * gamma[c] : gr[c];
            s1 += gh;
            s2 += gh * ((xr[c] - mean) * rstd);
        }
        const float c1 = owner_sum<true>(s1, red) / (float)D, c2 = owner_sum<true>(s2, red) / (float)D;
        for (int c = threadIdx.x; c < D; c += 256) {
            const float gh = gamma ? gr[c] * gamma[c] : gr[c];
            const float d = rstd * (gh - c1 - (xr[c] - mean) * rstd * c2);
            dr[c] = assign ? d : dr[c] + d;
        }
    }
}

// ---- parameter gradients ------------------------------------------------------------------------------------------------------
// Stage 1: block (tile, split) owns the 64 * VEC columns of its tile and the rows [split * rpb, (split + 1) * rpb): wave w takes
// rows w, w + 4, ... of them, a lane VEC adjacent columns (a wave reads 1 KB of a row at VEC = 4), the loads of U rows in flight.
// The four waves' sums are added in wave order and stored as part[split][0 = dgamma, 1 = dbeta][D].
constexpr int PARAM_U = 4;
template <int VEC>
__global__ __launch_bounds__(256) void layer_norm_param_partial_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                       const float* __restrict__ stats, float* __restrict__ part,
                                                                       long long rows, int D, long long rpb, int nt) {
    __shared__ float sm[4][2][64 * VEC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * VEC;
    const bool on = col < D;  // VEC = 4 only with D % 4 == 0: a quad is inside the row or outside it
    const int cc = on ? col : 0;
    const long long r0 = blockIdx.y * rpb, r1 = r0 + rpb < rows ? r0 + rpb : rows;
    float dg[VEC], db[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) dg[k] = db[k] = 0.f;
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
    auto add = [&](const Ld& l, float mean, float rstd) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            dg[k] += l.g[k] * ((l.x[k] - mean) * rstd);
            db[k] += l.g[k];
        }
    };
    long long r = r0 + w;
    for (; r + 4 * (PARAM_U - 1) < r1; r += 4 * PARAM_U) {
        Ld l[PARAM_U];
        float mean[PARAM_U], rstd[PARAM_U];
#pragma unroll
        for (int u = 0; u < PARAM_U; ++u) {
            l[u] = load(r + 4 * u);
            mean[u] = stats[(r + 4 * u) * 2];
            rstd[u] = stats[(r + 4 * u) * 2 + 1];
        }
#pragma unroll
        for (int u = 0; u < PARAM_U; ++u) add(l[u], mean[u], rstd[u]);
    }
    for (; r < r1; r += 4) add(load(r), stats[r * 2], stats[r * 2 + 1]);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        sm[w][0][lane * VEC + k] = dg[k];
        sm[w][1][lane * VEC + k] = db[k];
    }
    __syncthreads();
    // 2 * 64 * VEC sums for 256 threads
    for (int i = threadIdx.x; i < 2 * 64 * VEC; i += 256) {
        const int which = i / (64 * VEC), j = i % (64 * VEC), c = blockIdx.x * 64 * VEC + j;
        if (c < D) part[((size_t)blockIdx.y * 2 + which) * D + c] = (sm[0][which][j] + sm[1][which][j]) + (sm[2][which][j] + sm[3][which][j]);
    }
}

// Stage 2: block (tile, which) sums the splits of 64 columns - wave w the splits [w * per, (w + 1) * per) in ascending order, the
// four waves' sums in wave order - and adds the total to the output or assigns it.
__global__ __launch_bounds__(256) void layer_norm_param_final_kernel(const float* __restrict__ part, float* __restrict__ dgamma,
                                                                     float* __restrict__ dbeta, int D, int splits, int assign) {
    __shared__ float sm[4][64];
    float* out = blockIdx.y ? dbeta : dgamma;
    if (!out) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = blockIdx.x * 64 + lane;
    const int per = (splits + 3) / 4, lo = w * per, hi = lo + per < splits ? lo + per : splits;
    float s = 0.f;
    if (col < D) {
        const float* p = part + (size_t)blockIdx.y * D + col;
#pragma unroll 8
        for (int i = lo; i < hi; ++i) s += p[(size_t)i * 2 * D];
    }
    sm[w][lane] = s;
    __syncthreads();
    if (w == 0 && col < D) {
        const float total = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
        out[col] = assign ? total : out[col] + total;
    }
}

unsigned row_grid(long long rows, int rows_per_block) {
    const long long b = (rows + rows_per_block - 1) / rows_per_block;
    return (unsigned)(b < (long long)MAX_GRID ? b : (long long)MAX_GRID);
}

int check_geometry(const char* who, long long rows, int D) {
    NK_CHECK(D > 0 && D <= (1 << 30), "%s: D = %d (the normalised extent must be in 1 .. 2^30)", who, D);
    NK_CHECK(rows >= 0, "%s: rows = %lld", who, rows);
    return NK_OK;
}

int layer_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, long long rows,
                   int D, int assign) {
    NK_USE(dev);
    if (int rc = check_geometry("nk_layer_norm_bwd", rows, D)) return rc;
    NK_CHECK(dx && g && x && stats, "null pointer in nk_layer_norm_bwd (only gamma may be NULL)");
    if (rows == 0) return NK_OK;
    const bool vec = D % 4 == 0 && D <= BLOCK_MAX_D && al16(dx) && al16(g) && al16(x) && (!gamma || al16(gamma));
    const int flags = assign | (nk_streams_past_cache((size_t)rows * D * (assign ? 12 : 16)) ? 2 : 0);
#define NK_LN_BWD(V, BLOCK) \
    hipLaunchKernelGGL((layer_norm_bwd_kernel<V, BLOCK>), dim3(row_grid(rows, BLOCK ? 1 : 4)), dim3(256), 0, dev->compute, flags, dx, g, x, gamma, stats, rows, D)
    if (!vec) hipLaunchKernelGGL(layer_norm_bwd_general_kernel, dim3(row_grid(rows, 1)), dim3(256), 0, dev->compute, assign, dx, g, x, gamma, stats, rows, D);
    else if (D <= 256) NK_LN_BWD(1, false);
    else if (D <= 512) NK_LN_BWD(2, false);
    else if (D <= 1024) NK_LN_BWD(4, false);
    else if (D <= WAVE_MAX_D) NK_LN_BWD(8, false);
    else if (D <= 4096) NK_LN_BWD(4, true);
    else if (D <= 8192) NK_LN_BWD(8, true);
    else NK_LN_BWD(16, true);
#undef NK_LN_BWD
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int layer_norm_bwd_params(nk_device* dev, float* dgamma, float* dbeta, const float* g, const float* x, const float* stats,
                          long long rows, int D, int assign) {
    NK_USE(dev);
    if (int rc = check_geometry("nk_layer_norm_bwd_params", rows, D)) return rc;
    NK_CHECK(dgamma || dbeta, "nk_layer_norm_bwd_params: dgamma and dbeta are both NULL");
    NK_CHECK(g && x && stats, "null pointer in nk_layer_norm_bwd_params");
    if (rows == 0) return NK_OK;
    const int vecw = (D % 4 == 0 && al16(g) && al16(x)) ? 4 : 1;
    const int tiles = (D + 64 * vecw - 1) / (64 * vecw);
    // rows per block: about 2048 blocks in all (eight per CU) and at least 16 rows each (one unrolled trip of every wave); a
    // function of (rows, D) alone, so the summation order - and the result's bits - do not depend on the device
    long long want = (2048 + tiles - 1) / tiles, rpb = (rows + want - 1) / want;
    rpb = rpb < 16 ? 16 : (rpb + 3) / 4 * 4;
    long long splits = (rows + rpb - 1) / rpb;
    if (splits > 65535) { rpb = ((rows + 65534) / 65535 + 3) / 4 * 4; splits = (rows + rpb - 1) / rpb; }
    void* ws = nullptr;
    if (int rc = nk_workspace(dev, (size_t)splits * 2 * D * sizeof(float), &ws)) return rc;
    const int nt = nk_streams_past_cache((size_t)rows * D * 8) ? 1 : 0;
    if (vecw == 4)
        hipLaunchKernelGGL((layer_norm_param_partial_kernel<4>), dim3(tiles, (unsigned)splits), dim3(256), 0, dev->compute, g, x, stats, (float*)ws, rows, D, rpb, nt);
    else
        hipLaunchKernelGGL((layer_norm_param_partial_kernel<1>), dim3(tiles, (unsigned)splits), dim3(256), 0, dev->compute, g, x, stats, (float*)ws, rows, D, rpb, nt);
    NK_LAUNCH_CHECK();
    hipLaunchKernelGGL(layer_norm_param_final_kernel, dim3((D + 63) / 64, 2), dim3(256), 0, dev->compute, (const float*)ws, dgamma, dbeta, D, (int)splits, assign);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

// ---- RMS normalisation ---------------------------------------------------------------------------------------------------------
// y = x * rstd * gamma with rstd = 1 / sqrt(sum(x * x) / D + eps): no centring, so ONE reduction forward and ONE backward where
// LayerNorm has two each, no mean in `stats` (rows floats: rstd alone) and no beta.  Same families and the same V per D bracket
// as the LayerNorm kernels above, chosen from D and alignment alone.
__device__ __forceinline__ float sq4(const float4& v) { return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }

template <int V, bool BLOCK>
__global__ __launch_bounds__(256) void rms_norm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           float* __restrict__ y, float* __restrict__ stats, long long rows, int D,
                                                           float eps) {
    constexpr int T = BLOCK ? 256 : 64;
    __shared__ float red[4];
    const int t = BLOCK ? threadIdx.x : threadIdx.x & 63;
    const long long first = BLOCK ? blockIdx.x : blockIdx.x * 4ll + (threadIdx.x >> 6), step = BLOCK ? gridDim.x : gridDim.x * 4ll;
    for (long long row = first; row < rows; row += step) {
        float4 v[V];
        quads_load<V, T>(v, x + row * D, t, D, false);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i)
            if ((i * T + t) * 4 < D) q += sq4(v[i]);
        const float rstd = 1.f / sqrtf(owner_sum<BLOCK>(q, red) / (float)D + eps);
        if (stats && t == 0) stats[row] = rstd;
        float* yr = y + row * D;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = (i * T + t) * 4;
            if (c < D) {
                float4 o = make_float4(v[i].x * rstd, v[i].y * rstd, v[i].z * rstd, v[i].w * rstd);
                if (gamma) { const float4 w = *reinterpret_cast<const float4*>(gamma + c); o.x *= w.x; o.y *= w.y; o.z *= w.z; o.w *= w.w; }
                nk_store_stream(reinterpret_cast<float4*>(yr + c), o);
            }
        }
    }
}

// dx (+)= rstd * (gh - xhat * mean_D(gh * xhat)),  gh = g * gamma,  xhat = x * rstd as the forward formed it
// flags: bit 0 assign, bit 1 operands beyond the Infinity Cache (launch-time choice, nk_common.h)
template <int V, bool BLOCK>
__global__ __launch_bounds__(256) void rms_norm_bwd_kernel(int flags, float* __restrict__ dx, const float* __restrict__ g,
                                                           const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ stats, long long rows, int D) {
    constexpr int T = BLOCK ? 256 : 64;
    __shared__ float red[4];
    const int t = BLOCK ? threadIdx.x : threadIdx.x & 63;
    const long long first = BLOCK ? blockIdx.x : blockIdx.x * 4ll + (threadIdx.x >> 6), step = BLOCK ? gridDim.x : gridDim.x * 4ll;
    const bool assign = flags & 1, nt = flags & 2;
    for (long long row = first; row < rows; row += step) {
        float4 gv[V], xv[V], dv[V];
        quads_load<V, T>(gv, g + row * D, t, D, nt);
        quads_load<V, T>(xv, x + row * D, t, D, nt);
        if (!assign) quads_load<V, T>(dv, dx + row * D, t, D, nt);
        const float rstd = stats[row];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = (i * T + t) * 4;
            if (c < D) {
                if (gamma) { const float4 w = *reinterpret_cast<const float4*>(gamma + c); gv[i].x *= w.x; gv[i].y *= w.y; gv[i].z *= w.z; gv[i].w *= w.w; }
                xv[i].x *= rstd; xv[i].y *= rstd; xv[i].z *= rstd; xv[i].w *= rstd;
                s += dot4(gv[i], xv[i]);
            }
        }
        const float cm = owner_sum<BLOCK>(s, red) / (float)D;
        float* dr = dx + row * D;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = (i * T + t) * 4;
            if (c < D) {
                float4 d = make_float4(rstd * (gv[i].x - xv[i].x * cm), rstd * (gv[i].y - xv[i].y * cm),
                                       rstd * (gv[i].z - xv[i].z * cm), rstd * (gv[i].w - xv[i].w * cm));
                if (!assign) { d.x += dv[i].x; d.y += dv[i].y; d.z += dv[i].z; d.w += dv[i].w; }
                nk_store_stream(reinterpret_cast<float4*>(dr + c), d);
            }
        }
    }
}

// General kernels: any D, any alignment; a 256-thread block per row, scalar passes over memory (the row is re-read from cache).
__global__ __launch_bounds__(256) void rms_norm_fwd_general_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                   float* __restrict__ y, float* __restrict__ stats, long long rows,
                                                                   int D, float eps) {
    __shared__ float red[4];
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* xr = x + row * D;
        float* yr = y + row * D;
        float q = 0.f;
        for (int c = threadIdx.x; c < D; c += 256) q += xr[c] * xr[c];
        const float rstd = 1.f / sqrtf(owner_sum<true>(q, red) / (float)D + eps);
        if (stats && threadIdx.x == 0) stats[row] = rstd;
        for (int c = threadIdx.x; c < D; c += 256) {
            float o = xr[c] * rstd;
            if (gamma) o *= gamma[c];
            yr[c] = o;
        }
    }
}

__global__ __launch_bounds__(256) void rms_norm_bwd_general_kernel(int assign, float* __restrict__ dx, const float* __restrict__ g,
                                                                   const float* __restrict__ x, const float* __restrict__ gamma,
                                                                   const float* __restrict__ stats, long long rows, int D) {
    __shared__ float red[4];
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* gr = g + row * D;
        const float* xr = x + row * D;
        float* dr = dx + row * D;
        const float rstd = stats[row];
        float s = 0.f;
        for (int c = threadIdx.x; c < D; c += 256) {
            const float gh = gamma ? gr[c] * gamma[c] : gr[c];
            s += gh * (xr[c] * rstd);
        }
        const float cm = owner_sum<true>(s, red) / (float)D;
        for (int c = threadIdx.x; c < D; c += 256) {
            const float gh = gamma ? gr[c] * gamma[c] : gr[c];
            const float d = rstd * (gh - xr[c] * rstd * cm);
            dr[c] = assign ? d : dr[c] + d;
        }
    }
}

// dgamma, stage 1: the tiling of layer_norm_param_partial_kernel with ONE sum per column: block (tile, split) owns 64 * VEC
// columns and the rows [split * rpb, (split + 1) * rpb), wave w rows w, w + 4, ... of them with the loads of U rows in flight; the
// four waves' sums are added in wave order and stored as part[split][D].
template <int VEC>
__global__ __launch_bounds__(256) void rms_norm_gamma_partial_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                     const float* __restrict__ stats, float* __restrict__ part,
                                                                     long long rows, int D, long long rpb, int nt) {
    __shared__ float sm[4][64 * VEC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * VEC;
    const bool on = col < D;  // VEC = 4 only with D % 4 == 0: a quad is inside the row or outside it
    const int cc = on ? col : 0;
    const long long r0 = blockIdx.y * rpb, r1 = r0 + rpb < rows ? r0 + rpb : rows;
    float dg[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) dg[k] = 0.f;
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
    auto add = [&](const Ld& l, float rstd) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) dg[k] += l.g[k] * (l.x[k] * rstd);
    };
    long long r = r0 + w;
    for (; r + 4 * (PARAM_U - 1) < r1; r += 4 * PARAM_U) {
        Ld l[PARAM_U];
        float rstd[PARAM_U];
#pragma unroll
        for (int u = 0; u < PARAM_U; ++u) {
            l[u] = load(r + 4 * u);
            rstd[u] = stats[r + 4 * u];
        }
#pragma unroll
        for (int u = 0; u < PARAM_U; ++u) add(l[u], rstd[u]);
    }
    for (; r < r1; r += 4) add(load(r), stats[r]);
#pragma unroll
    for (int k = 0; k < VEC; ++k) sm[w][lane * VEC + k] = dg[k];
    __syncthreads();
    for (int j = threadIdx.x; j < 64 * VEC; j += 256) {
        const int c = blockIdx.x * 64 * VEC + j;
        if (c < D) part[(size_t)blockIdx.y * D + c] = (sm[0][j] + sm[1][j]) + (sm[2][j] + sm[3][j]);
    }
}

// Stage 2: block `tile` sums the splits of 64 columns - wave w the splits [w * per, (w + 1) * per) in ascending order, the four
// waves' sums in wave order - and adds the total to dgamma or assigns it.
__global__ __launch_bounds__(256) void rms_norm_gamma_final_kernel(const float* __restrict__ part, float* __restrict__ dgamma, int D,
                                                                   int splits, int assign) {
    __shared__ float sm[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = blockIdx.x * 64 + lane;
    const int per = (splits + 3) / 4, lo = w * per, hi = lo + per < splits ? lo + per : splits;
    float s = 0.f;
    if (col < D) {
        const float* p = part + col;
#pragma unroll 8
        for (int i = lo; i < hi; ++i) s += p[(size_t)i * D];
    }
    sm[w][lane] = s;
    __syncthreads();
    if (w == 0 && col < D) {
        const float total = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
        dgamma[col] = assign ? total : dgamma[col] + total;
    }
}

int rms_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, long long rows,
                 int D, int assign) {
    NK_USE(dev);
    const char* who = assign ? "nk_rms_norm_bwd_assign" : "nk_rms_norm_bwd";
    if (int rc = check_geometry(who, rows, D)) return rc;
    NK_CHECK(dx && g && x && stats, "null pointer in %s (only gamma may be NULL)", who);
    if (rows == 0) return NK_OK;
    const bool vec = D % 4 == 0 && D <= BLOCK_MAX_D && al16(dx) && al16(g) && al16(x) && (!gamma || al16(gamma));
    const int flags = assign | (nk_streams_past_cache((size_t)rows * D * (assign ? 12 : 16)) ? 2 : 0);
#define NK_RMS_BWD(V, BLOCK) \
    hipLaunchKernelGGL((rms_norm_bwd_kernel<V, BLOCK>), dim3(row_grid(rows, BLOCK ? 1 : 4)), dim3(256), 0, dev->compute, flags, dx, g, x, gamma, stats, rows, D)
    if (!vec) hipLaunchKernelGGL(rms_norm_bwd_general_kernel, dim3(row_grid(rows, 1)), dim3(256), 0, dev->compute, assign, dx, g, x, gamma, stats, rows, D);
    else if (D <= 256) NK_RMS_BWD(1, false);
    else if (D <= 512) NK_RMS_BWD(2, false);
    else if (D <= 1024) NK_RMS_BWD(4, false);
    else if (D <= WAVE_MAX_D) NK_RMS_BWD(8, false);
    else if (D <= 4096) NK_RMS_BWD(4, true);
    else if (D <= 8192) NK_RMS_BWD(8, true);
    else NK_RMS_BWD(16, true);
#undef NK_RMS_BWD
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int rms_norm_bwd_gamma(nk_device* dev, float* dgamma, const float* g, const float* x, const float* stats, long long rows, int D,
                       int assign) {
    NK_USE(dev);
    const char* who = assign ? "nk_rms_norm_bwd_gamma_assign" : "nk_rms_norm_bwd_gamma";
    if (int rc = check_geometry(who, rows, D)) return rc;
    NK_CHECK(dgamma && g && x && stats, "null pointer in %s", who);
    if (rows == 0) return NK_OK;
    const int vecw = (D % 4 == 0 && al16(g) && al16(x)) ? 4 : 1;
    const int tiles = (D + 64 * vecw - 1) / (64 * vecw);
    // rows per block by the rule of layer_norm_bwd_params: a function of (rows, D) alone, so is the summation order
    long long want = (2048 + tiles - 1) / tiles, rpb = (rows + want - 1) / want;
    rpb = rpb < 16 ? 16 : (rpb + 3) / 4 * 4;
    long long splits = (rows + rpb - 1) / rpb;
    if (splits > 65535) { rpb = ((rows + 65534) / 65535 + 3) / 4 * 4; splits = (rows + rpb - 1) / rpb; }
    void* ws = nullptr;
    if (int rc = nk_workspace(dev, (size_t)splits * D * sizeof(float), &ws)) return rc;
    const int nt = nk_streams_past_cache((size_t)rows * D * 8) ? 1 : 0;
    if (vecw == 4)
        hipLaunchKernelGGL((rms_norm_gamma_partial_kernel<4>), dim3(tiles, (unsigned)splits), dim3(256), 0, dev->compute, g, x, stats, (float*)ws, rows, D, rpb, nt);
    else
        hipLaunchKernelGGL((rms_norm_gamma_partial_kernel<1>), dim3(tiles, (unsigned)splits), dim3(256), 0, dev->compute, g, x, stats, (float*)ws, rows, D, rpb, nt);
    NK_LAUNCH_CHECK();
    hipLaunchKernelGGL(rms_norm_gamma_final_kernel, dim3((D + 63) / 64), dim3(256), 0, dev->compute, (const float*)ws, dgamma, D, (int)splits, assign);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_layer_norm_fwd(nk_device* dev, const float* x, const float* gamma, const float* beta, float* y, float* stats, long long rows,
                      int D, double eps) {
    NK_USE(dev);
    if (int rc = check_geometry("nk_layer_norm_fwd", rows, D)) return rc;
    NK_CHECK(eps >= 0.0 && eps <= 3.0e38, "nk_layer_norm_fwd: eps = %g (must be finite and not negative)", eps);  // NaN fails both
    NK_CHECK(x && y, "null pointer in nk_layer_norm_fwd (gamma, beta and stats may be NULL)");
    if (rows == 0) return NK_OK;
    const bool vec = D % 4 == 0 && D <= BLOCK_MAX_D && al16(x) && al16(y) && (!gamma || al16(gamma)) && (!beta || al16(beta));
    const float e = (float)eps;
#define NK_LN_FWD(V, BLOCK) \
    hipLaunchKernelGGL((layer_norm_fwd_kernel<V, BLOCK>), dim3(row_grid(rows, BLOCK ? 1 : 4)), dim3(256), 0, dev->compute, x, gamma, beta, y, stats, rows, D, e)
    if (!vec) hipLaunchKernelGGL(layer_norm_fwd_general_kernel, dim3(row_grid(rows, 1)), dim3(256), 0, dev->compute, x, gamma, beta, y, stats, rows, D, e);
    else if (D <= 256) NK_LN_FWD(1, false);
    else if (D <= 512) NK_LN_FWD(2, false);
    else if (D <= 1024) NK_LN_FWD(4, false);
    else if (D <= WAVE_MAX_D) NK_LN_FWD(8, false);
    else if (D <= 4096) NK_LN_FWD(4, true);
    else if (D <= 8192) NK_LN_FWD(8, true);
    else NK_LN_FWD(16, true);
#undef NK_LN_FWD
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int nk_layer_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, long long rows,
                      int D) {
    return layer_norm_bwd(dev, dx, g, x, gamma, stats, rows, D, 0);
}
int nk_layer_norm_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats,
                             long long rows, int D) {
    return layer_norm_bwd(dev, dx, g, x, gamma, stats, rows, D, 1);
}
int nk_layer_norm_bwd_params(nk_device* dev, float* dgamma, float* dbeta, const float* g, const float* x, const float* stats,
                             long long rows, int D) {
    return layer_norm_bwd_params(dev, dgamma, dbeta, g, x, stats, rows, D, 0);
}
int nk_layer_norm_bwd_params_assign(nk_device* dev, float* dgamma, float* dbeta, const float* g, const float* x, const float* stats,
                                    long long rows, int D) {
    return layer_norm_bwd_params(dev, dgamma, dbeta, g, x, stats, rows, D, 1);
}

int nk_rms_norm_fwd(nk_device* dev, const float* x, const float* gamma, float* y, float* stats, long long rows, int D, double eps) {
    NK_USE(dev);
    if (int rc = check_geometry("nk_rms_norm_fwd", rows, D)) return rc;
    NK_CHECK(eps >= 0.0 && eps <= 3.0e38, "nk_rms_norm_fwd: eps = %g (must be finite and not negative)", eps);  // NaN fails both
    NK_CHECK(x && y, "null pointer in nk_rms_norm_fwd (gamma and stats may be NULL)");
    if (rows == 0) return NK_OK;
    const bool vec = D % 4 == 0 && D <= BLOCK_MAX_D && al16(x) && al16(y) && (!gamma || al16(gamma));
    const float e = (float)eps;
#define NK_RMS_FWD(V, BLOCK) \
    hipLaunchKernelGGL((rms_norm_fwd_kernel<V, BLOCK>), dim3(row_grid(rows, BLOCK ? 1 : 4)), dim3(256), 0, dev->compute, x, gamma, y, stats, rows, D, e)
    if (!vec) hipLaunchKernelGGL(rms_norm_fwd_general_kernel, dim3(row_grid(rows, 1)), dim3(256), 0, dev->compute, x, gamma, y, stats, rows, D, e);
    else if (D <= 256) NK_RMS_FWD(1, false);
    else if (D <= 512) NK_RMS_FWD(2, false);
    else if (D <= 1024) NK_RMS_FWD(4, false);
    else if (D <= WAVE_MAX_D) NK_RMS_FWD(8, false);
    else if (D <= 4096) NK_RMS_FWD(4, true);
    else if (D <= 8192) NK_RMS_FWD(8, true);
    else NK_RMS_FWD(16, true);
#undef NK_RMS_FWD
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int nk_rms_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, long long rows,
                    int D) {
    return rms_norm_bwd(dev, dx, g, x, gamma, stats, rows, D, 0);
}
int nk_rms_norm_bwd_assign(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats,
                           long long rows, int D) {
    return rms_norm_bwd(dev, dx, g, x, gamma, stats, rows, D, 1);
}
int nk_rms_norm_bwd_gamma(nk_device* dev, float* dgamma, const float* g, const float* x, const float* stats, long long rows, int D) {
    return rms_norm_bwd_gamma(dev, dgamma, g, x, stats, rows, D, 0);
}
int nk_rms_norm_bwd_gamma_assign(nk_device* dev, float* dgamma, const float* g, const float* x, const float* stats, long long rows,
                                 int D) {
    return rms_norm_bwd_gamma(dev, dgamma, g, x, stats, rows, D, 1);
}

}  // extern "C"
