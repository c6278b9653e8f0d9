// Multi-tensor optimizer launches (ours; semantics in include/neuronika_hip.h): the AdamW step, the global L2 norm of a list of
// gradients, and the scaling of that list by the clip coefficient.  Included by nk_norm.hip.
// All three kernels follow the plan of sgd_multi_kernel (nk_elementwise.hip):
//   walk       the launch walks the concatenation of its parameters in chunks of OPT_CHUNK elements, a chunk never straddles two
//              parameters; a block of 256 threads takes CONSECUTIVE chunks (nk_span_walk's order)
//   vector     a whole chunk whose pointers are 16-byte aligned is four trips of float4 accesses, every load issued before the first use
//   scalar     a ragged last chunk, or a parameter with a misaligned pointer, goes element by element through the SAME per-element
//              device function (adamw_one / sumsq_one / scale_one)
//   table      the parameter table is a by-value kernel argument of OPT_MULTI_MAX = 32 entries: the AdamW table is 1928 bytes of the
//              4096 a kernel's arguments may take (5 pointers + a length + a chunk prefix + 2 floats per entry).  A block finds its
//              parameter by binary search over the chunk prefix sums, and searches again only when a chunk leaves the parameter of the
//              chunk before it.  Longer lists are split into successive launches by the entry point.
// Every element is written by one thread; the norm has no atomics (one f64 partial per chunk at a GLOBAL chunk index, summed in a
// fixed order by one block): the bits are a function of the values and the lengths alone.
// Measured, MI355X, 1 GiB per tensor (benchmarks/adamw.py, profiles/r15_adamw.jsonl): AdamW 6.07 TB/s (0.925 of nk_copy's time per byte),
// with AMSGrad 5.92 (0.947).  The norm call (sum of squares + finalize) reads at 5.00 TB/s, 1.12 of the copy's time per byte: NOT shown to
// hide behind HBM.  The call is two kernels, and which of them holds the 12 % (the f64 convert + multiply-add and the per-chunk barrier,
// or the one-block finalize that adds 65536 partials one load at a time) has not been separated by a kernel trace.
#pragma once
#include <algorithm>
#include <cmath>

#include "nk_common.h"

namespace {

constexpr int OPT_MULTI_MAX = 32;
constexpr int OPT_CHUNK = 4096;
constexpr int OPT_TRIPS = OPT_CHUNK / (4 * 256);  // the launches use 256 threads
constexpr int OPT_FINALIZE_THREADS = 1024;

struct AdamwMulti {
    float* w[OPT_MULTI_MAX];
    const float* g[OPT_MULTI_MAX];
    float* m[OPT_MULTI_MAX];
    float* v[OPT_MULTI_MAX];
    float* vmax[OPT_MULTI_MAX];  // null: no AMSGrad maximum for this parameter
    size_t n[OPT_MULTI_MAX];
    unsigned first_chunk[OPT_MULTI_MAX + 1];  // prefix sums of ceil(n / OPT_CHUNK), strictly increasing (no empty entries)
    float sbc2[OPT_MULTI_MAX];                // sqrt(1 - beta2^step): the step number is per parameter
    float step_size[OPT_MULTI_MAX];           // lr / (1 - beta1^step)
    int count;
};
struct GradMulti {
    float* g[OPT_MULTI_MAX];
    size_t n[OPT_MULTI_MAX];
    unsigned first_chunk[OPT_MULTI_MAX + 1];
    int count;
};
static_assert(sizeof(AdamwMulti) + 64 <= 4096, "the AdamW table and its scalars must fit the kernel argument segment");

// the entry t with first_chunk[t] <= ch < first_chunk[t + 1]; `t` comes in as the entry of the chunk before
template <class Table>
__device__ __forceinline__ int opt_entry_of(const Table& a, unsigned ch, int t) {
    if (ch >= a.first_chunk[t] && ch < a.first_chunk[t + 1]) return t;
    int lo = 0, hi = a.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ch >= a.first_chunk[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void opt_store(float4* p, const float4& v, bool nt) {
    if (nt) nk_store_stream(p, v);
    else *p = v;
}

// ------------------------------------------------------------------------------------------------ AdamW
struct adamw_args {
    float keep;  // 1 - lr * weight_decay, formed on the host; 1 when weight_decay == 0 (then the product is skipped)
    float beta1, beta2, eps;
    bool decay;
};
// one element: decoupled decay, then the expression adam_kernel evaluates (adam/mod.rs:131-169, amsgrad/mod.rs:163-205).  No
// contraction: with it the compiler may fuse `w keep - q step_size` around either product, and chose differently in the vector and
// the scalar path (the 4096-element parameter differed from its offset twin in the last bit); every operation rounds on its own, as
// the NumPy restatement's do
__device__ __forceinline__ float adamw_one(float wi, float gi, float& m, float& v, float* vmax, const adamw_args& c, float sbc2,
                                           float step_size) {
#pragma clang fp contract(off)
    if (c.decay) wi = wi * c.keep;
    const float mi = m * c.beta1 + gi * (1.f - c.beta1);
    const float vi = v * c.beta2 + gi * gi * (1.f - c.beta2);
    m = mi; v = vi;
    float den = vi;
    if (vmax != nullptr) { den = fmaxf(*vmax, vi); *vmax = den; }
    return wi - mi / ((sqrtf(den) / sbc2) + c.eps) * step_size;
}

// nt: `nt` loads and stores (the launch's working set is beyond the Infinity Cache, nk_common.h)
__global__ __launch_bounds__(256) void adamw_multi_kernel(AdamwMulti a, adamw_args c, bool nt) {
    const unsigned total = a.first_chunk[a.count];
    const unsigned per = (total + gridDim.x - 1) / gridDim.x, c0 = blockIdx.x * per, c1 = c0 + per < total ? c0 + per : total;
    int t = 0;
    for (unsigned ch = c0; ch < c1; ++ch) {
        t = opt_entry_of(a, ch, t);
        float* __restrict__ w = a.w[t];
        const float* __restrict__ g = a.g[t];
        float* __restrict__ m = a.m[t];
        float* __restrict__ v = a.v[t];
        float* __restrict__ vmax = a.vmax[t];
        const float sbc2 = a.sbc2[t], step_size = a.step_size[t];
        const size_t n = a.n[t], base = (size_t)(ch - a.first_chunk[t]) * OPT_CHUNK;
        const size_t end = base + OPT_CHUNK < n ? base + OPT_CHUNK : n;
        const bool vec = ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                           reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(vmax)) & 15) == 0;
        if (vec && end - base == OPT_CHUNK) {
            float4 wv[OPT_TRIPS], gv[OPT_TRIPS], mv[OPT_TRIPS], vv[OPT_TRIPS], xv[OPT_TRIPS];
#pragma unroll
            for (int u = 0; u < OPT_TRIPS; ++u) {
                const size_t i = base + 4 * threadIdx.x + (size_t)u * 1024;
                wv[u] = nk_load_stream(reinterpret_cast<const float4*>(w + i), nt);
                gv[u] = nk_load_stream(reinterpret_cast<const float4*>(g + i), nt);
                mv[u] = nk_load_stream(reinterpret_cast<const float4*>(m + i), nt);
                vv[u] = nk_load_stream(reinterpret_cast<const float4*>(v + i), nt);
                xv[u] = vmax ? nk_load_stream(reinterpret_cast<const float4*>(vmax + i), nt) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < OPT_TRIPS; ++u) {
                const size_t i = base + 4 * threadIdx.x + (size_t)u * 1024;
                wv[u].x = adamw_one(wv[u].x, gv[u].x, mv[u].x, vv[u].x, vmax ? &xv[u].x : nullptr, c, sbc2, step_size);
                wv[u].y = adamw_one(wv[u].y, gv[u].y, mv[u].y, vv[u].y, vmax ? &xv[u].y : nullptr, c, sbc2, step_size);
                wv[u].z = adamw_one(wv[u].z, gv[u].z, mv[u].z, vv[u].z, vmax ? &xv[u].z : nullptr, c, sbc2, step_size);
                wv[u].w = adamw_one(wv[u].w, gv[u].w, mv[u].w, vv[u].w, vmax ? &xv[u].w : nullptr, c, sbc2, step_size);
                opt_store(reinterpret_cast<float4*>(m + i), mv[u], nt);
                opt_store(reinterpret_cast<float4*>(v + i), vv[u], nt);
                if (vmax) opt_store(reinterpret_cast<float4*>(vmax + i), xv[u], nt);
                opt_store(reinterpret_cast<float4*>(w + i), wv[u], nt);
            }
        } else {
            for (size_t i = base + threadIdx.x; i < end; i += 256) {
                float mi = m[i], vi = v[i];
                const float wi = adamw_one(w[i], g[i], mi, vi, vmax ? vmax + i : nullptr, c, sbc2, step_size);
                m[i] = mi; v[i] = vi;
                w[i] = wi;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ global L2 norm
// acc + x^2, the element widened to f64 first: one fused multiply-add, spelled out so that both paths below round alike
__device__ __forceinline__ double sumsq_one(double acc, float x) {
    const double d = (double)x;
    return __builtin_fma(d, d, acc);
}
__device__ __forceinline__ double opt_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// partial[chunk_base + ch] = the sum of squares of chunk ch, in f64.  Thread t of the block owns elements 4 t + 1024 u + j
// (u, j = 0 .. 3) of the chunk and adds them in that order, in the vector and in the scalar path alike; then the 64 lanes of a wave
// (butterfly), then the four waves in order.  Plain loads: the step kernel reads the same gradients next.
__global__ __launch_bounds__(256) void grad_sumsq_multi_kernel(GradMulti a, double* __restrict__ partial, unsigned chunk_base) {
    __shared__ double wave_part[2][256 / NK_WAVE];
    const unsigned total = a.first_chunk[a.count];
    const unsigned per = (total + gridDim.x - 1) / gridDim.x, c0 = blockIdx.x * per, c1 = c0 + per < total ? c0 + per : total;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int t = 0;
    for (unsigned ch = c0; ch < c1; ++ch) {
        t = opt_entry_of(a, ch, t);
        const float* __restrict__ g = a.g[t];
        const size_t n = a.n[t], base = (size_t)(ch - a.first_chunk[t]) * OPT_CHUNK;
        const size_t end = base + OPT_CHUNK < n ? base + OPT_CHUNK : n;
        double acc = 0.0;
        if ((reinterpret_cast<uintptr_t>(g) & 15) == 0 && end - base == OPT_CHUNK) {
            float4 gv[OPT_TRIPS];
#pragma unroll
            for (int u = 0; u < OPT_TRIPS; ++u) gv[u] = *reinterpret_cast<const float4*>(g + base + 4 * threadIdx.x + (size_t)u * 1024);
#pragma unroll
            for (int u = 0; u < OPT_TRIPS; ++u) {
                acc = sumsq_one(acc, gv[u].x); acc = sumsq_one(acc, gv[u].y);
                acc = sumsq_one(acc, gv[u].z); acc = sumsq_one(acc, gv[u].w);
            }
        } else {
#pragma unroll
            for (int u = 0; u < OPT_TRIPS; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const size_t i = base + 4 * threadIdx.x + (size_t)u * 1024 + j;
                    if (i < end) acc = sumsq_one(acc, g[i]);
                }
        }
        acc = opt_wave_sum(acc);
        // two LDS rows taken in turn: one barrier per chunk (a wave that writes row p again has passed the barrier of the chunk
        // between, which thread 0 reaches only after it has read row p)
        double* row = wave_part[ch & 1];
        if (lane == 0) row[wid] = acc;
        __syncthreads();
        if (threadIdx.x == 0) partial[chunk_base + ch] = ((row[0] + row[1]) + row[2]) + row[3];
    }
}

// one block: thread t adds partials t, t + 1024, ... in that order, then lanes, then waves; total_norm and the clip coefficient
__global__ __launch_bounds__(OPT_FINALIZE_THREADS) void grad_norm_finalize_kernel(const double* __restrict__ partial, unsigned total,
                                                                                   float max_norm, float* __restrict__ out) {
    __shared__ double wave_part[OPT_FINALIZE_THREADS / NK_WAVE];
    double acc = 0.0;
    for (unsigned k = threadIdx.x; k < total; k += OPT_FINALIZE_THREADS) acc += partial[k];
    acc = opt_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int i = 0; i < OPT_FINALIZE_THREADS / NK_WAVE; ++i) sum += wave_part[i];
        const float total_norm = (float)sqrt(sum);
        const float coef = max_norm / (total_norm + 1e-6f);
        out[0] = total_norm;
        out[1] = coef > 1.f ? 1.f : coef;  // a NaN norm gives a NaN coefficient, not 1
    }
}

// ------------------------------------------------------------------------------------------------ g *= coef
__device__ __forceinline__ float scale_one(float g, float coef) { return g * coef; }

// coef == 1: nothing to do (g * 1 is g bit for bit), the block returns before it touches memory
__global__ __launch_bounds__(256) void grad_scale_multi_kernel(GradMulti a, const float* __restrict__ coef_p, bool nt) {
    const float coef = *coef_p;
    if (coef == 1.f) return;
    const unsigned total = a.first_chunk[a.count];
    const unsigned per = (total + gridDim.x - 1) / gridDim.x, c0 = blockIdx.x * per, c1 = c0 + per < total ? c0 + per : total;
    int t = 0;
    for (unsigned ch = c0; ch < c1; ++ch) {
        t = opt_entry_of(a, ch, t);
        float* __restrict__ g = a.g[t];
        const size_t n = a.n[t], base = (size_t)(ch - a.first_chunk[t]) * OPT_CHUNK;
        const size_t end = base + OPT_CHUNK < n ? base + OPT_CHUNK : n;
        if ((reinterpret_cast<uintptr_t>(g) & 15) == 0 && end - base == OPT_CHUNK) {
            float4 gv[OPT_TRIPS];
#pragma unroll
            for (int u = 0; u < OPT_TRIPS; ++u)
                gv[u] = nk_load_stream(reinterpret_cast<const float4*>(g + base + 4 * threadIdx.x + (size_t)u * 1024), nt);
#pragma unroll
            for (int u = 0; u < OPT_TRIPS; ++u) {
                gv[u].x = scale_one(gv[u].x, coef); gv[u].y = scale_one(gv[u].y, coef);
                gv[u].z = scale_one(gv[u].z, coef); gv[u].w = scale_one(gv[u].w, coef);
                opt_store(reinterpret_cast<float4*>(g + base + 4 * threadIdx.x + (size_t)u * 1024), gv[u], nt);
            }
        } else {
            for (size_t i = base + threadIdx.x; i < end; i += 256) g[i] = scale_one(g[i], coef);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// Rust `f32::powi` for e >= 1: repeated squaring in f32, the loop of nk_elementwise.hip's file-static powi_f32 (nk_adam_step), which
// an inventoried unit keeps to itself; the two must stay in step for weight_decay = 0 to be the project's Adam
inline float opt_powi_f32(float b, int e) {
    float r = 1.f;
    for (int k = e; k; k >>= 1) {
        if (k & 1) r *= b;
        b *= b;
    }
    return r;
}

inline size_t opt_chunks(size_t n) { return (n + OPT_CHUNK - 1) / OPT_CHUNK; }

// The checks the two list entries share: non-empty entries have a pointer, no pointer appears twice, and the chunks of the whole
// list fit the 32-bit chunk index.  `total_chunks` receives their number.
template <class P>
int opt_check_list(const char* what, const char* name, int count, P const* ptr, const size_t* n, size_t* total_chunks) {
    std::vector<const void*> seen;
    size_t chunks = 0;
    for (int i = 0; i < count; ++i) {
        if (n[i] == 0) continue;
        NK_CHECK(ptr[i] != nullptr, "%s: %s[%d] is a null pointer", what, name, i);
        chunks += opt_chunks(n[i]);
        NK_CHECK(chunks < (size_t(1) << 31), "%s: the list is beyond the chunk index (2^31 chunks of %d elements)", what, OPT_CHUNK);
        seen.push_back(ptr[i]);
    }
    std::sort(seen.begin(), seen.end());
    NK_CHECK(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "%s: the same %s pointer appears twice in one call", what, name);
    *total_chunks = chunks;
    return NK_OK;
}

// The next (up to) OPT_MULTI_MAX non-empty entries from `i` on: their list indices in idx[], their chunk prefix sums in first_chunk[]
// (padded with the total); returns how many.
inline int opt_next_batch(int& i, int count, const size_t* n, int* idx, unsigned* first_chunk) {
    int c = 0;
    first_chunk[0] = 0;
    for (; i < count && c < OPT_MULTI_MAX; ++i) {
        if (n[i] == 0) continue;
        idx[c] = i;
        first_chunk[c + 1] = first_chunk[c] + (unsigned)opt_chunks(n[i]);
        ++c;
    }
    for (int k = c + 1; k <= OPT_MULTI_MAX; ++k) first_chunk[k] = first_chunk[c];
    return c;
}
inline unsigned opt_grid(unsigned total) { return total < 8192u ? total : 8192u; }

}  // namespace

extern "C" {

int nk_adamw_step_multi(nk_device* dev, int count, float* const* w, const float* const* grad, float* const* exp_avg,
                        float* const* exp_avg_sq, float* const* max_exp_avg_sq, const size_t* n, const int* step, float lr, float beta1,
                        float beta2, float eps, float weight_decay) {
    const char* what = "nk_adamw_step_multi";
    NK_USE(dev);
    NK_CHECK(count >= 0 && (count == 0 || (w && grad && exp_avg && exp_avg_sq && n && step)), "%s: null table", what);
    size_t total_chunks = 0, bytes = 0;
    if (int rc = opt_check_list(what, "w", count, w, n, &total_chunks)) return rc;
    for (int i = 0; i < count; ++i) {
        NK_CHECK(step[i] >= 1, "%s: step[%d] = %d, the step number is 1-based", what, i, step[i]);
        if (n[i] == 0) continue;
        NK_CHECK(grad[i] && exp_avg[i] && exp_avg_sq[i], "%s: null pointer in entry %d", what, i);
        bytes += n[i] * (max_exp_avg_sq && max_exp_avg_sq[i] ? 36 : 28);
    }
    if (total_chunks == 0) return NK_OK;
    if (int rc = nk_refuse_capture(dev, "nk_adamw_step_multi: the bias corrections 1 - beta^step",
                                   "issue this optimizer step outside the captured region"))
        return rc;
    adamw_args c;
    c.decay = weight_decay != 0.f;
    c.keep = c.decay ? 1.f - lr * weight_decay : 1.f;
    c.beta1 = beta1; c.beta2 = beta2; c.eps = eps;
    const bool nt = nk_streams_past_cache(bytes);
    for (int i = 0; i < count;) {
        AdamwMulti a{};
        int idx[OPT_MULTI_MAX];
        a.count = opt_next_batch(i, count, n, idx, a.first_chunk);
        if (a.count == 0) break;
        for (int k = 0; k < a.count; ++k) {
            const int j = idx[k];
            a.w[k] = w[j]; a.g[k] = grad[j]; a.m[k] = exp_avg[j]; a.v[k] = exp_avg_sq[j];
            a.vmax[k] = max_exp_avg_sq ? max_exp_avg_sq[j] : nullptr;
            a.n[k] = n[j];
            const float bc1 = 1.f - opt_powi_f32(beta1, step[j]), bc2 = 1.f - opt_powi_f32(beta2, step[j]);
            a.sbc2[k] = sqrtf(bc2);
            a.step_size[k] = lr / bc1;
        }
        hipLaunchKernelGGL(adamw_multi_kernel, dim3(opt_grid(a.first_chunk[a.count])), dim3(256), 0, dev->compute, a, c, nt);
        NK_LAUNCH_CHECK();
    }
    return NK_OK;
}

int nk_adamw_step(nk_device* dev, float* w, const float* grad, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, size_t n,
                  float lr, float beta1, float beta2, float eps, int step, float weight_decay) {
    return nk_adamw_step_multi(dev, 1, &w, &grad, &exp_avg, &exp_avg_sq, max_exp_avg_sq ? &max_exp_avg_sq : nullptr, &n, &step, lr, beta1,
                               beta2, eps, weight_decay);
}

int nk_clip_grad_norm_multi(nk_device* dev, int count, float* const* grad, const size_t* n, float max_norm, float* out) {
    const char* what = "nk_clip_grad_norm_multi";
    NK_USE(dev);
    NK_CHECK(count >= 0 && (count == 0 || (grad && n)), "%s: null table", what);
    NK_CHECK(out != nullptr, "%s: out is a null pointer", what);
    NK_CHECK(max_norm > 0.f, "%s: max_norm must be positive (+inf: measure only), got %g", what, (double)max_norm);
    size_t total_chunks = 0, elems = 0;
    if (int rc = opt_check_list(what, "grad", count, grad, n, &total_chunks)) return rc;
    for (int i = 0; i < count; ++i) elems += n[i];
    double* partial = nullptr;
    if (total_chunks != 0) {
        void* ws = nullptr;
        if (int rc = nk_workspace(dev, total_chunks * sizeof(double), &ws)) return rc;
        partial = static_cast<double*>(ws);
    }
    const bool scale = total_chunks != 0 && !std::isinf(max_norm);
    const bool nt = nk_streams_past_cache(elems * 8);  // the scale pass: one read, one write
    for (int pass = 0; pass < (scale ? 2 : 1); ++pass) {
        unsigned chunk_base = 0;
        for (int i = 0; i < count;) {
            GradMulti a{};
            int idx[OPT_MULTI_MAX];
            a.count = opt_next_batch(i, count, n, idx, a.first_chunk);
            if (a.count == 0) break;
            for (int k = 0; k < a.count; ++k) { a.g[k] = grad[idx[k]]; a.n[k] = n[idx[k]]; }
            const unsigned total = a.first_chunk[a.count];
            if (pass == 0) hipLaunchKernelGGL(grad_sumsq_multi_kernel, dim3(opt_grid(total)), dim3(256), 0, dev->compute, a, partial, chunk_base);
            else hipLaunchKernelGGL(grad_scale_multi_kernel, dim3(opt_grid(total)), dim3(256), 0, dev->compute, a, out + 1, nt);
            NK_LAUNCH_CHECK();
            chunk_base += total;
        }
        if (pass == 0) {  // no partials: sqrt(0) = 0 and max_norm / 1e-6 > 1, so out = {0, 1}
            hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(OPT_FINALIZE_THREADS), 0, dev->compute, partial,
                               (unsigned)total_chunks, max_norm, out);
            NK_LAUNCH_CHECK();
        }
    }
    return NK_OK;
}

}  // extern "C"
