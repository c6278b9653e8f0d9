// Row normalisation over the trailing extent of a contiguous row-major tensor read as (rows, D) - LayerNorm and RMSNorm, ONE family:
// HBM-bound row kernels in the style of the softmax rows of nk_reduce.hip - the row lives in registers between the passes, so x is
// read from memory once.  The reference has no such layers; the semantics are fixed in include/neuronika_hip.h, all in f32:
//   LayerNorm  mean, then the biased variance as a SECOND pass over the centred values; gamma and beta; stats = {mean, rstd} per row
//   RMSNorm    rstd = 1 / sqrt(sum(x * x) / D + eps): no centring, so ONE reduction forward and ONE backward where LayerNorm has
//              two each; gamma alone; stats = rstd per row
//   forward / dx   D % 4 == 0, 16-byte aligned:  D <= 2048   one wave per row, V float4 per lane
//                                                D <= 16384  one 256-thread block per row, V float4 per thread, sums through LDS
//                  anything else (ragged D, unaligned pointers, longer rows): one block per row, scalar passes over memory
//   dgamma / dbeta one pass over g, x, stats: a block owns a tile of columns and a SPLIT of the rows and leaves one partial row
//                  (pair) in the workspace; a second kernel sums the splits in a fixed order.  No atomics: results repeat bit for bit.
// Each of the six kernel families is stated once, in a nk_norm_*_body.h that the LayerNorm and the RMSNorm kernel include inside
// their signatures under the switch NORM_CENTRED (1 = LayerNorm, 0 = RMSNorm); `#if NORM_CENTRED` stands only around what a mean
// or a beta brings.  The bodies are text and not force-inlined function templates because the latter moved the register allocation
// of 35 of the 38 kernels; included text left every instruction stream as it was (profiles/norm_rows_isa_identity.md).
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

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }  // true of a null pointer: an absent operand passes

constexpr int WAVE_MAX_D = 2048;    // V = 8 float4 per lane: forward 32 data VGPRs, dx with accumulation 96
constexpr int BLOCK_MAX_D = 16384;  // V = 16 float4 per thread of a 256-thread block
constexpr unsigned MAX_GRID = 1u << 20;  // blocks per launch; the kernels stride over the rows beyond it

__device__ __forceinline__ float sum4(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float4 sub4(const float4& v, float m) { return make_float4(v.x - m, v.y - m, v.z - m, v.w - m); }
__device__ __forceinline__ float sq4(const float4& v) { return (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w); }
__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }

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
            q += sq4(v[i]);
        }
    *mean = m;
    *rstd = 1.f / sqrtf(owner_sum<T == 256>(q, red) / (float)D + eps);
}

// ---- forward and dx, the row in registers (nk_norm_fwd_body.h, nk_norm_dx_body.h) ---------------------------------------------
template <int V, bool BLOCK>
__global__ __launch_bounds__(256) void layer_norm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ y,
                                                             float* __restrict__ stats, long long rows, int D, float eps) {
#define NORM_CENTRED 1
#include "nk_norm_fwd_body.h"
#undef NORM_CENTRED
}

template <int V, bool BLOCK>
__global__ __launch_bounds__(256) void rms_norm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           float* __restrict__ y, float* __restrict__ stats, long long rows, int D,
                                                           float eps) {
#define NORM_CENTRED 0
#include "nk_norm_fwd_body.h"
#undef NORM_CENTRED
}

template <int V, bool BLOCK>
__global__ __launch_bounds__(256) void layer_norm_bwd_kernel(int flags, float* __restrict__ dx, const float* __restrict__ g,
                                                             const float* __restrict__ x, const float* __restrict__ gamma,
                                                             const float* __restrict__ stats, long long rows, int D) {
#define NORM_CENTRED 1
#include "nk_norm_dx_body.h"
#undef NORM_CENTRED
}

template <int V, bool BLOCK>
__global__ __launch_bounds__(256) void rms_norm_bwd_kernel(int flags, float* __restrict__ dx, const float* __restrict__ g,
                                                           const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ stats, long long rows, int D) {
#define NORM_CENTRED 0
#include "nk_norm_dx_body.h"
#undef NORM_CENTRED
}

// ---- forward and dx, general (nk_norm_fwd_general_body.h, nk_norm_dx_general_body.h) -------------------------------------------
__global__ __launch_bounds__(256) void layer_norm_fwd_general_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, float* __restrict__ y,
                                                                     float* __restrict__ stats, long long rows, int D, float eps) {
#define NORM_CENTRED 1
#include "nk_norm_fwd_general_body.h"
#undef NORM_CENTRED
}

__global__ __launch_bounds__(256) void rms_norm_fwd_general_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                   float* __restrict__ y, float* __restrict__ stats, long long rows,
                                                                   int D, float eps) {
#define NORM_CENTRED 0
#include "nk_norm_fwd_general_body.h"
#undef NORM_CENTRED
}

__global__ __launch_bounds__(256) void layer_norm_bwd_general_kernel(int assign, float* __restrict__ dx, const float* __restrict__ g,
                                                                     const float* __restrict__ x, const float* __restrict__ gamma,
                                                                     const float* __restrict__ stats, long long rows, int D) {
#define NORM_CENTRED 1
#include "nk_norm_dx_general_body.h"
#undef NORM_CENTRED
}

__global__ __launch_bounds__(256) void rms_norm_bwd_general_kernel(int assign, float* __restrict__ dx, const float* __restrict__ g,
                                                                   const float* __restrict__ x, const float* __restrict__ gamma,
                                                                   const float* __restrict__ stats, long long rows, int D) {
#define NORM_CENTRED 0
#include "nk_norm_dx_general_body.h"
#undef NORM_CENTRED
}

// ---- parameter gradients (nk_norm_param_partial_body.h, nk_norm_param_final_body.h) --------------------------------------------
constexpr int PARAM_U = 4;
template <int VEC>
__global__ __launch_bounds__(256) void layer_norm_param_partial_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                       const float* __restrict__ stats, float* __restrict__ part,
                                                                       long long rows, int D, long long rpb, int nt) {
#define NORM_CENTRED 1
#include "nk_norm_param_partial_body.h"
#undef NORM_CENTRED
}

template <int VEC>
__global__ __launch_bounds__(256) void rms_norm_gamma_partial_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                     const float* __restrict__ stats, float* __restrict__ part,
                                                                     long long rows, int D, long long rpb, int nt) {
#define NORM_CENTRED 0
#include "nk_norm_param_partial_body.h"
#undef NORM_CENTRED
}

__global__ __launch_bounds__(256) void layer_norm_param_final_kernel(const float* __restrict__ part, float* __restrict__ dgamma,
                                                                     float* __restrict__ dbeta, int D, int splits, int assign) {
#define NORM_CENTRED 1
#include "nk_norm_param_final_body.h"
#undef NORM_CENTRED
}

__global__ __launch_bounds__(256) void rms_norm_gamma_final_kernel(const float* __restrict__ part, float* __restrict__ dgamma, int D,
                                                                   int splits, int assign) {
#define NORM_CENTRED 0
#include "nk_norm_param_final_body.h"
#undef NORM_CENTRED
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
unsigned row_grid(long long rows, int rows_per_block) {
    const long long b = (rows + rows_per_block - 1) / rows_per_block;
    return (unsigned)(b < (long long)MAX_GRID ? b : (long long)MAX_GRID);
}

int check_geometry(const char* who, long long rows, int D) {
    NK_CHECK(D > 0 && D <= (1 << 30), "%s: D = %d (the normalised extent must be in 1 .. 2^30)", who, D);
    NK_CHECK(rows >= 0, "%s: rows = %lld", who, rows);
    return NK_OK;
}

// Whether the row-in-registers kernels can take the call: quads, a row within a block's registers, every operand 16-byte aligned
bool rows_in_registers(int D, std::initializer_list<const void*> operands) {
    bool ok = D % 4 == 0 && D <= BLOCK_MAX_D;
    for (const void* p : operands) ok = ok && al16(p);
    return ok;
}

// The one dispatch ladder of forward and dx, from `vec`, `rows`, `D` and `dev` of the caller: the general kernel, or V float4 per
// lane of a wave (four rows a block), or V float4 per thread of a block.  Both kernels take the same argument list.
#define NK_NORM_ROWS(KERNEL, V, BLOCK, ...) \
    hipLaunchKernelGGL((KERNEL<V, BLOCK>), dim3(row_grid(rows, BLOCK ? 1 : 4)), dim3(256), 0, dev->compute, __VA_ARGS__)
#define NK_NORM_LADDER(KERNEL, GENERAL, ...)                                                                                  \
    do {                                                                                                                      \
        if (!vec) hipLaunchKernelGGL(GENERAL, dim3(row_grid(rows, 1)), dim3(256), 0, dev->compute, __VA_ARGS__);              \
        else if (D <= 256) NK_NORM_ROWS(KERNEL, 1, false, __VA_ARGS__);                                                       \
        else if (D <= 512) NK_NORM_ROWS(KERNEL, 2, false, __VA_ARGS__);                                                       \
        else if (D <= 1024) NK_NORM_ROWS(KERNEL, 4, false, __VA_ARGS__);                                                      \
        else if (D <= WAVE_MAX_D) NK_NORM_ROWS(KERNEL, 8, false, __VA_ARGS__);                                                \
        else if (D <= 4096) NK_NORM_ROWS(KERNEL, 4, true, __VA_ARGS__);                                                       \
        else if (D <= 8192) NK_NORM_ROWS(KERNEL, 8, true, __VA_ARGS__);                                                       \
        else NK_NORM_ROWS(KERNEL, 16, true, __VA_ARGS__);                                                                     \
    } while (0)

// dx's leading argument: the general kernel's `assign`, and for the row-in-registers kernels also their streaming bit
int dx_flags(bool vec, long long rows, int D, int assign) {
    return assign | (vec && nk_streams_past_cache((size_t)rows * D * (assign ? 12 : 16)) ? 2 : 0);
}

// The row split of the parameter gradients: about 2048 blocks in all (eight per CU) and at least 16 rows each (one unrolled trip of
// every wave), at most 65535 splits (gridDim.y).  A function of (rows, D) and the alignment alone, so the summation order - and the
// result's bits - do not depend on the device, and one rule for both norms.
struct ParamPlan { int vecw, tiles; long long rpb, splits; int nt; };
ParamPlan param_plan(const float* g, const float* x, long long rows, int D) {
    ParamPlan p;
    p.vecw = (D % 4 == 0 && al16(g) && al16(x)) ? 4 : 1;
    p.tiles = (D + 64 * p.vecw - 1) / (64 * p.vecw);
    const long long want = (2048 + p.tiles - 1) / p.tiles;
    p.rpb = (rows + want - 1) / want;
    p.rpb = p.rpb < 16 ? 16 : (p.rpb + 3) / 4 * 4;
    p.splits = (rows + p.rpb - 1) / p.rpb;
    if (p.splits > 65535) { p.rpb = ((rows + 65534) / 65535 + 3) / 4 * 4; p.splits = (rows + p.rpb - 1) / p.rpb; }
    p.nt = nk_streams_past_cache((size_t)rows * D * 8) ? 1 : 0;
    return p;
}

int layer_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, long long rows,
                   int D, int assign) {
    NK_USE(dev);
    if (int rc = check_geometry("nk_layer_norm_bwd", rows, D)) return rc;
    NK_CHECK(dx && g && x && stats, "null pointer in nk_layer_norm_bwd (only gamma may be NULL)");
    if (rows == 0) return NK_OK;
    const bool vec = rows_in_registers(D, {dx, g, x, gamma});
    NK_NORM_LADDER(layer_norm_bwd_kernel, layer_norm_bwd_general_kernel, dx_flags(vec, rows, D, assign), dx, g, x, gamma, stats, rows, D);
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
    const ParamPlan p = param_plan(g, x, rows, D);
    void* ws = nullptr;
    if (int rc = nk_workspace(dev, (size_t)p.splits * 2 * D * sizeof(float), &ws)) return rc;
    if (p.vecw == 4)
        hipLaunchKernelGGL((layer_norm_param_partial_kernel<4>), dim3(p.tiles, (unsigned)p.splits), dim3(256), 0, dev->compute, g, x, stats, (float*)ws, rows, D, p.rpb, p.nt);
    else
        hipLaunchKernelGGL((layer_norm_param_partial_kernel<1>), dim3(p.tiles, (unsigned)p.splits), dim3(256), 0, dev->compute, g, x, stats, (float*)ws, rows, D, p.rpb, p.nt);
    NK_LAUNCH_CHECK();
    hipLaunchKernelGGL(layer_norm_param_final_kernel, dim3((D + 63) / 64, 2), dim3(256), 0, dev->compute, (const float*)ws, dgamma, dbeta, D, (int)p.splits, assign);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int rms_norm_bwd(nk_device* dev, float* dx, const float* g, const float* x, const float* gamma, const float* stats, long long rows,
                 int D, int assign) {
    NK_USE(dev);
    const char* who = assign ? "nk_rms_norm_bwd_assign" : "nk_rms_norm_bwd";
    if (int rc = check_geometry(who, rows, D)) return rc;
    NK_CHECK(dx && g && x && stats, "null pointer in %s (only gamma may be NULL)", who);
    if (rows == 0) return NK_OK;
    const bool vec = rows_in_registers(D, {dx, g, x, gamma});
    NK_NORM_LADDER(rms_norm_bwd_kernel, rms_norm_bwd_general_kernel, dx_flags(vec, rows, D, assign), dx, g, x, gamma, stats, rows, D);
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
    const ParamPlan p = param_plan(g, x, rows, D);
    void* ws = nullptr;
    if (int rc = nk_workspace(dev, (size_t)p.splits * D * sizeof(float), &ws)) return rc;
    if (p.vecw == 4)
        hipLaunchKernelGGL((rms_norm_gamma_partial_kernel<4>), dim3(p.tiles, (unsigned)p.splits), dim3(256), 0, dev->compute, g, x, stats, (float*)ws, rows, D, p.rpb, p.nt);
    else
        hipLaunchKernelGGL((rms_norm_gamma_partial_kernel<1>), dim3(p.tiles, (unsigned)p.splits), dim3(256), 0, dev->compute, g, x, stats, (float*)ws, rows, D, p.rpb, p.nt);
    NK_LAUNCH_CHECK();
    hipLaunchKernelGGL(rms_norm_gamma_final_kernel, dim3((D + 63) / 64), dim3(256), 0, dev->compute, (const float*)ws, dgamma, D, (int)p.splits, assign);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // namespace

#include "nk_group_norm.h"  // GroupNorm / InstanceNorm: its kernels and entry points, built on the helpers above
#include "nk_quant_linear.h"  // weight-only int8 / int4 Linear: pack, unpack, the decode rows kernels and their entry points

extern "C" {

int nk_layer_norm_fwd(nk_device* dev, const float* x, const float* gamma, const float* beta, float* y, float* stats, long long rows,
                      int D, double eps) {
    NK_USE(dev);
    if (int rc = check_geometry("nk_layer_norm_fwd", rows, D)) return rc;
    NK_CHECK(eps >= 0.0 && eps <= 3.0e38, "nk_layer_norm_fwd: eps = %g (must be finite and not negative)", eps);  // NaN fails both
    NK_CHECK(x && y, "null pointer in nk_layer_norm_fwd (gamma, beta and stats may be NULL)");
    if (rows == 0) return NK_OK;
    const bool vec = rows_in_registers(D, {x, y, gamma, beta});
    NK_NORM_LADDER(layer_norm_fwd_kernel, layer_norm_fwd_general_kernel, x, gamma, beta, y, stats, rows, D, (float)eps);
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
    const bool vec = rows_in_registers(D, {x, y, gamma});
    NK_NORM_LADDER(rms_norm_fwd_kernel, rms_norm_fwd_general_kernel, x, gamma, y, stats, rows, D, (float)eps);
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
