// Smooth and gated activations (ours; semantics in include/neuronika_hip.h): GELU (erfc form), GELU (tanh form), SiLU, sigmoid, and
// the gated form y[r, j] = x[r, j] * act(x[r, H + j]) over the two halves of the last axis (GLU, GeGLU, SwiGLU).  Each is ONE streaming
// pass forward and ONE backward; the backward keeps the INPUT and recomputes from it.  Included by nk_norm.hip.
//   pointwise  the house streaming shape (nk_common.h): nk_span_walk over 16-byte groups, the loads of four trips in flight, `nt`
//              stores, `nt` loads in the backward passes whose working set is beyond the Infinity Cache; a scalar tail of n % 4
//   gated      H % 4 == 0: both halves of every row start on a 16-byte boundary, so the walk is over (row, j / 4) - consecutive lanes
//              take consecutive groups of the `a` half and the groups H / 4 further on of the `b` half: two coalesced streams per
//              wave, whatever the span boundary.  Any other H: a scalar kernel over (row, j), correct for every H.
// The activation is a template parameter.  Every element is written by one thread, no LDS: the bits are a function of the arguments and
// the data.
// Range: every formula is arranged so that a finite input gives finite results, forward and backward, without an inf * 0:
//   sigmoid family  e = exp(-|v|) in [0, 1], r = 1 / (1 + e): sigma(v) = r or e r by the sign of v, sigma (1 - sigma) = e r^2 -
//                   nothing overflows and neither tail cancels (SiLU: v = x; tanh-GELU: 0.5 (1 + tanh u) = sigma(2 u))
//   tanh-GELU       x^3 may overflow to +-inf, which sigma takes; x^2 in the derivative's polynomial is clamped at ACT_X2_MAX, beyond
//                   which sigma (1 - sigma) is exactly 0 in f32
//   GELU            Phi(x) = 0.5 erfc(-x / sqrt 2) keeps the negative tail; x^2 may overflow inside exp(-x^2 / 2), giving 0
#pragma once
#include "nk_common.h"

namespace {

constexpr float ACT_SQRT1_2 = 0.70710678118654752440f;     // 1 / sqrt(2)
constexpr float ACT_INV_SQRT_2PI = 0.39894228040143267794f;
constexpr float ACT_2K = 1.59576912160573071176f;          // 2 sqrt(2 / pi)
constexpr float ACT_C = 0.044715f;
constexpr float ACT_X2_MAX = 1.0e4f;                       // |x| = 100: 2 u = 7.1e4, exp(-2 u) = 0
constexpr long long GLU_MAX_ELEMS = 0x7fffffffLL;          // rows * 2 H: the gated kernels index with 32 bits

struct act_vd {
    float v, d;  // act(x), act'(x)
};

// x * sigma(v) and its derivative sigma + x sigma (1 - sigma) dv, or (PLAIN) sigma(v) and sigma (1 - sigma) dv
template <bool PLAIN>
__device__ __forceinline__ act_vd act_sigma(float x, float v, float dv) {
    const float e = expf(-fabsf(v));
    const float r = __builtin_amdgcn_rcpf(1.f + e);        // 1 + e in [1, 2]
    const float s = v >= 0.f ? r : e * r;
    const float q = e * r * r * dv;                        // sigma (1 - sigma) dv
    act_vd o;
    o.v = PLAIN ? s : x * s;                               // a NaN v reaches s through e
    o.d = PLAIN ? q : s + x * q;
    return o;
}

template <int ACT>
__device__ __forceinline__ float act_value(float x) {
    if (ACT == NK_ACT_GELU) return x * (0.5f * erfcf(-x * ACT_SQRT1_2));
    if (ACT == NK_ACT_GELU_TANH) return act_sigma<false>(x, ACT_2K * (x + ACT_C * (x * x * x)), 0.f).v;
    if (ACT == NK_ACT_SILU) return act_sigma<false>(x, x, 0.f).v;
    return act_sigma<true>(x, x, 0.f).v;
}
template <int ACT>
__device__ __forceinline__ act_vd act_both(float x) {
    if (ACT == NK_ACT_GELU) {
        const float phi = 0.5f * erfcf(-x * ACT_SQRT1_2);
        act_vd o;
        o.v = x * phi;
        o.d = phi + x * (ACT_INV_SQRT_2PI * expf(-0.5f * (x * x)));
        return o;
    }
    if (ACT == NK_ACT_GELU_TANH)
        return act_sigma<false>(x, ACT_2K * (x + ACT_C * (x * x * x)), ACT_2K * (1.f + 3.f * ACT_C * fminf(x * x, ACT_X2_MAX)));
    if (ACT == NK_ACT_SILU) return act_sigma<false>(x, x, 1.f);
    return act_sigma<true>(x, x, 1.f);
}
template <int ACT>
__device__ __forceinline__ float act_deriv(float x) { return act_both<ACT>(x).d; }

template <int ACT>
__device__ __forceinline__ float4 act_value4(const float4& x) {
    return make_float4(act_value<ACT>(x.x), act_value<ACT>(x.y), act_value<ACT>(x.z), act_value<ACT>(x.w));
}

// ------------------------------------------------------------------------------------------------ pointwise
template <int ACT>
__global__ __launch_bounds__(256) void activation_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n) {
    const size_t n4 = n / 4;
    nk_span_walk<4>(n4, [&](size_t i) { return reinterpret_cast<const float4*>(x)[i]; },
                    [&](size_t i, const float4& v) { nk_store_stream(reinterpret_cast<float4*>(y) + i, act_value4<ACT>(v)); });
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) y[n4 * 4 + threadIdx.x] = act_value<ACT>(x[n4 * 4 + threadIdx.x]);
}

// dx (+)= g act'(x); nt: `nt` loads (operands beyond the Infinity Cache, nk_common.h)
template <int ACT, bool ASSIGN>
__global__ __launch_bounds__(256) void activation_bwd_kernel(float* __restrict__ dx, const float* __restrict__ g, const float* __restrict__ x,
                                                              size_t n, bool nt) {
    const size_t n4 = n / 4;
    struct R { float4 x, g, d; };
    nk_span_walk<4>(n4, [&](size_t i) {
        R r;
        r.x = nk_load_stream(reinterpret_cast<const float4*>(x) + i, nt);
        r.g = nk_load_stream(reinterpret_cast<const float4*>(g) + i, nt);
        r.d = ASSIGN ? make_float4(0.f, 0.f, 0.f, 0.f) : nk_load_stream(reinterpret_cast<const float4*>(dx) + i, nt);
        return r;
    }, [&](size_t i, const R& r) {
        float4 d;
        d.x = r.g.x * act_deriv<ACT>(r.x.x); d.y = r.g.y * act_deriv<ACT>(r.x.y);
        d.z = r.g.z * act_deriv<ACT>(r.x.z); d.w = r.g.w * act_deriv<ACT>(r.x.w);
        d.x += r.d.x; d.y += r.d.y; d.z += r.d.z; d.w += r.d.w;  // ASSIGN: + 0, so that a -0 product gives the +0 that `+=` on zeros gives
        nk_store_stream(reinterpret_cast<float4*>(dx) + i, d);
    });
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = n4 * 4 + threadIdx.x;
        const float v = g[i] * act_deriv<ACT>(x[i]);
        dx[i] = v + (ASSIGN ? 0.f : dx[i]);
    }
}

// ------------------------------------------------------------------------------------------------ gated, H % 4 == 0
// item i = (row, q): row = i / H4, q = i % H4; the a group is x4[row 2 H4 + q], the b group H4 further on
template <int ACT>
__global__ __launch_bounds__(256) void glu_fwd_vec_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned items, unsigned H4) {
    struct R { float4 a, b; };
    nk_span_walk<4>((size_t)items, [&](size_t i) {
        const unsigned row = (unsigned)i / H4, o = (unsigned)i + row * H4;  // row 2 H4 + q
        R r;
        r.a = reinterpret_cast<const float4*>(x)[o];
        r.b = reinterpret_cast<const float4*>(x)[o + H4];
        return r;
    }, [&](size_t i, const R& r) {
        const float4 s = act_value4<ACT>(r.b);
        nk_store_stream(reinterpret_cast<float4*>(y) + i, make_float4(r.a.x * s.x, r.a.y * s.y, r.a.z * s.z, r.a.w * s.w));
    });
}

// dx[r, j] (+)= g act(b), dx[r, H + j] (+)= g a act'(b)
template <int ACT, bool ASSIGN>
__global__ __launch_bounds__(256) void glu_bwd_vec_kernel(float* __restrict__ dx, const float* __restrict__ g, const float* __restrict__ x,
                                                           unsigned items, unsigned H4, bool nt) {
    struct R { float4 a, b, g, da, db; };
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    nk_span_walk<2>((size_t)items, [&](size_t i) {
        const unsigned row = (unsigned)i / H4, o = (unsigned)i + row * H4;
        R r;
        r.a = nk_load_stream(reinterpret_cast<const float4*>(x) + o, nt);
        r.b = nk_load_stream(reinterpret_cast<const float4*>(x) + o + H4, nt);
        r.g = nk_load_stream(reinterpret_cast<const float4*>(g) + i, nt);
        r.da = ASSIGN ? zero : nk_load_stream(reinterpret_cast<const float4*>(dx) + o, nt);
        r.db = ASSIGN ? zero : nk_load_stream(reinterpret_cast<const float4*>(dx) + o + H4, nt);
        return r;
    }, [&](size_t i, const R& r) {
        const unsigned row = (unsigned)i / H4, o = (unsigned)i + row * H4;
        const act_vd sx = act_both<ACT>(r.b.x), sy = act_both<ACT>(r.b.y), sz = act_both<ACT>(r.b.z), sw = act_both<ACT>(r.b.w);
        float4 da = make_float4(r.g.x * sx.v, r.g.y * sy.v, r.g.z * sz.v, r.g.w * sw.v);
        float4 db = make_float4(r.g.x * r.a.x * sx.d, r.g.y * r.a.y * sy.d, r.g.z * r.a.z * sz.d, r.g.w * r.a.w * sw.d);
        da.x += r.da.x; da.y += r.da.y; da.z += r.da.z; da.w += r.da.w;  // ASSIGN: + 0, as above
        db.x += r.db.x; db.y += r.db.y; db.z += r.db.z; db.w += r.db.w;
        nk_store_stream(reinterpret_cast<float4*>(dx) + o, da);
        nk_store_stream(reinterpret_cast<float4*>(dx) + o + H4, db);
    });
}

// ------------------------------------------------------------------------------------------------ gated, any H
template <int ACT>
__global__ __launch_bounds__(256) void glu_fwd_scalar_kernel(const float* __restrict__ x, float* __restrict__ y, unsigned items, unsigned H) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned row = (unsigned)i / H, o = (unsigned)i + row * H;
        y[i] = x[o] * act_value<ACT>(x[o + H]);
    }
}
template <int ACT, bool ASSIGN>
__global__ __launch_bounds__(256) void glu_bwd_scalar_kernel(float* __restrict__ dx, const float* __restrict__ g, const float* __restrict__ x,
                                                              unsigned items, unsigned H) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned row = (unsigned)i / H, o = (unsigned)i + row * H;
        const act_vd s = act_both<ACT>(x[o + H]);
        const float da = g[i] * s.v, db = g[i] * x[o] * s.d;
        dx[o] = da + (ASSIGN ? 0.f : dx[o]);
        dx[o + H] = db + (ASSIGN ? 0.f : dx[o + H]);
    }
}

// ------------------------------------------------------------------------------------------------ host side
bool act_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

#define ACT_POINTER(p, what) \
    NK_CHECK((p) != nullptr && act_al16(p), "%s: %s is %s", what, #p, (p) ? "not 16-byte aligned" : "a null pointer")
#define ACT_DISPATCH(act, CALL)                       \
    switch (act) {                                    \
        case NK_ACT_GELU: CALL(NK_ACT_GELU); break;   \
        case NK_ACT_GELU_TANH: CALL(NK_ACT_GELU_TANH); break; \
        case NK_ACT_SILU: CALL(NK_ACT_SILU); break;   \
        default: CALL(NK_ACT_SIGMOID); break;         \
    }

bool act_known(int act) { return act >= NK_ACT_GELU && act <= NK_ACT_SIGMOID; }

template <bool ASSIGN>
int activation_bwd(nk_device* dev, int act, float* dx, const float* g, const float* x, size_t n) {
    const char* what = ASSIGN ? "nk_activation_bwd_assign" : "nk_activation_bwd";
    NK_CHECK(act_known(act), "%s: unknown activation %d", what, act);
    if (n != 0) {
        ACT_POINTER(dx, what);
        ACT_POINTER(g, what);
        ACT_POINTER(x, what);
    }
    NK_CHECK(dev != nullptr, "%s: null device handle", what);
    if (n == 0) return NK_OK;
    NK_USE(dev);
    const bool nt = nk_streams_past_cache(n * (ASSIGN ? 12 : 16));
    const dim3 grid(nk_stream_grid(n / 4 + 1, 256)), block(256);
#define ACT_BWD(A) hipLaunchKernelGGL((activation_bwd_kernel<A, ASSIGN>), grid, block, 0, dev->compute, dx, g, x, n, nt)
    ACT_DISPATCH(act, ACT_BWD)
#undef ACT_BWD
    NK_LAUNCH_CHECK();
    return NK_OK;
}

// the shared argument checks of the gated entries
int glu_check(int act, long long rows, int H, const char* what) {
    NK_CHECK(act_known(act), "%s: unknown activation %d", what, act);
    NK_CHECK(H > 0, "%s: H must be positive, got %d", what, H);
    NK_CHECK(rows >= 0, "%s: rows must not be negative, got %lld", what, rows);
    NK_CHECK(rows <= GLU_MAX_ELEMS / (2LL * H), "%s: rows * 2 H = %lld * 2 * %d is beyond the index type (2^31 - 1 elements)", what, rows, H);
    return NK_OK;
}

template <bool ASSIGN>
int glu_bwd(nk_device* dev, int act, float* dx, const float* g, const float* x, long long rows, int H) {
    const char* what = ASSIGN ? "nk_glu_bwd_assign" : "nk_glu_bwd";
    if (int rc = glu_check(act, rows, H, what)) return rc;
    if (rows != 0) {
        ACT_POINTER(dx, what);
        ACT_POINTER(g, what);
        ACT_POINTER(x, what);
    }
    NK_CHECK(dev != nullptr, "%s: null device handle", what);
    if (rows == 0) return NK_OK;
    NK_USE(dev);
    const unsigned items = (unsigned)(rows * H);
    if (H % 4 == 0) {
        const bool nt = nk_streams_past_cache((size_t)items * 4 * (ASSIGN ? 5 : 7));  // x: 2, g: 1, dx: 2 written (and 2 read by `+=`)
        const dim3 grid(nk_stream_grid(items / 4, 256)), block(256);
#define GLU_BWD(A) hipLaunchKernelGGL((glu_bwd_vec_kernel<A, ASSIGN>), grid, block, 0, dev->compute, dx, g, x, items / 4, (unsigned)H / 4, nt)
        ACT_DISPATCH(act, GLU_BWD)
#undef GLU_BWD
    } else {
        const dim3 grid(nk_stream_grid(items, 256)), block(256);
#define GLU_BWD(A) hipLaunchKernelGGL((glu_bwd_scalar_kernel<A, ASSIGN>), grid, block, 0, dev->compute, dx, g, x, items, (unsigned)H)
        ACT_DISPATCH(act, GLU_BWD)
#undef GLU_BWD
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_activation_fwd(nk_device* dev, int act, const float* x, float* y, size_t n) {
    const char* what = "nk_activation_fwd";
    NK_CHECK(act_known(act), "%s: unknown activation %d", what, act);
    if (n != 0) {
        ACT_POINTER(x, what);
        ACT_POINTER(y, what);
    }
    NK_CHECK(dev != nullptr, "%s: null device handle", what);
    if (n == 0) return NK_OK;
    NK_USE(dev);
    const dim3 grid(nk_stream_grid(n / 4 + 1, 256)), block(256);
#define ACT_FWD(A) hipLaunchKernelGGL((activation_fwd_kernel<A>), grid, block, 0, dev->compute, x, y, n)
    ACT_DISPATCH(act, ACT_FWD)
#undef ACT_FWD
    NK_LAUNCH_CHECK();
    return NK_OK;
}
int nk_activation_bwd(nk_device* dev, int act, float* dx, const float* g, const float* x, size_t n) {
    return activation_bwd<false>(dev, act, dx, g, x, n);
}
int nk_activation_bwd_assign(nk_device* dev, int act, float* dx, const float* g, const float* x, size_t n) {
    return activation_bwd<true>(dev, act, dx, g, x, n);
}

int nk_glu_fwd(nk_device* dev, int act, const float* x, float* y, long long rows, int H) {
    const char* what = "nk_glu_fwd";
    if (int rc = glu_check(act, rows, H, what)) return rc;
    if (rows != 0) {
        ACT_POINTER(x, what);
        ACT_POINTER(y, what);
    }
    NK_CHECK(dev != nullptr, "%s: null device handle", what);
    if (rows == 0) return NK_OK;
    NK_USE(dev);
    const unsigned items = (unsigned)(rows * H);
    if (H % 4 == 0) {
        const dim3 grid(nk_stream_grid(items / 4, 256)), block(256);
#define GLU_FWD(A) hipLaunchKernelGGL((glu_fwd_vec_kernel<A>), grid, block, 0, dev->compute, x, y, items / 4, (unsigned)H / 4)
        ACT_DISPATCH(act, GLU_FWD)
#undef GLU_FWD
    } else {
        const dim3 grid(nk_stream_grid(items, 256)), block(256);
#define GLU_FWD(A) hipLaunchKernelGGL((glu_fwd_scalar_kernel<A>), grid, block, 0, dev->compute, x, y, items, (unsigned)H)
        ACT_DISPATCH(act, GLU_FWD)
#undef GLU_FWD
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}
int nk_glu_bwd(nk_device* dev, int act, float* dx, const float* g, const float* x, long long rows, int H) {
    return glu_bwd<false>(dev, act, dx, g, x, rows, H);
}
int nk_glu_bwd_assign(nk_device* dev, int act, float* dx, const float* g, const float* x, long long rows, int H) {
    return glu_bwd<true>(dev, act, dx, g, x, rows, H);
}

}  // extern "C"
