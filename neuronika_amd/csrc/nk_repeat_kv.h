// repeat_kv (ours; semantics in include/neuronika_hip.h): the training / prefill side of grouped-query attention.  The fused
// attention core keeps running on H = Hkv*G heads of K and V: kv head k is written G times in front of it (heads k*G .. k*G + G - 1)
// and the gradients of the copies are summed behind it.  Included by nk_norm.hip.  Streaming kernels: one thread per element (or
// 16-byte group) of the NARROW operand, which it reads or writes once, and a loop over the G copies in ascending order -
//   fwd         y[r, (k*G + j)*dh + e] = x[r, k*dh + e], a bit-exact copy
//   bwd         dx[r, k*dh + e] += ((g_0 + g_1) + g_2) + ...   with g_j = g[r, (k*G + j)*dh + e], f32, j ascending
//   bwd_assign  dx[r, k*dh + e]  = that sum
// so the bits are fixed by the order.  16-byte accesses (T = float4, DV = dh / 4) when dh % 4 == 0 and both strides and pointers
// allow it, scalar otherwise.  Row offsets are 64-bit; columns outside [0, Hkv*dh) of x / dx and [0, Hkv*G*dh) of y / g are never
// touched, so the operands may be column blocks of packed buffers.  No atomics, no LDS.
#pragma once
#include "nk_common.h"

namespace {

__device__ __forceinline__ float rkv_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 rkv_add(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

constexpr int RKV_FWD = 0, RKV_BWD = 1, RKV_BWD_ASSIGN = 2;

// `narrow` is x (read) or dx (written), `wide` is y (written) or g (read); strides and DV in units of T.  W = Hkv*DV.
template <typename T, int MODE>
__global__ void __launch_bounds__(256) repeat_kv_kernel(T* __restrict__ narrow, long long ldn, T* __restrict__ wide, long long ldw, int W, int G,
                                                        int DV, long long total) {
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const long long r = i / W;
        const int c = (int)(i % W), k = c / DV, e = c % DV;
        T* __restrict__ np = narrow + r * ldn + c;
        T* __restrict__ wp = wide + r * ldw + (long long)k * G * DV + e;
        if (MODE == RKV_FWD) {
            const T v = *np;
            for (int j = 0; j < G; ++j) wp[(long long)j * DV] = v;
        } else {
            T s = wp[0];
            for (int j = 1; j < G; ++j) s = rkv_add(s, wp[(long long)j * DV]);
            *np = MODE == RKV_BWD ? rkv_add(*np, s) : s;
        }
    }
}

bool rkv_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int MODE>
int repeat_kv_launch(nk_device* dev, const char* what, float* narrow, int ldn, float* wide, int ldw, int rows, int Hkv, int G, int dh) {
    NK_CHECK(dev != nullptr, "null device handle");
    NK_CHECK(rows > 0 && Hkv > 0 && G > 0 && dh > 0, "%s: rows, Hkv, G and dh must be positive, got %d, %d, %d, %d", what, rows, Hkv, G, dh);
    NK_CHECK((long long)Hkv * G * dh <= 0x7fffffffLL, "%s: Hkv*G*dh must fit 31 bits", what);
    NK_CHECK(narrow != nullptr && wide != nullptr, "%s: null pointer", what);
    NK_CHECK(ldn >= Hkv * dh, "%s: row stride %d is shorter than Hkv*dh = %d", what, ldn, Hkv * dh);
    NK_CHECK(ldw >= Hkv * G * dh, "%s: row stride %d is shorter than Hkv*G*dh = %d", what, ldw, Hkv * G * dh);
    NK_USE(dev);
    const bool vec = dh % 4 == 0 && ldn % 4 == 0 && ldw % 4 == 0 && rkv_al16(narrow) && rkv_al16(wide);
    const int DV = vec ? dh / 4 : dh, W = Hkv * DV;
    const long long total = (long long)rows * W;
    const dim3 grid(nk_stream_grid((size_t)total, 256)), block(256);
    if (vec)
        hipLaunchKernelGGL((repeat_kv_kernel<float4, MODE>), grid, block, 0, dev->compute, reinterpret_cast<float4*>(narrow), (long long)(ldn / 4),
                           reinterpret_cast<float4*>(wide), (long long)(ldw / 4), W, G, DV, total);
    else
        hipLaunchKernelGGL((repeat_kv_kernel<float, MODE>), grid, block, 0, dev->compute, narrow, (long long)ldn, wide, (long long)ldw, W, G, DV,
                           total);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_repeat_kv_fwd(nk_device* dev, const float* x, int ldx, float* y, int ldy, int rows, int Hkv, int G, int dh) {
    return repeat_kv_launch<RKV_FWD>(dev, "nk_repeat_kv_fwd", const_cast<float*>(x), ldx, y, ldy, rows, Hkv, G, dh);  // x is only read
}
int nk_repeat_kv_bwd(nk_device* dev, float* dx, int lddx, const float* g, int ldg, int rows, int Hkv, int G, int dh) {
    return repeat_kv_launch<RKV_BWD>(dev, "nk_repeat_kv_bwd", dx, lddx, const_cast<float*>(g), ldg, rows, Hkv, G, dh);  // g is only read
}
int nk_repeat_kv_bwd_assign(nk_device* dev, float* dx, int lddx, const float* g, int ldg, int rows, int Hkv, int G, int dh) {
    return repeat_kv_launch<RKV_BWD_ASSIGN>(dev, "nk_repeat_kv_bwd_assign", dx, lddx, const_cast<float*>(g), ldg, rows, Hkv, G, dh);
}

}  // extern "C"
