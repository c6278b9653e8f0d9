// Rotary position embedding (ours; semantics in include/neuronika_hip.h): the first `rot` columns of every head of a strided row
// buffer are rotated by the angle of the row's position, in place or out of place, from a (max_pos, rot / 2, 2) table of (cos, sin)
// made in f64.  Included by nk_norm.hip.  One streaming pass; the backward is the same pass with the sign of the sine flipped.
//   table    filled on the HOST: frequency, product, cos and sin in f64, rounded to f32 once, one upload.  An f32 angle is 1e-3 rad
//            off at position 16 384; an f64 kernel would buy nothing for a table built once per model.
//   vector   rot / 2 % 4 == 0 (half-split) or rot % 4 == 0 (interleaved), dh % 4 == 0, both strides % 4 == 0, every base 16-byte
//            aligned.  An item is 16 bytes of a head: half-split - the float4 at column 4 q AND its partner rot / 2 further on, with
//            the two table float4 (c0 s0 c1 s1 | c2 s2 c3 s3) of their four pairs; interleaved - one float4 = two pairs and one
//            table float4.  Columns [rot, dh) are further items of the head (a copy, or `dx (+)= g`); the in-place forms do not
//            visit them.  Consecutive lanes take consecutive items: consecutive 16-byte pieces of a row (two such streams when
//            half-split).  The walk is the span walk of nk_common.h, U = 2: 2 x (2 data + 2 table [+ 2 dx]) loads in flight.
//   scalar   everything else: an item is one pair or one pass-through column, grid-stride.
// A thread owns BOTH members of every pair it touches and reads them before it writes either: y == x needs no barrier.  No LDS, no
// atomics.  The table row of a position (rot floats) is shared by every head and sample at that position and stays in L2.
// Both families evaluate
//     y1 = fmaf(x1, c, -(x2 * s));   y2 = fmaf(x2, c, x1 * s)            (inverse: s -> -s, exact)
// so the bits of an element are a function of its pair, its position and the table alone.  The position start[b] + t is clamped into
// [0, max_pos) here: no start can make a thread read outside the table.
// Index types: rows = B * T and the items of a row fit 31 bits (checked by the host side); row offsets rows * ld are 64-bit.
#pragma once
#include <cmath>

#include "nk_common.h"

namespace {

struct rope_geom {
    const float* table;
    const int* start;           // B positions or null
    long long lds, ldd;         // row strides of the source and the destination, in floats
    unsigned T, dh, rot, max_pos;
    unsigned ipr, iph, npair;   // items per row, per head; the first npair items of a head are pairs, the others pass-through
};

// position of row (b, t) given start[b] (0 without a start array), clamped into the table
__device__ __forceinline__ unsigned rope_clamp(const rope_geom& G, int s0, unsigned t) {
    long long p = (long long)s0 + t;
    p = p < 0 ? 0 : p;
    return p >= (long long)G.max_pos ? G.max_pos - 1 : (unsigned)p;
}
// item -> (row, head, q); 32-bit division whenever the launch's item count allows it (uniform branch)
__device__ __forceinline__ void rope_split(const rope_geom& G, size_t i, bool small, unsigned& row, unsigned& h, unsigned& q) {
    unsigned rem;
    if (small) {
        row = (unsigned)i / G.ipr;
        rem = (unsigned)i - row * G.ipr;
    } else {
        row = (unsigned)(i / G.ipr);
        rem = (unsigned)(i - (size_t)row * G.ipr);
    }
    h = rem / G.iph;
    q = rem - h * G.iph;
}
template <bool INV>
__device__ __forceinline__ void rope_pair(float x1, float x2, float c, float s, float& y1, float& y2) {
    if (INV) s = -s;
    y1 = fmaf(x1, c, -(x2 * s));
    y2 = fmaf(x2, c, x1 * s);
}
template <bool NT>
__device__ __forceinline__ float4 rope_ld(const float* p) { return nk_load_stream(reinterpret_cast<const float4*>(p), NT); }
template <bool NT>
__device__ __forceinline__ void rope_st(float* p, const float4& v) {
    if (NT) nk_store_stream(reinterpret_cast<float4*>(p), v);
    else *reinterpret_cast<float4*>(p) = v;
}
__device__ __forceinline__ float4 rope_add4(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// IL: interleaved pairing.  INV: the transposed rotation.  ACC: dst += (INV only).  NT: `nt` loads and stores (the pass is beyond the
// Infinity Cache).  src may equal dst unless ACC.
// The span walk of nk_common.h (block b owns a contiguous span, U trips' loads in flight) written out in three phases per trip, so that
// nothing waits between the loads: (1) where the U items live and their positions - the start[b] loads of all of them together,
// under the one uniform branch of the kernel; (2) every data, table and dx load, BRANCH-FREE: a pass-through item reads its own
// 16 bytes in place of a partner and the head of its table row, and drops both; (3) rotate, select, store.
template <bool IL, bool INV, bool ACC, bool NT>
__global__ __launch_bounds__(256) void rope_vec_kernel(const float* src, float* dst, rope_geom G, size_t items) {
    constexpr int U = 2;
    const bool small = items <= 0xffffffffull;
    const unsigned half = G.rot / 2;
    const size_t per = (items + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, end = lo + per < items ? lo + per : items;
    for (size_t i0 = lo + threadIdx.x; i0 < end; i0 += U * 256) {
        bool live[U], pair[U];
        unsigned q[U], t[U], b[U], pos[U];
        size_t os[U], od[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const size_t i = i0 + u * 256;
            live[u] = i < end;
            unsigned row, h;
            rope_split(G, live[u] ? i : i0, small, row, h, q[u]);  // a dead slot re-reads the trip's first item and stores nothing
            pair[u] = q[u] < G.npair;
            const unsigned col = h * G.dh + (pair[u] ? 4 * q[u] : G.rot + 4 * (q[u] - G.npair));
            os[u] = (size_t)row * G.lds + col;
            od[u] = (size_t)row * G.ldd + col;
            b[u] = row / G.T;
            t[u] = row - b[u] * G.T;
        }
        if (G.start) {
            int s0[U];
#pragma unroll
            for (int u = 0; u < U; ++u) s0[u] = G.start[b[u]];
#pragma unroll
            for (int u = 0; u < U; ++u) pos[u] = rope_clamp(G, s0[u], t[u]);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) pos[u] = rope_clamp(G, 0, t[u]);
        }
        float4 xa[U], xb[U], t0[U], t1[U], da[U], db[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned other = pair[u] ? half : 0u;
            const float* tp = G.table + (size_t)pos[u] * G.rot + (pair[u] ? (IL ? 4 : 8) * q[u] : 0u);
            xa[u] = rope_ld<NT>(src + os[u]);
            t0[u] = *reinterpret_cast<const float4*>(tp);
            if (!IL) {
                xb[u] = rope_ld<NT>(src + os[u] + other);
                t1[u] = *reinterpret_cast<const float4*>(tp + 4);
            }
            if (ACC) {
                da[u] = rope_ld<NT>(dst + od[u]);
                if (!IL) db[u] = rope_ld<NT>(dst + od[u] + other);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float4 ya, yb;
            if (IL) {
                rope_pair<INV>(xa[u].x, xa[u].y, t0[u].x, t0[u].y, ya.x, ya.y);
                rope_pair<INV>(xa[u].z, xa[u].w, t0[u].z, t0[u].w, ya.z, ya.w);
            } else {
                rope_pair<INV>(xa[u].x, xb[u].x, t0[u].x, t0[u].y, ya.x, yb.x);
                rope_pair<INV>(xa[u].y, xb[u].y, t0[u].z, t0[u].w, ya.y, yb.y);
                rope_pair<INV>(xa[u].z, xb[u].z, t1[u].x, t1[u].y, ya.z, yb.z);
                rope_pair<INV>(xa[u].w, xb[u].w, t1[u].z, t1[u].w, ya.w, yb.w);
            }
            if (!pair[u]) ya = xa[u];
            if (ACC) ya = rope_add4(da[u], ya);
            if (live[u]) rope_st<NT>(dst + od[u], ya);
            if (!IL && live[u] && pair[u]) {
                if (ACC) yb = rope_add4(db[u], yb);
                rope_st<NT>(dst + od[u] + half, yb);
            }
        }
    }
}

// item = one pair (q < npair) or one pass-through column
template <bool INV, bool ACC>
__global__ __launch_bounds__(256) void rope_scalar_kernel(const float* src, float* dst, rope_geom G, size_t items, bool il) {
    const bool small = items <= 0xffffffffull;
    const unsigned half = G.rot / 2;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < items; i += (size_t)gridDim.x * blockDim.x) {
        unsigned row, h, q;
        rope_split(G, i, small, row, h, q);
        const float* s = src + (size_t)row * G.lds + h * G.dh;
        float* d = dst + (size_t)row * G.ldd + h * G.dh;
        if (q >= G.npair) {
            const unsigned c = G.rot + (q - G.npair);
            const float v = s[c];
            d[c] = ACC ? d[c] + v : v;
            continue;
        }
        const unsigned c1 = il ? 2 * q : q, c2 = il ? 2 * q + 1 : q + half;
        const unsigned b = row / G.T;
        const float* t = G.table + (size_t)rope_clamp(G, G.start ? G.start[b] : 0, row - b * G.T) * G.rot + 2 * q;
        const float x1 = s[c1], x2 = s[c2];
        float y1, y2;
        rope_pair<INV>(x1, x2, t[0], t[1], y1, y2);
        d[c1] = ACC ? d[c1] + y1 : y1;
        d[c2] = ACC ? d[c2] + y2 : y2;
    }
}

bool rope_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The checks every entry shares, then the family by the rules above (a base off a 16-byte boundary is how the parity tests enter
// the scalar family with a vector shape).  src -> dst: x -> y forward, g -> dx backward.
template <bool INV, bool ACC>
int rope_launch(nk_device* dev, const char* what, const float* src, int lds, float* dst, int ldd, const float* table, const int* start, int B,
                int T, int NH, int dh, int rot, int max_pos, int interleaved) {
    NK_CHECK(B > 0 && T > 0 && NH > 0 && dh > 0 && max_pos > 0, "%s: B, T, NH, dh and max_pos must be positive, got %d, %d, %d, %d, %d", what, B,
             T, NH, dh, max_pos);
    NK_CHECK(rot >= 2 && rot <= dh && rot % 2 == 0, "%s: rot must be even and in [2, dh = %d], got %d", what, dh, rot);
    NK_CHECK((long long)B * T <= 0x7fffffffLL, "%s: B * T = %lld rows are beyond the index type (2^31 - 1)", what, (long long)B * T);
    NK_CHECK((long long)NH * dh <= 0x7fffffffLL && (long long)NH * dh <= lds && (long long)NH * dh <= ldd,
             "%s: NH * dh = %lld columns do not fit the row strides %d and %d", what, (long long)NH * dh, lds, ldd);
    NK_CHECK(start != nullptr || T <= max_pos, "%s: T = %d positions from 0 exceed the table's %d", what, T, max_pos);
    NK_CHECK(src != nullptr && dst != nullptr && table != nullptr, "%s: null pointer", what);
    NK_CHECK(!ACC || src != dst, "%s: dx == g is legal for the assign form only", what);
    NK_CHECK(src != dst || lds == ldd, "%s: the in-place form needs equal strides, got %d and %d", what, lds, ldd);
    NK_CHECK(dev != nullptr, "%s: null device handle", what);
    NK_USE(dev);
    const bool il = interleaved != 0, inplace = src == dst;
    const bool vec = (il ? rot % 4 == 0 : rot % 8 == 0) && dh % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && rope_al16(src) && rope_al16(dst) &&
                     rope_al16(table);
    rope_geom G;
    G.table = table; G.start = start; G.lds = lds; G.ldd = ldd;
    G.T = (unsigned)T; G.dh = (unsigned)dh; G.rot = (unsigned)rot; G.max_pos = (unsigned)max_pos;
    const unsigned pass = inplace ? 0u : (unsigned)(dh - rot);  // in place the pass-through columns are already where they belong
    if (vec) {
        G.npair = (unsigned)rot / (il ? 4 : 8);
        G.iph = G.npair + pass / 4;
    } else {
        G.npair = (unsigned)rot / 2;
        G.iph = G.npair + pass;
    }
    G.ipr = G.iph * (unsigned)NH;
    const size_t items = (size_t)B * T * G.ipr;
    const dim3 grid(nk_stream_grid(items, 256)), block(256);
    if (vec) {
        // bytes the pass touches: read + write of the visited columns (+ the read of dx)
        const bool nt = nk_streams_past_cache(items * (il ? 16 : (size_t)32) * (ACC ? 3 : 2));
#define ROPE_VEC(IL, NT) hipLaunchKernelGGL((rope_vec_kernel<IL, INV, ACC, NT>), grid, block, 0, dev->compute, src, dst, G, items)
        if (il && nt) ROPE_VEC(true, true);
        else if (il) ROPE_VEC(true, false);
        else if (nt) ROPE_VEC(false, true);
        else ROPE_VEC(false, false);
#undef ROPE_VEC
    } else {
        hipLaunchKernelGGL((rope_scalar_kernel<INV, ACC>), grid, block, 0, dev->compute, src, dst, G, items, il);
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // namespace

extern "C" {

int nk_rope_table(nk_device* dev, float* table, int max_pos, int rot, double base) {
    const char* what = "nk_rope_table";
    NK_CHECK(max_pos > 0, "%s: max_pos must be positive, got %d", what, max_pos);
    NK_CHECK(rot >= 2 && rot % 2 == 0, "%s: rot must be even and at least 2, got %d", what, rot);
    NK_CHECK(base > 0.0 && std::isfinite(base), "%s: base must be positive and finite", what);
    NK_CHECK((long long)max_pos * rot <= 0x7fffffffLL, "%s: max_pos * rot = %lld entries are beyond the index type (2^31 - 1)", what,
             (long long)max_pos * rot);
    NK_CHECK(table != nullptr, "%s: null pointer", what);
    NK_CHECK(dev != nullptr, "%s: null device handle", what);
    NK_USE(dev);
    if (int rc = nk_refuse_capture(dev, what, "fill the table before the capture begins")) return rc;
    const int half = rot / 2;
    std::vector<double> theta((size_t)half);
    for (int j = 0; j < half; ++j) theta[(size_t)j] = std::pow(base, -2.0 * j / (double)rot);
    std::vector<float> host((size_t)max_pos * rot);
    for (int p = 0; p < max_pos; ++p)
        for (int j = 0; j < half; ++j) {
            const double a = (double)p * theta[(size_t)j];
            host[((size_t)p * half + j) * 2] = (float)std::cos(a);
            host[((size_t)p * half + j) * 2 + 1] = (float)std::sin(a);
        }
    NK_HIP(hipMemcpyAsync(table, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, dev->compute));
    NK_HIP(hipStreamSynchronize(dev->compute));  // `host` dies with this call
    return NK_OK;
}

int nk_rope_fwd(nk_device* dev, const float* x, int ldx, float* y, int ldy, const float* table, const int* start, int B, int T, int NH, int dh,
                int rot, int max_pos, int interleaved) {
    return rope_launch<false, false>(dev, "nk_rope_fwd", x, ldx, y, ldy, table, start, B, T, NH, dh, rot, max_pos, interleaved);
}
int nk_rope_bwd(nk_device* dev, float* dx, int lddx, const float* g, int ldg, const float* table, const int* start, int B, int T, int NH, int dh,
                int rot, int max_pos, int interleaved) {
    return rope_launch<true, true>(dev, "nk_rope_bwd", g, ldg, dx, lddx, table, start, B, T, NH, dh, rot, max_pos, interleaved);
}
int nk_rope_bwd_assign(nk_device* dev, float* dx, int lddx, const float* g, int ldg, const float* table, const int* start, int B, int T, int NH,
                       int dh, int rot, int max_pos, int interleaved) {
    return rope_launch<true, false>(dev, "nk_rope_bwd_assign", g, ldg, dx, lddx, table, start, B, T, NH, dh, rot, max_pos, interleaved);
}

}  // extern "C"
