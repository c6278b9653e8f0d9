// Nearest and linear (bilinear, trilinear) resampling over 1, 2 or 3 spatial axes of an (N, C, spatial...) tensor: forward, and the
// backward in GATHER form - a thread owns input elements and walks the outputs that read them in ascending row-major order - so there
// is no atomic anywhere and every result repeats bit for bit.  Semantics: include/neuronika_hip.h.  Included once, by nk_pool.hip, whose
// pool_al16 and pool_grid it uses.  Every geometry is normalised to three axes (D, H, W), a missing axis being 1 -> 1; the linear
// kernels still take the number of real axes as a template argument, because an axis that is not there contributes no arithmetic
// (1 * a + 0 * a is not a for an infinite a).
//
// Every kernel walks ROWS: `lanes` (a power of two) lanes lie along W, a block of 256 threads holds 256 / lanes rows, and the
// row -> (plane, d, h) divisions, the source rows of nearest and the (i0, i1, l0, l1) of the outer axes happen once per row.  Along
// the row nothing is divided: the integer quotients nearest needs (the source column of an output, the first output of an input
// column) are carried as (quotient, remainder) pairs from one division per thread and stepped.
//
// Classes, chosen by the host code at the bottom from (mode, in, out) and the pointers' 16-byte alignment alone; all of them do the
// same operations per element in the same order, so they give the same bits:
//   NEAREST2  nearest, out_W == 2 in_W, in_W % 4 == 0, both pointers 16-byte aligned, any ratio on the outer axes.  Forward: a lane
//             loads 16 bytes of x and stores two 16-byte groups to every output row that reads its input row.  Backward: a lane
//             owns 16 bytes of dx and reads g in 16-byte loads.
//   VECTOR    forward: out_W % 4 == 0 and y aligned - a lane makes four adjacent outputs from scalar gathers and stores 16 bytes;
//             backward: in_W % 4 == 0 and dx aligned - a lane owns 16 bytes of dx, one read of g serving its four elements.
//   GENERIC   the same two kernels with one element per lane: any shape, any alignment.
// Plain loads and stores throughout: the streaming (`nt`) forms are unmeasured for these passes and left out.
//
// Rounding.  Every f32 operation of the linear mode is rounded on its own.  upsample_mul / _add / _sub are what __fmul_rn / __fadd_rn /
// __fsub_rn promise, written as plain operators under `#pragma clang fp contract(off)`: this toolchain's __f*_rn are plain operators
// compiled with contraction allowed, which the compiler may still fuse into an FMA once they are inlined next to each other.

namespace {

__device__ __forceinline__ float upsample_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float upsample_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float upsample_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

struct UpStep { unsigned q, r; };
struct UpGeom {
    int in[3], out[3];     // (D, H, W)
    float s[3];            // linear: the f32 source step of each axis
    int align;
    int in_plane, out_plane;
    long long planes;      // N * C
    long long rows;        // planes * out_D * out_H (forward) or planes * in_D * in_H (backward, NEAREST2 forward)
    int lanes;             // lanes along W
    // floor((i * wnum + wadd) / wden) along W, stepped by one element and by one lane stride
    unsigned wnum, wden, wadd;
    UpStep one, stride;
    // linear backward: floor(i * num / den) - lo .. + hi surely holds every output that reads input i of that axis
    unsigned num[3], den[3];
    long long lo[3], hi[3], ceil_ratio;
};

// The one place the source position of an output index is computed: forward and backward both call it.
struct UpAxis { int i[2]; float l[2]; };
__device__ __forceinline__ UpAxis upsample_axis(int o, int in, float s, int align) {
    const float fo = (float)o;
    const float src = align ? upsample_mul(s, fo) : fmaxf(upsample_sub(upsample_mul(s, upsample_add(fo, 0.5f)), 0.5f), 0.f);
    UpAxis a;
    a.i[0] = min((int)floorf(src), in - 1);
    a.i[1] = min(a.i[0] + 1, in - 1);
    a.l[1] = upsample_sub(src, (float)a.i[0]);
    a.l[0] = upsample_sub(1.f, a.l[1]);
    return a;
}
__device__ __forceinline__ float upsample_pair(float l0, float a, float l1, float b) { return upsample_add(upsample_mul(l0, a), upsample_mul(l1, b)); }

struct UpWalk { unsigned v, rem; };
__device__ __forceinline__ UpWalk upsample_walk(unsigned i, unsigned num, unsigned add, unsigned den) {
    const unsigned long long t = (unsigned long long)i * num + add;
    UpWalk k;
    k.v = (unsigned)(t / den);
    k.rem = (unsigned)(t % den);
    return k;
}
__device__ __forceinline__ void upsample_step(UpWalk& k, UpStep s, unsigned den) {
    k.v += s.q;
    k.rem += s.r;  // both below den <= 2^31 - 1
    if (k.rem >= den) { k.rem -= den; ++k.v; }
}

struct UpRow { long long plane; int d, h; };
__device__ __forceinline__ UpRow upsample_row(long long row, int D, int H) {
    UpRow r;
    r.plane = row / (D * H);  // D * H <= a plane: 31 bits
    const int t = (int)(row - r.plane * (D * H));
    r.d = t / H;
    r.h = t - r.d * H;
    return r;
}
// nearest: the source index of output o, and the first output whose source is >= i
__device__ __forceinline__ int upsample_near_src(int o, int in, int out) { return min((int)(((long long)o * in) / out), in - 1); }
__device__ __forceinline__ int upsample_near_first(int i, int in, int out) { return (int)(((long long)i * out + in - 1) / in); }

// ------------------------------------------------------------------------------------------------ forward, VEC = 1 (generic) or 4
template <int ND, int MODE, int VEC>
__global__ __launch_bounds__(256) void upsample_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, UpGeom q) {
    const int cx = threadIdx.x & (q.lanes - 1), ry = threadIdx.x / q.lanes, rpb = 256 / q.lanes;
    const int ID = q.in[0], IH = q.in[1], IW = q.in[2], OD = q.out[0], OH = q.out[1], OW = q.out[2];
    const int ow0 = cx * VEC, span = q.lanes * VEC;
    UpWalk k0 = {0u, 0u};
    if (MODE == NK_UPSAMPLE_NEAREST && ow0 < OW) k0 = upsample_walk((unsigned)ow0, q.wnum, q.wadd, q.wden);
    for (long long row = (long long)blockIdx.x * rpb + ry; row < q.rows; row += (long long)gridDim.x * rpb) {
        const UpRow r = upsample_row(row, OD, OH);
        const float* xp = x + r.plane * q.in_plane;
        float* yr = y + row * OW;
        if (MODE == NK_UPSAMPLE_NEAREST) {
            const float* xr = xp + ((long long)upsample_near_src(r.d, ID, OD) * IH + upsample_near_src(r.h, IH, OH)) * IW;
            UpWalk k = k0;
            for (int ow = ow0; ow < OW; ow += span) {
                if (VEC == 4) {
                    UpWalk t = k;
                    float e[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        e[j] = xr[min(t.v, (unsigned)(IW - 1))];
                        upsample_step(t, q.one, q.wden);
                    }
                    *reinterpret_cast<float4*>(yr + ow) = make_float4(e[0], e[1], e[2], e[3]);
                } else {
                    yr[ow] = xr[min(k.v, (unsigned)(IW - 1))];
                }
                upsample_step(k, q.stride, q.wden);
            }
        } else {
            UpAxis ad = {{0, 0}, {1.f, 0.f}}, ah = {{0, 0}, {1.f, 0.f}};
            if (ND >= 3) ad = upsample_axis(r.d, ID, q.s[0], q.align);
            if (ND >= 2) ah = upsample_axis(r.h, IH, q.s[1], q.align);
            const float* p[2][2];
#pragma unroll
            for (int cd = 0; cd < 2; ++cd)
#pragma unroll
                for (int ch = 0; ch < 2; ++ch) p[cd][ch] = xp + ((long long)ad.i[cd] * IH + ah.i[ch]) * IW;
            for (int ow = ow0; ow < OW; ow += span) {
                float e[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const UpAxis aw = upsample_axis(ow + j, IW, q.s[2], q.align);
                    float v[2][2];
#pragma unroll
                    for (int cd = 0; cd < (ND >= 3 ? 2 : 1); ++cd)
#pragma unroll
                        for (int ch = 0; ch < (ND >= 2 ? 2 : 1); ++ch)
                            v[cd][ch] = upsample_pair(aw.l[0], p[cd][ch][aw.i[0]], aw.l[1], p[cd][ch][aw.i[1]]);
                    if (ND >= 2) {
#pragma unroll
                        for (int cd = 0; cd < (ND >= 3 ? 2 : 1); ++cd) v[cd][0] = upsample_pair(ah.l[0], v[cd][0], ah.l[1], v[cd][1]);
                    }
                    if (ND >= 3) v[0][0] = upsample_pair(ad.l[0], v[0][0], ad.l[1], v[1][0]);
                    e[j] = v[0][0];
                }
                if (VEC == 4) {
                    *reinterpret_cast<float4*>(yr + ow) = make_float4(e[0], e[VEC > 1 ? 1 : 0], e[VEC > 2 ? 2 : 0], e[VEC > 3 ? 3 : 0]);
                } else {
                    yr[ow] = e[0];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, VEC = 1 (generic) or 4
// the outputs lo .. hi of one axis among the candidates c - q.lo .. c + more + q.hi that read an input index in [i, i + n): the
// membership is upsample_axis's own answer.  The source position never decreases with o, so the readers of an index are contiguous.
__device__ __forceinline__ void upsample_readers(const UpGeom& q, int a, long long c, long long more, int i, int n, int& lo, int& hi) {
    const long long from = c - q.lo[a] > 0 ? c - q.lo[a] : 0;
    const long long to = c + more + q.hi[a] < q.out[a] - 1 ? c + more + q.hi[a] : q.out[a] - 1;
    lo = INT_MAX;
    hi = -1;
    for (long long o = from; o <= to; ++o) {
        const UpAxis t = upsample_axis((int)o, q.in[a], q.s[a], q.align);
        if ((t.i[0] >= i && t.i[0] < i + n) || (t.i[1] >= i && t.i[1] < i + n)) {
            lo = min(lo, (int)o);
            hi = (int)o;
        }
    }
}

template <int ND, int MODE, int VEC>
__global__ __launch_bounds__(256) void upsample_bwd_kernel(float* __restrict__ dx, const float* __restrict__ g, UpGeom q, int assign) {
    const int cx = threadIdx.x & (q.lanes - 1), ry = threadIdx.x / q.lanes, rpb = 256 / q.lanes;
    const int ID = q.in[0], IH = q.in[1], IW = q.in[2], OD = q.out[0], OH = q.out[1], OW = q.out[2];
    const int iw0 = cx * VEC, span = q.lanes * VEC;
    UpWalk k0 = {0u, 0u};
    if (iw0 < IW) k0 = upsample_walk((unsigned)iw0, q.wnum, q.wadd, q.wden);
    for (long long row = (long long)blockIdx.x * rpb + ry; row < q.rows; row += (long long)gridDim.x * rpb) {
        const UpRow r = upsample_row(row, ID, IH);
        const float* gp = g + r.plane * q.out_plane;
        float* dr = dx + row * IW;
        int d_lo = 0, d_hi = 0, h_lo = 0, h_hi = 0;
        if (MODE == NK_UPSAMPLE_NEAREST) {
            d_lo = upsample_near_first(r.d, ID, OD); d_hi = upsample_near_first(r.d + 1, ID, OD) - 1;
            h_lo = upsample_near_first(r.h, IH, OH); h_hi = upsample_near_first(r.h + 1, IH, OH) - 1;
        } else {
            if (ND >= 3) upsample_readers(q, 0, ((long long)r.d * q.num[0]) / q.den[0], 0, r.d, 1, d_lo, d_hi);
            if (ND >= 2) upsample_readers(q, 1, ((long long)r.h * q.num[1]) / q.den[1], 0, r.h, 1, h_lo, h_hi);
        }
        UpWalk k = k0;
        for (int iw = iw0; iw < IW; iw += span) {
            float acc[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
            if (MODE == NK_UPSAMPLE_NEAREST) {
                int first[VEC + 1];  // element j is read by the outputs first[j] .. first[j + 1] - 1
                UpWalk t = k;
#pragma unroll
                for (int j = 0; j <= VEC; ++j) {
                    first[j] = (int)min(t.v, (unsigned)OW);
                    upsample_step(t, q.one, q.wden);
                }
                for (int od = d_lo; od <= d_hi; ++od)
                    for (int oh = h_lo; oh <= h_hi; ++oh) {
                        const float* gr = gp + ((long long)od * OH + oh) * OW;
#pragma unroll
                        for (int j = 0; j < VEC; ++j)
                            for (int ow = first[j]; ow < first[j + 1]; ++ow) acc[j] = upsample_add(acc[j], gr[ow]);
                    }
            } else {
                int w_lo, w_hi;
                upsample_readers(q, 2, (long long)k.v, (VEC - 1) * q.ceil_ratio, iw, VEC, w_lo, w_hi);
                for (int od = d_lo; od <= d_hi; ++od) {
                    UpAxis ad = {{0, -1}, {1.f, 0.f}};
                    if (ND >= 3) ad = upsample_axis(od, ID, q.s[0], q.align);
                    const bool md[2] = {ND < 3 || ad.i[0] == r.d, ND >= 3 && ad.i[1] == r.d};
                    if (!md[0] && !md[1]) continue;
                    for (int oh = h_lo; oh <= h_hi; ++oh) {
                        UpAxis ah = {{0, -1}, {1.f, 0.f}};
                        if (ND >= 2) ah = upsample_axis(oh, IH, q.s[1], q.align);
                        const bool mh[2] = {ND < 2 || ah.i[0] == r.h, ND >= 2 && ah.i[1] == r.h};
                        if (!mh[0] && !mh[1]) continue;
                        const float* gr = gp + ((long long)od * OH + oh) * OW;
                        for (int ow = w_lo; ow <= w_hi; ++ow) {
                            const UpAxis aw = upsample_axis(ow, IW, q.s[2], q.align);
                            const float gv = gr[ow];
#pragma unroll
                            for (int j = 0; j < VEC; ++j)
#pragma unroll
                                for (int cd = 0; cd < (ND >= 3 ? 2 : 1); ++cd)
#pragma unroll
                                    for (int ch = 0; ch < (ND >= 2 ? 2 : 1); ++ch)
#pragma unroll
                                        for (int cw = 0; cw < 2; ++cw)
                                            if (md[cd] && mh[ch] && aw.i[cw] == iw + j) {
                                                float w = aw.l[cw];
                                                if (ND >= 2) w = upsample_mul(ah.l[ch], w);
                                                if (ND >= 3) w = upsample_mul(ad.l[cd], w);
                                                acc[j] = upsample_add(acc[j], upsample_mul(w, gv));
                                            }
                        }
                    }
                }
            }
            if (VEC == 4) {
                float4 v = make_float4(acc[0], acc[VEC > 1 ? 1 : 0], acc[VEC > 2 ? 2 : 0], acc[VEC > 3 ? 3 : 0]);
                if (!assign) {
                    const float4 o = *reinterpret_cast<const float4*>(dr + iw);
                    v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
                }
                *reinterpret_cast<float4*>(dr + iw) = v;
            } else {
                dr[iw] = assign ? acc[0] : dr[iw] + acc[0];
            }
            upsample_step(k, q.stride, q.wden);
        }
    }
}

// ------------------------------------------------------------------------------------------------ NEAREST2: out_W == 2 in_W
__global__ __launch_bounds__(256) void upsample_nearest2_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, UpGeom q) {
    const int cx = threadIdx.x & (q.lanes - 1), ry = threadIdx.x / q.lanes, rpb = 256 / q.lanes;
    const int ID = q.in[0], IH = q.in[1], OD = q.out[0], OH = q.out[1], OW = q.out[2], groups = q.in[2] / 4;
    for (long long row = (long long)blockIdx.x * rpb + ry; row < q.rows; row += (long long)gridDim.x * rpb) {
        const UpRow r = upsample_row(row, ID, IH);
        const int d_lo = upsample_near_first(r.d, ID, OD), d_hi = upsample_near_first(r.d + 1, ID, OD) - 1;
        const int h_lo = upsample_near_first(r.h, IH, OH), h_hi = upsample_near_first(r.h + 1, IH, OH) - 1;
        const float4* xr = reinterpret_cast<const float4*>(x) + row * groups;
        float* yp = y + r.plane * q.out_plane;
        for (int j = cx; j < groups; j += q.lanes) {
            const float4 v = xr[j];
            for (int od = d_lo; od <= d_hi; ++od)
                for (int oh = h_lo; oh <= h_hi; ++oh) {
                    float4* yr = reinterpret_cast<float4*>(yp + ((long long)od * OH + oh) * OW) + 2 * j;
                    yr[0] = make_float4(v.x, v.x, v.y, v.y);
                    yr[1] = make_float4(v.z, v.z, v.w, v.w);
                }
        }
    }
}

__global__ __launch_bounds__(256) void upsample_nearest2_bwd_kernel(float* __restrict__ dx, const float* __restrict__ g, UpGeom q, int assign) {
    const int cx = threadIdx.x & (q.lanes - 1), ry = threadIdx.x / q.lanes, rpb = 256 / q.lanes;
    const int ID = q.in[0], IH = q.in[1], OD = q.out[0], OH = q.out[1], OW = q.out[2], groups = q.in[2] / 4;
    for (long long row = (long long)blockIdx.x * rpb + ry; row < q.rows; row += (long long)gridDim.x * rpb) {
        const UpRow r = upsample_row(row, ID, IH);
        const int d_lo = upsample_near_first(r.d, ID, OD), d_hi = upsample_near_first(r.d + 1, ID, OD) - 1;
        const int h_lo = upsample_near_first(r.h, IH, OH), h_hi = upsample_near_first(r.h + 1, IH, OH) - 1;
        float4* dr = reinterpret_cast<float4*>(dx) + row * groups;
        const float* gp = g + r.plane * q.out_plane;
        for (int j = cx; j < groups; j += q.lanes) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int od = d_lo; od <= d_hi; ++od)
                for (int oh = h_lo; oh <= h_hi; ++oh) {
                    const float4* gr = reinterpret_cast<const float4*>(gp + ((long long)od * OH + oh) * OW) + 2 * j;
                    const float4 a = gr[0], b = gr[1];
                    acc.x = upsample_add(upsample_add(acc.x, a.x), a.y);
                    acc.y = upsample_add(upsample_add(acc.y, a.z), a.w);
                    acc.z = upsample_add(upsample_add(acc.z, b.x), b.y);
                    acc.w = upsample_add(upsample_add(acc.w, b.z), b.w);
                }
            if (!assign) {
                const float4 o = dr[j];
                acc = make_float4(o.x + acc.x, o.y + acc.y, o.z + acc.z, o.w + acc.w);
            }
            dr[j] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
// The validity rules of the header, the one place they live.
int upsample_geometry(const char* who, int nd, int mode, int align_corners, const int* x_shape, const int* out_size, UpGeom* q) {
    NK_CHECK(nd >= 1 && nd <= 3, "%s: nd = %d (1, 2 or 3 spatial axes)", who, nd);
    NK_CHECK(mode == NK_UPSAMPLE_NEAREST || mode == NK_UPSAMPLE_LINEAR, "%s: unknown mode %d", who, mode);
    NK_CHECK(mode == NK_UPSAMPLE_LINEAR || align_corners == 0, "%s: align_corners has no meaning for the nearest mode", who);
    NK_CHECK(x_shape && out_size, "null pointer in %s", who);
    NK_CHECK(x_shape[0] >= 0 && x_shape[1] >= 0, "%s: negative extent (N = %d, C = %d)", who, x_shape[0], x_shape[1]);
    UpGeom t{};
    for (int a = 0; a < 3; ++a) {
        t.in[a] = t.out[a] = 1;
        t.s[a] = 1.f;
        t.num[a] = 0; t.den[a] = 1; t.lo[a] = t.hi[a] = 0;
    }
    t.align = align_corners != 0;
    long long in_plane = 1, out_plane = 1;
    for (int i = 0; i < nd; ++i) {
        const int a = 3 - nd + i, in = x_shape[2 + i], out = out_size[i];
        NK_CHECK(in >= 1, "%s: spatial extent %d of axis %d", who, in, i);
        NK_CHECK(out >= 1, "%s: output extent %d of axis %d", who, out, i);
        in_plane *= in;
        out_plane *= out;
        NK_CHECK(in_plane <= INT_MAX && out_plane <= INT_MAX, "%s: a plane of more than 2^31 - 1 elements", who);
        t.in[a] = in; t.out[a] = out;
        t.s[a] = t.align ? (out == 1 ? 0.f : (float)(in - 1) / (float)(out - 1)) : (float)in / (float)out;
        // the outputs near floor(i * num / den): exact source positions of the readers of i lie within (i - 1, i + 1) (align_corners)
        // or (i - 1, i + 2) output steps; `slack` covers the f32 rounding of the position, below 2^-22 of the larger extent
        const long long num = t.align ? out - 1 : out, den = t.align ? in - 1 : in;
        const long long slack = 2 + (std::max(in, out) >> 21);
        if (den == 0 || num == 0) {
            t.num[a] = 0; t.den[a] = 1; t.lo[a] = 0; t.hi[a] = out;
        } else {
            const long long R = (num + den - 1) / den;
            t.num[a] = (unsigned)num; t.den[a] = (unsigned)den; t.lo[a] = R + slack; t.hi[a] = 2 * R + slack;
            if (a == 2) t.ceil_ratio = R;
        }
    }
    t.in_plane = (int)in_plane;
    t.out_plane = (int)out_plane;
    t.planes = (long long)x_shape[0] * x_shape[1];
    *q = t;
    return NK_OK;
}

// `items` lane items per row, `vec` elements each; floor((i * num + add) / den) is what the lanes step along W
void upsample_rows(UpGeom& q, long long rows, int items, int vec, unsigned num, unsigned add, unsigned den) {
    int lanes = 1;
    while (lanes < 256 && lanes < items) lanes *= 2;
    q.lanes = lanes;
    q.rows = rows;
    q.wnum = num; q.wadd = add; q.wden = den;
    q.one = UpStep{num / den, num % den};
    const unsigned long long s = (unsigned long long)lanes * vec * num;
    q.stride = UpStep{(unsigned)(s / den), (unsigned)(s % den)};
}
inline int upsample_grid(const UpGeom& q) { return pool_grid((q.rows + 256 / q.lanes - 1) / (256 / q.lanes) * 256); }

#define UPSAMPLE_LAUNCH(KERNEL, MODE, VEC, ...)                                                                            \
    do {                                                                                                                   \
        if (MODE == NK_UPSAMPLE_NEAREST) hipLaunchKernelGGL((KERNEL<3, NK_UPSAMPLE_NEAREST, VEC>), dim3(grid), dim3(256), 0, dev->compute, __VA_ARGS__); \
        else if (nd == 1) hipLaunchKernelGGL((KERNEL<1, NK_UPSAMPLE_LINEAR, VEC>), dim3(grid), dim3(256), 0, dev->compute, __VA_ARGS__);                \
        else if (nd == 2) hipLaunchKernelGGL((KERNEL<2, NK_UPSAMPLE_LINEAR, VEC>), dim3(grid), dim3(256), 0, dev->compute, __VA_ARGS__);                \
        else hipLaunchKernelGGL((KERNEL<3, NK_UPSAMPLE_LINEAR, VEC>), dim3(grid), dim3(256), 0, dev->compute, __VA_ARGS__);                             \
    } while (0)

int upsample_fwd(nk_device* dev, const char* who, int nd, int mode, int align_corners, const float* x, const int* x_shape, float* y,
                 const int* out_size) {
    NK_USE(dev);
    UpGeom q;
    if (int rc = upsample_geometry(who, nd, mode, align_corners, x_shape, out_size, &q)) return rc;
    NK_CHECK(x && y, "null pointer in %s", who);
    if (q.planes == 0) return NK_OK;
    const int IW = q.in[2], OW = q.out[2];
    if (mode == NK_UPSAMPLE_NEAREST && OW == 2 * (long long)IW && IW % 4 == 0 && pool_al16(x) && pool_al16(y)) {
        upsample_rows(q, q.planes * q.in[0] * q.in[1], IW / 4, 4, 1, 0, 1);
        hipLaunchKernelGGL(upsample_nearest2_fwd_kernel, dim3(upsample_grid(q)), dim3(256), 0, dev->compute, x, y, q);
    } else {
        const int vec = OW % 4 == 0 && pool_al16(y) ? 4 : 1;
        upsample_rows(q, q.planes * q.out[0] * q.out[1], (OW + vec - 1) / vec, vec, (unsigned)IW, 0, (unsigned)OW);
        const int grid = upsample_grid(q);
        if (vec == 4) UPSAMPLE_LAUNCH(upsample_fwd_kernel, mode, 4, x, y, q);
        else UPSAMPLE_LAUNCH(upsample_fwd_kernel, mode, 1, x, y, q);
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int upsample_bwd(nk_device* dev, const char* who, int nd, int mode, int align_corners, float* dx, const int* x_shape, const float* g,
                 const int* out_size, int assign) {
    NK_USE(dev);
    UpGeom q;
    if (int rc = upsample_geometry(who, nd, mode, align_corners, x_shape, out_size, &q)) return rc;
    NK_CHECK(dx && g, "null pointer in %s", who);
    if (q.planes == 0) return NK_OK;
    const int IW = q.in[2], OW = q.out[2];
    const long long rows = q.planes * q.in[0] * q.in[1];
    if (mode == NK_UPSAMPLE_NEAREST && OW == 2 * (long long)IW && IW % 4 == 0 && pool_al16(dx) && pool_al16(g)) {
        upsample_rows(q, rows, IW / 4, 4, 1, 0, 1);
        hipLaunchKernelGGL(upsample_nearest2_bwd_kernel, dim3(upsample_grid(q)), dim3(256), 0, dev->compute, dx, g, q, assign);
    } else {
        const int vec = IW % 4 == 0 && pool_al16(dx) ? 4 : 1;
        if (mode == NK_UPSAMPLE_NEAREST) upsample_rows(q, rows, (IW + vec - 1) / vec, vec, (unsigned)OW, (unsigned)(IW - 1), (unsigned)IW);
        else upsample_rows(q, rows, (IW + vec - 1) / vec, vec, q.num[2], 0, q.den[2]);
        const int grid = upsample_grid(q);
        if (vec == 4) UPSAMPLE_LAUNCH(upsample_bwd_kernel, mode, 4, dx, g, q, assign);
        else UPSAMPLE_LAUNCH(upsample_bwd_kernel, mode, 1, dx, g, q, assign);
    }
    NK_LAUNCH_CHECK();
    return NK_OK;
}
#undef UPSAMPLE_LAUNCH

}  // namespace

extern "C" {

int nk_upsample_out_size(int nd, const int* x_shape, const double* scale, int* out_size) {
    NK_CHECK(nd >= 1 && nd <= 3, "nk_upsample_out_size: nd = %d (1, 2 or 3 spatial axes)", nd);
    NK_CHECK(x_shape && scale && out_size, "null pointer in nk_upsample_out_size");
    NK_CHECK(x_shape[0] >= 0 && x_shape[1] >= 0, "nk_upsample_out_size: negative extent (N = %d, C = %d)", x_shape[0], x_shape[1]);
    int out[3];
    long long in_plane = 1, out_plane = 1;
    for (int i = 0; i < nd; ++i) {
        NK_CHECK(x_shape[2 + i] >= 1, "nk_upsample_out_size: spatial extent %d of axis %d", x_shape[2 + i], i);
        NK_CHECK(std::isfinite(scale[i]) && scale[i] > 0.0, "nk_upsample_out_size: scale %g of axis %d (must be finite and positive)", scale[i], i);
        const double o = std::floor((double)x_shape[2 + i] * scale[i]);
        NK_CHECK(o >= 1.0 && o <= (double)INT_MAX, "nk_upsample_out_size: output extent %g of axis %d", o, i);
        out[i] = (int)o;
        in_plane *= x_shape[2 + i];
        out_plane *= out[i];
        NK_CHECK(in_plane <= INT_MAX && out_plane <= INT_MAX, "nk_upsample_out_size: a plane of more than 2^31 - 1 elements");
    }
    for (int i = 0; i < nd; ++i) out_size[i] = out[i];
    return NK_OK;
}

int nk_upsample_fwd(nk_device* dev, int nd, int mode, int align_corners, const float* x, const int* x_shape, float* y, const int* out_size) {
    return upsample_fwd(dev, "nk_upsample_fwd", nd, mode, align_corners, x, x_shape, y, out_size);
}
int nk_upsample_bwd(nk_device* dev, int nd, int mode, int align_corners, float* dx, const int* x_shape, const float* g, const int* out_size) {
    return upsample_bwd(dev, "nk_upsample_bwd", nd, mode, align_corners, dx, x_shape, g, out_size, 0);
}
int nk_upsample_bwd_assign(nk_device* dev, int nd, int mode, int align_corners, float* dx, const int* x_shape, const float* g,
                           const int* out_size) {
    return upsample_bwd(dev, "nk_upsample_bwd_assign", nd, mode, align_corners, dx, x_shape, g, out_size, 1);
}

}  // extern "C"
