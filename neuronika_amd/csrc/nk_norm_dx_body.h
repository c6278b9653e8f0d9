// The body of the row-in-registers dx kernels of nk_norm.hip, included INSIDE the signatures of layer_norm_bwd_kernel<V, BLOCK> and
// rms_norm_bwd_kernel<V, BLOCK> (no kernel of its own, no include guard; the includer defines and undefines NORM_CENTRED).
//   dx (+)= rstd * (gh - c1 - xhat * c2),  gh = g * gamma,  xhat = (x - mean) * rstd as the forward formed it,
//   c2 = mean_D(gh * xhat) and, centred only, c1 = mean_D(gh); RMSNorm has no mean, no c1 and one reduction.
// flags: bit 0 assign, bit 1 operands beyond the Infinity Cache (launch-time choice, nk_common.h)
#if NORM_CENTRED
#define NORM_DX(e) rstd * (gv[i].e - c1 - xv[i].e * c2)
#else
#define NORM_DX(e) rstd * (gv[i].e - xv[i].e * c2)
#endif
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
#if NORM_CENTRED
        const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
        float s1 = 0.f;
#else
        const float rstd = stats[row];
#endif
        float s2 = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = (i * T + t) * 4;
            if (c < D) {
                if (gamma) { const float4 w = *reinterpret_cast<const float4*>(gamma + c); gv[i].x *= w.x; gv[i].y *= w.y; gv[i].z *= w.z; gv[i].w *= w.w; }
#if NORM_CENTRED
                xv[i] = sub4(xv[i], mean);
#endif
                xv[i].x *= rstd; xv[i].y *= rstd; xv[i].z *= rstd; xv[i].w *= rstd;
#if NORM_CENTRED
                s1 += sum4(gv[i]);
#endif
                s2 += dot4(gv[i], xv[i]);
            }
        }
#if NORM_CENTRED
        const float c1 = owner_sum<BLOCK>(s1, red) / (float)D;
#endif
        const float c2 = owner_sum<BLOCK>(s2, red) / (float)D;
        float* dr = dx + row * D;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = (i * T + t) * 4;
            if (c < D) {
                float4 d = make_float4(NORM_DX(x), NORM_DX(y), NORM_DX(z), NORM_DX(w));
                if (!assign) { d.x += dv[i].x; d.y += dv[i].y; d.z += dv[i].z; d.w += dv[i].w; }
                nk_store_stream(reinterpret_cast<float4*>(dr + c), d);
            }
        }
    }
#undef NORM_DX
