// The body of the row-in-registers forward kernels of nk_norm.hip.  No kernel of its own and no include guard: it is included INSIDE
// the signatures of layer_norm_fwd_kernel<V, BLOCK> and rms_norm_fwd_kernel<V, BLOCK>, whose includer defines, and undefines after
// the include, NORM_CENTRED (1 = LayerNorm: mean and beta exist, stats holds {mean, rstd} per row; 0 = RMSNorm: rstd alone).
// BLOCK = false: blocks of four waves, a wave per row.  BLOCK = true: a 256-thread block per row.
    constexpr int T = BLOCK ? 256 : 64;
    __shared__ float red[4];
    const int t = BLOCK ? threadIdx.x : threadIdx.x & 63;
    const long long first = BLOCK ? blockIdx.x : blockIdx.x * 4ll + (threadIdx.x >> 6), step = BLOCK ? gridDim.x : gridDim.x * 4ll;
    for (long long row = first; row < rows; row += step) {
        float4 v[V];
        quads_load<V, T>(v, x + row * D, t, D, false);
#if NORM_CENTRED
        float mean, rstd;
        row_stats<V, T>(v, t, D, eps, red, &mean, &rstd);
        if (stats && t == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
#else
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < V; ++i)
            if ((i * T + t) * 4 < D) q += sq4(v[i]);
        const float rstd = 1.f / sqrtf(owner_sum<BLOCK>(q, red) / (float)D + eps);
        if (stats && t == 0) stats[row] = rstd;
#endif
        float* yr = y + row * D;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const int c = (i * T + t) * 4;
            if (c < D) {
                float4 o = make_float4(v[i].x * rstd, v[i].y * rstd, v[i].z * rstd, v[i].w * rstd);
                if (gamma) { const float4 w = *reinterpret_cast<const float4*>(gamma + c); o.x *= w.x; o.y *= w.y; o.z *= w.z; o.w *= w.w; }
#if NORM_CENTRED
                if (beta) { const float4 b = *reinterpret_cast<const float4*>(beta + c); o.x += b.x; o.y += b.y; o.z += b.z; o.w += b.w; }
#endif
                nk_store_stream(reinterpret_cast<float4*>(yr + c), o);
            }
        }
    }
