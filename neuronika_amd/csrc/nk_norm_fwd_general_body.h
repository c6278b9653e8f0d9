// The body of the general forward kernels of nk_norm.hip: any D, any alignment; a 256-thread block per row, scalar passes over
// memory (the row is re-read from cache).  Included INSIDE the signatures of layer_norm_fwd_general_kernel and
// rms_norm_fwd_general_kernel (no kernel of its own, no include guard; the includer defines and undefines NORM_CENTRED).
    __shared__ float red[4];
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* xr = x + row * D;
        float* yr = y + row * D;
#if NORM_CENTRED
        float s = 0.f;
        for (int c = threadIdx.x; c < D; c += 256) s += xr[c];
        const float mean = owner_sum<true>(s, red) / (float)D;
#define NORM_XC(c) (xr[c] - mean)
#else
#define NORM_XC(c) xr[c]
#endif
        float q = 0.f;
        for (int c = threadIdx.x; c < D; c += 256) { const float d = NORM_XC(c); q += d * d; }
        const float rstd = 1.f / sqrtf(owner_sum<true>(q, red) / (float)D + eps);
#if NORM_CENTRED
        if (stats && threadIdx.x == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
#else
        if (stats && threadIdx.x == 0) stats[row] = rstd;
#endif
        for (int c = threadIdx.x; c < D; c += 256) {
            float o = NORM_XC(c) * rstd;
            if (gamma) o *= gamma[c];
#if NORM_CENTRED
            if (beta) o += beta[c];
#endif
            yr[c] = o;
        }
    }
#undef NORM_XC
