// The body of the general dx kernels of nk_norm.hip: any D, any alignment; a 256-thread block per row, scalar passes over memory.
// Included INSIDE the signatures of layer_norm_bwd_general_kernel and rms_norm_bwd_general_kernel (no kernel of its own, no include
// guard; the includer defines and undefines NORM_CENTRED).  The formula is that of nk_norm_dx_body.h.
#if NORM_CENTRED
#define NORM_XC(c) (xr[c] - mean)
#define NORM_DX(gh, c) rstd * (gh - c1 - NORM_XC(c) * rstd * c2)
#else
#define NORM_XC(c) xr[c]
#define NORM_DX(gh, c) rstd * (gh - NORM_XC(c) * rstd * c2)
#endif
    __shared__ float red[4];
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* gr = g + row * D;
        const float* xr = x + row * D;
        float* dr = dx + row * D;
#if NORM_CENTRED
        const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
        float s1 = 0.f;
#else
        const float rstd = stats[row];
#endif
        float s2 = 0.f;
        for (int c = threadIdx.x; c < D; c += 256) {
            const float gh = gamma ? gr[c] * gamma[c] : gr[c];
#if NORM_CENTRED
            s1 += gh;
#endif
            s2 += gh * (NORM_XC(c) * rstd);
        }
#if NORM_CENTRED
        const float c1 = owner_sum<true>(s1, red) / (float)D;
#endif
        const float c2 = owner_sum<true>(s2, red) / (float)D;
        for (int c = threadIdx.x; c < D; c += 256) {
            const float gh = gamma ? gr[c] * gamma[c] : gr[c];
            const float d = NORM_DX(gh, c);
            dr[c] = assign ? d : dr[c] + d;
        }
    }
#undef NORM_DX
#undef NORM_XC
