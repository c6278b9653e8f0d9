// The body of the combine kernels of single-query attention (nk_attention_decode.h says what they compute).  No kernel of its own and
// no include guard: it is included INSIDE the signatures of adec_combine_kernel and adw_combine_kernel.  One thread per (problem,
// column).  The includer defines, and undefines after the include:
//   ADEC_WINDOW   0: a problem of n keys has chunks 0 .. (n - 1) / C.  1: chunks lo / C .. (n - 1) / C, lo = max(0, n - W); arguments
//                 W and ring.  Either way its partials are the first nc of its nchunks places in the workspace.
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int e = (int)(i % dh);
    const long long prob = i / dh;
    const int row = (int)(prob / H), b = row / T, t = row % T;
#if ADEC_WINDOW
    const int n = adec_len(start, b, t, cap, ring), lo = n > W ? n - W : 0;
    if (n <= 0) return;  // zeroed by the partial kernel
    const int nc = (n - 1) / C - lo / C + 1;
    if (nc == 1) return;  // written by the partial kernel
#else
    const int n = adec_len(start, b, t, cap, 0);
    if (n <= C) return;  // written by the partial kernel
    const int nc = (n + C - 1) / C;
#endif
    const size_t stride = (size_t)dh + 2;
    const float* __restrict__ part = ws + (size_t)prob * nchunks * stride;
    float m = part[dh];
    for (int c = 1; c < nc; ++c) m = fmaxf(m, part[c * stride + dh]);
    float o = 0.f, l = 0.f;
    for (int c = 0; c < nc; ++c) {
        const float f = __builtin_amdgcn_exp2f(part[c * stride + dh] - m);
        o = __builtin_fmaf(part[c * stride + e], f, o);
        l = __builtin_fmaf(part[c * stride + dh + 1], f, l);
    }
    O[(size_t)prob * dh + e] = o / l;  // prob = (b*T + t)*H + h: column h*dh + e of row b*T + t
