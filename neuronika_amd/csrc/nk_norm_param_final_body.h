// The body of stage 2 of the parameter gradients of nk_norm.hip, included INSIDE the signatures of layer_norm_param_final_kernel
// and rms_norm_gamma_final_kernel (no kernel of its own, no include guard; the includer defines and undefines NORM_CENTRED).  A block
// sums the splits of 64 columns - wave w the splits [w * per, (w + 1) * per) in ascending order, the four waves' sums in wave order -
// and adds the total to the output or assigns it.  Centred, the grid is (tiles, 2) and blockIdx.y picks dgamma or dbeta and its plane
// of `part`; otherwise the grid is (tiles) and there is dgamma alone.
    __shared__ float sm[4][64];
#if NORM_CENTRED
    constexpr int NP = 2;
    const unsigned plane = blockIdx.y;
    float* out = plane ? dbeta : dgamma;
    if (!out) return;
#else
    constexpr int NP = 1, plane = 0;
    float* out = dgamma;
#endif
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = blockIdx.x * 64 + lane;
    const int per = (splits + 3) / 4, lo = w * per, hi = lo + per < splits ? lo + per : splits;
    float s = 0.f;
    if (col < D) {
        const float* p = part + (size_t)plane * D + col;
#pragma unroll 8
        for (int i = lo; i < hi; ++i) s += p[(size_t)i * NP * D];
    }
    sm[w][lane] = s;
    __syncthreads();
    if (w == 0 && col < D) {
        const float total = (sm[0][lane] + sm[1][lane]) + (sm[2][lane] + sm[3][lane]);
        out[col] = assign ? total : out[col] + total;
    }
