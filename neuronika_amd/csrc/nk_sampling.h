// Token sampling (ours; semantics in include/neuronika_hip.h): greedy, temperature, top-k and top-p over rows of logits, the chosen
// index written as f32.  Included by nk_norm.hip.  ONE workgroup of 1024 threads per row; every decision is an integer comparison.
//   keys     a logit becomes an order-preserving 32-bit key (-0 as +0, NaN = 0 below -inf): a larger value has a larger key, equal
//            values have equal keys.  The weight of a token is a function of its key, the row's maximum and c alone
//            (sample_weight, the one place the exponential is taken), so equal values carry equal weights and every sum below is a
//            64-bit integer sum - exact, whatever order the lanes arrive in.
//   access   vector family: the row pointer and ld keep every row 16-byte aligned - float4 loads, the last partial quad by scalars.
//            scalar family: everything else.  A thread always owns the quad of elements 4q .. 4q+3, so both families and the staged
//            form see the same elements in the same places.
//   staging  V <= SAMPLE_STAGE: pass 1 leaves the keys in LDS (128 KiB) and the later passes read them there; larger rows are read
//            again from global memory (they sit in L2: a row is at most 4 MiB).
//   passes   1  the maximum and its first index: the 64-bit maximum of (key << 32 | ~index).  Greedy rows, and rows whose maximum
//               is not finite, end here.
//            2  top-k: radix select, four 8-bit digits from the top, a histogram of COUNTS per digit in LDS (integer LDS atomics,
//               a thread adds a run of equal digits once), a suffix scan over the 256 bins, the digit that holds the k-th largest.
//            3  top-p: the same select with histograms of the WEIGHTS of the tokens top-k kept; the first histogram's total is W,
//               which gives the target.  Without top-p: one pass that sums the kept weights.
//            4  the draw: one Philox call per row, R = mulhi64(r64, W), then tiles of 4096 elements in index order - a block scan of
//               the quads' weights, the one thread whose quad's running sum crosses R writes the id, the walk stops at that tile.
// No float atomics, no global atomics, no workspace.  Nothing is written but ids[row], by exactly one thread.
#pragma once
#include <cmath>

#include "nk_common.h"

namespace {

typedef unsigned long long sample_u64;
constexpr int SAMPLE_NT = 1024;        // 16 waves
constexpr int SAMPLE_STAGE = 32768;    // keys a row may keep in LDS
constexpr int SAMPLE_BINS = 256;       // 8-bit digits
constexpr unsigned SAMPLE_KEY_NINF = 0x007fffffu, SAMPLE_KEY_PINF = 0xff800000u;  // finite values lie strictly between

struct sample_smem {
    sample_u64 hist[SAMPLE_BINS];
    sample_u64 suf[SAMPLE_BINS + 1];   // suf[d] = sum of hist[d ..], suf[256] = 0
    sample_u64 wave[SAMPLE_NT / 64];
    unsigned sel;
};

__device__ __forceinline__ unsigned sample_key(float x) {
    unsigned b = __float_as_uint(x);
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0u;  // NaN: below -inf
    if (b == 0x80000000u) b = 0u;                    // -0 counts as +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float sample_value(unsigned k) {  // the inverse, for k != 0
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// w = (uint64)(e * 2^40), e = 2^((x - m) * c); 0 for NaN and -inf; the maximum itself has 2^40 whatever c is
__device__ __forceinline__ sample_u64 sample_weight(unsigned k, float m, float c) {
    if (k <= SAMPLE_KEY_NINF) return 0;
    const float d = sample_value(k) - m;
    if (d == 0.f) return 1ull << 40;
    return (sample_u64)(exp2f(d * c) * 1099511627776.0f);
}

// the keys of elements 4q .. 4q+3 of a row in global memory; returns how many of them exist (the others get key 0)
template <bool VEC>
__device__ __forceinline__ int sample_load_quad(const float* x, unsigned V, unsigned q, unsigned (&k)[4]) {
    const unsigned i = 4 * q;
    if (VEC && i + 4 <= V) {
        const float4 v = *reinterpret_cast<const float4*>(x + i);
        k[0] = sample_key(v.x); k[1] = sample_key(v.y); k[2] = sample_key(v.z); k[3] = sample_key(v.w);
        return 4;
    }
    const int n = V - i < 4u ? (int)(V - i) : 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = j < n ? sample_key(x[i + j]) : 0u;
    return n;
}

template <bool VEC, bool STAGED>
struct sample_row {
    const float* x;
    const unsigned* keys;  // LDS, (V + 3) / 4 quads, the tail of the last quad 0
    unsigned V;
    __device__ __forceinline__ int quad(unsigned q, unsigned (&k)[4]) const {
        if (STAGED) {
            const uint4 v = *reinterpret_cast<const uint4*>(keys + 4 * q);
            k[0] = v.x; k[1] = v.y; k[2] = v.z; k[3] = v.w;
            return V - 4 * q < 4u ? (int)(V - 4 * q) : 4;
        }
        return sample_load_quad<VEC>(x, V, q, k);
    }
};

// block-wide maximum (MAX) or sum of one 64-bit value per thread; the result in every thread.  Two barriers.
template <bool MAX>
__device__ __forceinline__ sample_u64 sample_block_reduce(sample_u64 v, sample_smem& sm) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const sample_u64 u = __shfl_xor(v, off, 64);
        v = MAX ? (u > v ? u : v) : v + u;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm.wave[threadIdx.x >> 6] = v;
    __syncthreads();
    sample_u64 r = sm.wave[0];
#pragma unroll
    for (int i = 1; i < SAMPLE_NT / 64; ++i) {
        const sample_u64 u = sm.wave[i];
        r = MAX ? (u > r ? u : r) : r + u;
    }
    return r;
}

// suf[d] = hist[d] + hist[d + 1] + .. over the 256 bins, by the first four waves.  Enter behind a barrier; leaves behind one.
__device__ __forceinline__ void sample_suffix(sample_smem& sm) {
    const unsigned tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    sample_u64 v = 0;
    if (tid < SAMPLE_BINS) {
        v = sm.hist[tid];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const sample_u64 u = __shfl_down(v, off, 64);
            if (lane + off < 64) v += u;
        }
        if (lane == 0) sm.wave[wid] = v;
    }
    __syncthreads();
    if (tid < SAMPLE_BINS) {
        for (unsigned w = wid + 1; w < SAMPLE_BINS / 64; ++w) v += sm.wave[w];
        sm.suf[tid] = v;
        if (tid == 0) sm.suf[SAMPLE_BINS] = 0;
    }
    __syncthreads();
}

// The largest key t for which the values of {tokens with key >= t} sum to >= target, and that sum.  A token's value is 1 (a count:
// top-k, target = k) or, WEIGHTED, its weight when its key is >= floor_key and 0 otherwise (top-p; the target is formed from the
// first histogram's total, the W of the tokens top-k kept).  Invariant of the walk down the digits: above < target <= above + the
// sum of the tokens under the current prefix.
template <bool WEIGHTED, class Row>
__device__ __forceinline__ void sample_select(const Row& row, sample_smem& sm, float m, float c, unsigned floor_key, sample_u64 target, float top_p,
                                              unsigned& thr, sample_u64& kept) {
    const unsigned tid = threadIdx.x, nq = (row.V + 3) / 4;
    sample_u64 prefix = 0, above = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < SAMPLE_BINS) sm.hist[tid] = 0;
        __syncthreads();
        unsigned cur = 0;
        sample_u64 acc = 0;  // a run of equal digits is added once
        for (unsigned q = tid; q < nq; q += SAMPLE_NT) {
            unsigned k[4];
            const int n = row.quad(q, k);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= n || ((sample_u64)k[j] >> (shift + 8)) != prefix) continue;
                const sample_u64 v = WEIGHTED ? (k[j] >= floor_key ? sample_weight(k[j], m, c) : 0ull) : 1ull;
                const unsigned d = (k[j] >> shift) & (SAMPLE_BINS - 1);
                if (d != cur) {
                    if (acc) atomicAdd(&sm.hist[cur], acc);
                    cur = d;
                    acc = 0;
                }
                acc += v;
            }
        }
        if (acc) atomicAdd(&sm.hist[cur], acc);
        __syncthreads();
        sample_suffix(sm);
        if (WEIGHTED && shift == 24) {
            const sample_u64 W = sm.suf[0];
            target = (sample_u64)((double)top_p * (double)W);
            target = target < 1 ? 1 : (target > W ? W : target);
        }
        if (tid < SAMPLE_BINS && above + sm.suf[tid] >= target && above + sm.suf[tid + 1] < target) sm.sel = tid;
        __syncthreads();
        const unsigned d = sm.sel & (SAMPLE_BINS - 1);
        kept = above + sm.suf[d];
        above += sm.suf[d + 1];
        prefix = (prefix << 8) | d;
    }
    thr = (unsigned)prefix;
}

// The lowest index whose running sum of kept weights, in index order, exceeds R (R < the sum of all of them).
template <class Row>
__device__ __forceinline__ void sample_draw(const Row& row, sample_smem& sm, float m, float c, unsigned thr, sample_u64 R, float* id) {
    const unsigned tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nq = (row.V + 3) / 4;
    sample_u64 base = 0;
    for (unsigned q0 = 0; q0 < nq; q0 += SAMPLE_NT) {
        const unsigned q = q0 + tid;
        sample_u64 w[4] = {0, 0, 0, 0};
        if (q < nq) {
            unsigned k[4];
            const int n = row.quad(q, k);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n && k[j] >= thr) w[j] = sample_weight(k[j], m, c);
        }
        const sample_u64 mine = w[0] + w[1] + w[2] + w[3];
        sample_u64 inc = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const sample_u64 u = __shfl_up(inc, off, 64);
            if ((int)lane >= off) inc += u;
        }
        __syncthreads();  // the previous tile's reads of sm.wave
        if (lane == 63) sm.wave[wid] = inc;
        __syncthreads();
        sample_u64 lo = base + inc - mine, total = 0;
#pragma unroll
        for (unsigned i = 0; i < SAMPLE_NT / 64; ++i) {
            const sample_u64 t = sm.wave[i];
            if (i < wid) lo += t;
            total += t;
        }
        if (lo <= R && R - lo < mine) {  // this quad crosses R: one thread of the whole walk
            sample_u64 run = lo;
            int j = 0;
            for (; j < 3; ++j) {
                run += w[j];
                if (run > R) break;
            }
            *id = (float)(4 * q + (unsigned)j);
        }
        base += total;
        if (base > R) break;  // uniform
    }
}

template <bool VEC, bool STAGED>
__global__ __launch_bounds__(SAMPLE_NT) void sample_row_kernel(const float* logits, long long ld, unsigned V, float* ids, int greedy, float c,
                                                               unsigned top_k, float top_p, uint2 key, uint2 offset) {
    __shared__ sample_smem sm;
    __shared__ __attribute__((aligned(16))) unsigned keys[STAGED ? SAMPLE_STAGE : 4];
    const unsigned tid = threadIdx.x, r = blockIdx.x, nq = (V + 3) / 4;
    const float* x = logits + (size_t)r * ld;
    if (tid == 0) sm.sel = 0;
    // pass 1: the maximum and its first index (equal keys: the larger ~index, the lower index); the keys go to LDS on the way
    sample_u64 best = 0;
    for (unsigned q = tid; q < nq; q += SAMPLE_NT) {
        unsigned k[4];
        const int n = sample_load_quad<VEC>(x, V, q, k);
        if (STAGED) *reinterpret_cast<uint4*>(keys + 4 * q) = make_uint4(k[0], k[1], k[2], k[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const sample_u64 cand = (sample_u64)k[j] << 32 | (0xffffffffu - (4 * q + j));
            if (j < n && cand > best) best = cand;
        }
    }
    best = sample_block_reduce<true>(best, sm);
    const unsigned kmax = (unsigned)(best >> 32), imax = 0xffffffffu - (unsigned)best;
    if (greedy || kmax <= SAMPLE_KEY_NINF || kmax >= SAMPLE_KEY_PINF) {
        if (tid == 0) ids[r] = (float)imax;
        return;
    }
    const float m = sample_value(kmax);
    const sample_row<VEC, STAGED> row{x, keys, V};
    unsigned thr = 0;
    sample_u64 W = 0;
    if (top_k > 0 && top_k < V) sample_select<false>(row, sm, m, c, 0u, (sample_u64)top_k, 1.f, thr, W);
    if (top_p < 1.f) {
        sample_select<true>(row, sm, m, c, thr, 1ull, top_p, thr, W);
    } else {
        sample_u64 s = 0;
        for (unsigned q = tid; q < nq; q += SAMPLE_NT) {
            unsigned k[4];
            const int n = row.quad(q, k);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n && k[j] >= thr) s += sample_weight(k[j], m, c);
        }
        W = sample_block_reduce<false>(s, sm);
    }
    const uint4 rnd = philox4x32_10(make_uint4(offset.x, offset.y, r, 0x53414D50u), key);
    const sample_u64 R = __umul64hi((sample_u64)rnd.y << 32 | rnd.x, W);
    sample_draw(row, sm, m, c, thr, R, ids + r);
}

}  // namespace

extern "C" {

int nk_sample_stage_limit(void) { return SAMPLE_STAGE; }

int nk_sample_fwd(nk_device* dev, const float* logits, long long ld, int rows, int V, float* ids, float temperature, int top_k, float top_p,
                  uint64_t seed, uint64_t offset) {
    const char* what = "nk_sample_fwd";
    NK_CHECK(logits != nullptr && ids != nullptr, "%s: null pointer", what);
    NK_CHECK(rows > 0, "%s: rows must be positive, got %d", what, rows);
    NK_CHECK(V > 0 && V <= (1 << 20), "%s: V must be in [1, 2^20], got %d", what, V);
    NK_CHECK(ld >= (long long)V, "%s: ld = %lld is shorter than a row of V = %d", what, ld, V);
    NK_CHECK(temperature >= 0.f && std::isfinite(temperature), "%s: temperature must be finite and not negative", what);
    NK_CHECK(top_p > 0.f, "%s: top_p must be positive", what);  // false for NaN
    NK_CHECK(dev != nullptr, "%s: null device handle", what);
    NK_USE(dev);
    const bool greedy = temperature == 0.f;
    if (!greedy)
        if (int rc = nk_refuse_capture(dev, "nk_sample_fwd: the Philox offset (every replay would draw the same ids)",
                                       "sample outside the capture, or capture the greedy form (temperature 0)"))
            return rc;
    const float c = greedy ? 0.f : 1.44269504f / temperature;
    const bool vec = (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && ld % 4 == 0;
    const bool staged = !greedy && V <= SAMPLE_STAGE;  // a greedy row is read once
    const uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32)), off = make_uint2((unsigned)offset, (unsigned)(offset >> 32));
    const dim3 grid((unsigned)rows), block(SAMPLE_NT);
#define SAMPLE_GO(VEC, STAGED)                                                                                                        \
    hipLaunchKernelGGL((sample_row_kernel<VEC, STAGED>), grid, block, 0, dev->compute, logits, ld, (unsigned)V, ids, greedy ? 1 : 0, c, \
                       (unsigned)(top_k > 0 ? top_k : 0), top_p, key, off)
    if (vec && staged) SAMPLE_GO(true, true);
    else if (vec) SAMPLE_GO(true, false);
    else if (staged) SAMPLE_GO(false, true);
    else SAMPLE_GO(false, false);
#undef SAMPLE_GO
    NK_LAUNCH_CHECK();
    return NK_OK;
}

}  // extern "C"
