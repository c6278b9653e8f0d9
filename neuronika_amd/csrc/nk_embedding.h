// Embedding table (ours; semantics in include/neuronika_hip.h): a row gather forward, and a backward that is a scatter-add of n
// gradient rows into a (V, D) table WITHOUT float atomics - an inverted index of the ids (which tokens selected row v, in ascending
// token order) and an ordered sum per table row.  Included by nk_norm.hip, the row-kernel unit.
//   gather        lanes own columns, `lpr` lanes per row (a power of two, 64 / lpr rows per wave), four accesses in flight per lane;
//                 16-byte accesses where D % 4 == 0 and the pointers are 16-byte aligned (T = float4), scalar otherwise (T = float)
//   index         two launches over slabs of S vocabulary rows, one 1024-thread block per slab; every block scans all n ids (4 n bytes,
//                 L2 resident).  count: per-row counts through integer LDS atomics (a count does not depend on arrival order) and
//                 the slab's totals.  place: the block's offset from the totals of the slabs before it, an exclusive scan of its
//                 counts -> row_start, then the ids again in tiles of 4096: the tile's tokens of this slab are compacted IN TOKEN
//                 ORDER into LDS and one wave places them by row, ranks from ballots.  perm is the same on every run.
//                 padding_idx and ids >= V are dropped here.  Rows longer than EMB_CHUNK tokens are also listed chunk by chunk.
//   ordered sum   the owner of (row, 4 lpr columns) walks the row's perm segment in order with four gradient rows in flight,
//                 accumulates in registers from the FIRST contribution and writes once (+= or assign).  Rows longer than EMB_CHUNK
//                 are left to two further launches: one owner per listed chunk leaves a partial row in the workspace, then the
//                 row's partials are added in chunk order.  EMB_CHUNK is part of the summation order: a constant of the library.
#pragma once
#include "nk_common.h"

namespace {

constexpr int EMB_CHUNK = 128;          // tokens one owner sums; longer rows are summed chunk by chunk (partials added in chunk order)
constexpr int EMB_SLAB_MAX = 4096;      // vocabulary rows per index block (its LDS counters), 4 per thread
constexpr int EMB_INDEX_THREADS = 1024;
constexpr int EMB_TILE = 4096;          // tokens per placement tile, 4 per thread
constexpr int EMB_MAX_V = 1 << 24;      // f32 holds ids exactly up to 2^24
constexpr long long EMB_MAX_N = 1ll << 30;
constexpr int EMB_MAX_D = 1 << 24;
constexpr long long EMB_MAX_BLOCKS = 1 << 16;  // blocks per launch of the row kernels; they stride over the rest

bool emb_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// `id as usize` of an f32 id, as nk_nll_* reads its targets (Rust's saturating cast): NaN and negatives are 0, the fraction is dropped
__device__ __forceinline__ long long emb_read_id(float t) {
    if (!(t > 0.f)) return 0;
    if (t >= 9.2233720368547758e18f) return 0x7fffffffffffffffLL;
    return (long long)t;
}
// the row of id `f` inside the slab [v0, v0 + S), or -1: another slab's, >= V, or the padding id
__device__ __forceinline__ int emb_slab_row(float f, int V, long long pad, int v0, int S) {
    const long long id = emb_read_id(f);
    if (id >= V || id == pad) return -1;
    const long long r = id - v0;
    return r >= 0 && r < S ? (int)r : -1;
}

template <typename T> __device__ __forceinline__ T emb_zero();
template <> __device__ __forceinline__ float emb_zero<float>() { return 0.f; }
template <> __device__ __forceinline__ float4 emb_zero<float4>() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float emb_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 emb_add(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// out[t, :] = weight[idx[t], :], a zero row for an id >= V.  DV = D in units of T.
template <typename T>
__global__ void __launch_bounds__(256) emb_gather_kernel(const T* __restrict__ w, const float* __restrict__ idx, T* __restrict__ out, long long n,
                                                         int V, int DV, int lpr) {
    const int lane = threadIdx.x & 63, sub = lane & (lpr - 1), rin = lane / lpr, rpw = 64 / lpr;
    const long long waves = (long long)gridDim.x * 4, wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    for (long long t0 = wave * rpw; t0 < n; t0 += waves * rpw) {
        const long long t = t0 + rin;
        if (t >= n) continue;
        const long long id = emb_read_id(idx[t]);
        const bool hit = id < V;
        const T* __restrict__ src = w + (size_t)(hit ? id : 0) * DV;
        T* __restrict__ dst = out + (size_t)t * DV;
        for (int q = sub; q < DV; q += 4 * lpr) {
            T r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = hit && q + u * lpr < DV ? src[q + u * lpr] : emb_zero<T>();
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (q + u * lpr < DV) dst[q + u * lpr] = r[u];
        }
    }
}

__device__ __forceinline__ int emb_wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// sums of a pair of integers over a 1024-thread block, in every thread; red: 32 ints
__device__ __forceinline__ int2 emb_block_sum2(int a, int b, int* red) {
    a = emb_wave_sum_i(a);
    b = emb_wave_sum_i(b);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) {
        red[wid] = a;
        red[16 + wid] = b;
    }
    __syncthreads();
    int ra = 0, rb = 0;
#pragma unroll
    for (int i = 0; i < EMB_INDEX_THREADS / 64; ++i) {
        ra += red[i];
        rb += red[16 + i];
    }
    return make_int2(ra, rb);
}
__device__ __forceinline__ int emb_chunks_of(int len) { return len > EMB_CHUNK ? (len + EMB_CHUNK - 1) / EMB_CHUNK : 0; }

// Index, first launch: counts[v] for the rows of this block's slab and slab_tot[slab] = {tokens, listed chunks}.
__global__ void __launch_bounds__(EMB_INDEX_THREADS) emb_index_count_kernel(const float* __restrict__ idx, int n, int V, int S, long long pad,
                                                                            int* __restrict__ counts, int2* __restrict__ slab_tot) {
    __shared__ int cnt[EMB_SLAB_MAX];
    __shared__ int red[32];
    const int tid = threadIdx.x, v0 = blockIdx.x * S;
    for (int r = tid; r < S; r += EMB_INDEX_THREADS) cnt[r] = 0;
    __syncthreads();
    for (int t = tid; t < n; t += 4 * EMB_INDEX_THREADS) {
        int r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int tu = t + u * EMB_INDEX_THREADS;
            r[u] = tu < n ? emb_slab_row(idx[tu], V, pad, v0, S) : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (r[u] >= 0) atomicAdd(&cnt[r[u]], 1);
    }
    __syncthreads();
    int tok = 0, lch = 0;
    for (int r = tid; r < S && v0 + r < V; r += EMB_INDEX_THREADS) {
        const int c = cnt[r];
        counts[v0 + r] = c;
        tok += c;
        lch += emb_chunks_of(c);
    }
    const int2 tot = emb_block_sum2(tok, lch, red);
    if (tid == 0) slab_tot[blockIdx.x] = tot;
}

// Index, second launch: row_start[V + 1], perm[n'] (n' = tokens kept; each row's positions ascending), list[nlong] = {row, chunk} of
// every chunk of every row longer than EMB_CHUNK, rows ascending, chunks ascending.
__global__ void __launch_bounds__(EMB_INDEX_THREADS) emb_index_place_kernel(const float* __restrict__ idx, int n, int V, int S, long long pad,
                                                                            const int* __restrict__ counts, const int2* __restrict__ slab_tot,
                                                                            int* __restrict__ row_start, int* __restrict__ perm,
                                                                            int2* __restrict__ list, int list_cap, int* __restrict__ nlong) {
    __shared__ int cursor[EMB_SLAB_MAX];
    __shared__ int lt[EMB_TILE];
    __shared__ int lr[EMB_TILE];
    __shared__ int red[32];
    __shared__ int wsum[2][EMB_INDEX_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, v0 = blockIdx.x * S;
    int a = 0, b = 0;
    for (int s = tid; s < (int)blockIdx.x; s += EMB_INDEX_THREADS) {
        const int2 x = slab_tot[s];
        a += x.x;
        b += x.y;
    }
    const int2 base = emb_block_sum2(a, b, red);
    // exclusive scan of the slab's counts: a thread owns rows 4 tid .. 4 tid + 3
    int c[4], nc[4], ts = 0, ls = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 4 * tid + j;
        c[j] = r < S && v0 + r < V ? counts[v0 + r] : 0;
        nc[j] = emb_chunks_of(c[j]);
        ts += c[j];
        ls += nc[j];
    }
    int it = ts, il = ls;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int x = __shfl_up(it, off, 64), y = __shfl_up(il, off, 64);
        if (lane >= off) {
            it += x;
            il += y;
        }
    }
    if (lane == 63) {
        wsum[0][wid] = it;
        wsum[1][wid] = il;
    }
    __syncthreads();
    int wt = 0, wl = 0, tt = 0, tl = 0;
#pragma unroll
    for (int i = 0; i < EMB_INDEX_THREADS / 64; ++i) {
        if (i < wid) {
            wt += wsum[0][i];
            wl += wsum[1][i];
        }
        tt += wsum[0][i];
        tl += wsum[1][i];
    }
    int et = base.x + wt + it - ts, el = base.y + wl + il - ls;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 4 * tid + j;
        if (r < S && v0 + r < V) {
            row_start[v0 + r] = et;
            cursor[r] = et;
            for (int q = 0; q < nc[j]; ++q)
                if (el + q < list_cap) list[el + q] = make_int2(v0 + r, q);
            et += c[j];
            el += nc[j];
        }
    }
    if (blockIdx.x == gridDim.x - 1 && tid == 0) {
        row_start[V] = base.x + tt;
        *nlong = base.y + tl < list_cap ? base.y + tl : list_cap;
    }
    if (tt == 0) return;  // no token selects a row of this slab (the same decision in every thread)
    for (int tile = 0; tile < n; tile += EMB_TILE) {
        int rr[4], mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = tile + 4 * tid + j;
            rr[j] = t < n ? emb_slab_row(idx[t], V, pad, v0, S) : -1;
            mine += rr[j] >= 0;
        }
        int inc = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int x = __shfl_up(inc, off, 64);
            if (lane >= off) inc += x;
        }
        __syncthreads();  // the placing wave is done with the previous tile's list
        if (lane == 63) wsum[0][wid] = inc;
        __syncthreads();
        int at = inc - mine, total = 0;
#pragma unroll
        for (int i = 0; i < EMB_INDEX_THREADS / 64; ++i) {
            if (i < wid) at += wsum[0][i];
            total += wsum[0][i];
        }
        if (total == 0) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (rr[j] >= 0) {
                lt[at] = tile + 4 * tid + j;
                lr[at] = rr[j];
                ++at;
            }
        __syncthreads();
        if (wid != 0) continue;
        // one wave places the tile's tokens, 64 at a time in list (= token) order: tokens of one row take consecutive slots in lane order
        for (int g0 = 0; g0 < total; g0 += 64) {
            const int e = g0 + lane;
            const bool on = e < total;
            const int r = on ? lr[e] : -1, t = on ? lt[e] : 0;
            unsigned long long todo = __ballot(on);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const int lrow = __shfl(r, leader, 64);
                const bool same = on && r == lrow;
                const unsigned long long group = __ballot(same);
                const int slot = cursor[lrow];
                if (same) {
                    const int pos = slot + __popcll(group & ((1ull << lane) - 1ull));
                    if (pos < n) perm[pos] = t;
                }
                if (lane == leader) cursor[lrow] = slot + __popcll(group);
                todo &= ~group;
            }
        }
    }
}

// acc[k] (columns q0 + k lpr) = the sum of the gradient rows perm[s .. e), e > s, in that order, starting from the first row itself.
// Four rows' loads are issued before the first of them is added, the next four positions with them.
template <typename T>
__device__ __forceinline__ void emb_segment_sum(T (&acc)[4], const T* __restrict__ g, const int* __restrict__ perm, int s, int e, int DV, int q0,
                                                int lpr) {
    {
        const T* __restrict__ row = g + (size_t)perm[s] * DV;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = q0 + k * lpr < DV ? row[q0 + k * lpr] : emb_zero<T>();
    }
    int tk[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) tk[j] = perm[s + 1 + j < e ? s + 1 + j : e - 1];
    for (int i = s + 1; i < e; i += 4) {
        int nx[4];  // the next four positions, fetched under this group's row loads
#pragma unroll
        for (int j = 0; j < 4; ++j) nx[j] = perm[i + 4 + j < e ? i + 4 + j : e - 1];
        T r[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const T* __restrict__ row = g + (size_t)tk[j] * DV;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[j][k] = q0 + k * lpr < DV ? row[q0 + k * lpr] : emb_zero<T>();
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j < e) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = emb_add(acc[k], r[j][k]);
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) tk[j] = nx[j];
    }
}

// One owner (lpr lanes) per (table row, 4 lpr columns): rows of at most EMB_CHUNK tokens.  Empty rows: nothing (+=), zeros (assign).
template <typename T, bool ASSIGN>
__global__ void __launch_bounds__(256) emb_rowsum_kernel(T* __restrict__ dw, const T* __restrict__ g, const int* __restrict__ row_start,
                                                         const int* __restrict__ perm, int V, int DV, int lpr, int colchunks) {
    const int lane = threadIdx.x & 63, sub = lane & (lpr - 1), rin = lane / lpr, rpw = 64 / lpr;
    const long long waves = (long long)gridDim.x * 4, wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long items = (long long)V * colchunks;
    for (long long i0 = wave * rpw; i0 < items; i0 += waves * rpw) {
        const long long item = i0 + rin;
        if (item >= items) continue;
        const int v = (int)(item / colchunks), q0 = (int)(item % colchunks) * 4 * lpr + sub;
        const int s = row_start[v], e = row_start[v + 1];
        if (e - s > EMB_CHUNK || (e == s && !ASSIGN)) continue;
        T acc[4] = {emb_zero<T>(), emb_zero<T>(), emb_zero<T>(), emb_zero<T>()};
        if (e > s) emb_segment_sum<T>(acc, g, perm, s, e, DV, q0, lpr);
        T* __restrict__ dst = dw + (size_t)v * DV;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (q0 + k * lpr < DV) dst[q0 + k * lpr] = ASSIGN ? acc[k] : emb_add(dst[q0 + k * lpr], acc[k]);
    }
}

// One owner per (listed chunk, 4 lpr columns): partial[k, :] = the ordered sum of chunk list[k] of its row.
template <typename T>
__global__ void __launch_bounds__(256) emb_chunksum_kernel(T* __restrict__ partial, const T* __restrict__ g, const int* __restrict__ row_start,
                                                           const int* __restrict__ perm, const int2* __restrict__ list,
                                                           const int* __restrict__ nlong, int DV, int lpr, int colchunks) {
    const int lane = threadIdx.x & 63, sub = lane & (lpr - 1), rin = lane / lpr, rpw = 64 / lpr;
    const long long waves = (long long)gridDim.x * 4, wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long items = (long long)*nlong * colchunks;
    for (long long i0 = wave * rpw; i0 < items; i0 += waves * rpw) {
        const long long item = i0 + rin;
        if (item >= items) continue;
        const int k = (int)(item / colchunks), q0 = (int)(item % colchunks) * 4 * lpr + sub;
        const int2 vc = list[k];
        const int s = row_start[vc.x] + vc.y * EMB_CHUNK, end = row_start[vc.x + 1], e = s + EMB_CHUNK < end ? s + EMB_CHUNK : end;
        T acc[4];
        emb_segment_sum<T>(acc, g, perm, s, e, DV, q0, lpr);
        T* __restrict__ dst = partial + (size_t)k * DV;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q0 + j * lpr < DV) dst[q0 + j * lpr] = acc[j];
    }
}

// One owner per (row longer than EMB_CHUNK, 4 lpr columns): the row's partials added in chunk order, starting from the first.
template <typename T, bool ASSIGN>
__global__ void __launch_bounds__(256) emb_chunkadd_kernel(T* __restrict__ dw, const T* __restrict__ partial, const int* __restrict__ row_start,
                                                           const int2* __restrict__ list, const int* __restrict__ nlong, int DV, int lpr,
                                                           int colchunks) {
    const int lane = threadIdx.x & 63, sub = lane & (lpr - 1), rin = lane / lpr, rpw = 64 / lpr;
    const long long waves = (long long)gridDim.x * 4, wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int nl = *nlong;
    const long long items = (long long)nl * colchunks;
    for (long long i0 = wave * rpw; i0 < items; i0 += waves * rpw) {
        const long long item = i0 + rin;
        if (item >= items) continue;
        const int k = (int)(item / colchunks), q0 = (int)(item % colchunks) * 4 * lpr + sub;
        const int2 vc = list[k];
        if (vc.y != 0) continue;  // the row's first chunk leads
        int nch = emb_chunks_of(row_start[vc.x + 1] - row_start[vc.x]);
        if (nch > nl - k) nch = nl - k;
        T acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = q0 + j * lpr < DV ? partial[(size_t)k * DV + q0 + j * lpr] : emb_zero<T>();
#pragma unroll 4
        for (int c = 1; c < nch; ++c) {
            const T* __restrict__ row = partial + (size_t)(k + c) * DV;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (q0 + j * lpr < DV) acc[j] = emb_add(acc[j], row[q0 + j * lpr]);
        }
        T* __restrict__ dst = dw + (size_t)vc.x * DV;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q0 + j * lpr < DV) dst[q0 + j * lpr] = ASSIGN ? acc[j] : emb_add(dst[q0 + j * lpr], acc[j]);
    }
}

// lanes per row: the power of two that gives a lane four accesses (one, two ... for narrow rows), 64 at most
struct emb_geometry {
    int DV, lpr, colchunks;
};
emb_geometry emb_geometry_of(int D, bool vec) {
    emb_geometry s;
    s.DV = vec ? D / 4 : D;
    s.lpr = 1;
    while (s.lpr < 64 && s.lpr * 4 < s.DV) s.lpr *= 2;
    s.colchunks = (s.DV + 4 * s.lpr - 1) / (4 * s.lpr);
    return s;
}
unsigned emb_grid(long long items, int lpr) {
    const long long per_block = 4 * (64 / lpr), b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > EMB_MAX_BLOCKS ? EMB_MAX_BLOCKS : b));
}
size_t emb_round256(size_t b) { return (b + 255) & ~(size_t)255; }

int emb_check(nk_device* dev, const void* a, const void* b, const void* idx, long long n, int V, int D, const char* what) {
    NK_CHECK(dev != nullptr, "null device handle");
    NK_CHECK(n >= 0 && n <= EMB_MAX_N, "%s: n must be in 0 .. 2^30, got %lld", what, n);
    NK_CHECK(V >= 1 && V <= EMB_MAX_V, "%s: num_embeddings must be in 1 .. 2^24 (ids are stored as f32), got %d", what, V);
    NK_CHECK(D >= 1 && D <= EMB_MAX_D, "%s: embedding_dim must be in 1 .. 2^24, got %d", what, D);
    NK_CHECK(a != nullptr && (n == 0 || (b != nullptr && idx != nullptr)), "%s: null pointer", what);
    return NK_OK;
}

template <typename T, bool ASSIGN>
int emb_bwd_launch(nk_device* dev, float* dweight, const float* g, const float* idx, int n, int V, int D, long long pad) {
    const emb_geometry s = emb_geometry_of(D, sizeof(T) == 16);
    const int S = V / 512 + 1 < 32 ? 32 : (V / 512 + 1 > EMB_SLAB_MAX ? EMB_SLAB_MAX : V / 512 + 1), slabs = (V + S - 1) / S;
    const bool chunked = n > EMB_CHUNK;                 // a row longer than one chunk is possible
    const int list_cap = chunked ? 2 * (n / EMB_CHUNK) + 1 : 0;  // a long row of L tokens has at most 2 L / EMB_CHUNK chunks
    // workspace: counts[V] | row_start[V + 1] | slab_tot[slabs] | perm[n] | list[list_cap] | nlong | partial[list_cap][D]
    size_t off[8], at = 0;
    const size_t sizes[7] = {(size_t)V * 4, ((size_t)V + 1) * 4, (size_t)slabs * 8, (size_t)n * 4, (size_t)list_cap * 8, 4, (size_t)list_cap * D * 4};
    for (int i = 0; i < 7; ++i) {
        off[i] = at;
        at += emb_round256(sizes[i] ? sizes[i] : 1);
    }
    void* ws = nullptr;
    if (int rc = nk_workspace(dev, at, &ws)) return rc;
    char* base = static_cast<char*>(ws);
    int* counts = reinterpret_cast<int*>(base + off[0]);
    int* row_start = reinterpret_cast<int*>(base + off[1]);
    int2* slab_tot = reinterpret_cast<int2*>(base + off[2]);
    int* perm = reinterpret_cast<int*>(base + off[3]);
    int2* list = reinterpret_cast<int2*>(base + off[4]);
    int* nlong = reinterpret_cast<int*>(base + off[5]);
    T* partial = reinterpret_cast<T*>(base + off[6]);
    hipLaunchKernelGGL(emb_index_count_kernel, dim3(slabs), dim3(EMB_INDEX_THREADS), 0, dev->compute, idx, n, V, S, pad, counts, slab_tot);
    NK_LAUNCH_CHECK();
    hipLaunchKernelGGL(emb_index_place_kernel, dim3(slabs), dim3(EMB_INDEX_THREADS), 0, dev->compute, idx, n, V, S, pad, counts, slab_tot, row_start,
                       perm, list, list_cap, nlong);
    NK_LAUNCH_CHECK();
    T* dw = reinterpret_cast<T*>(dweight);
    const T* gt = reinterpret_cast<const T*>(g);
    hipLaunchKernelGGL((emb_rowsum_kernel<T, ASSIGN>), dim3(emb_grid((long long)V * s.colchunks, s.lpr)), dim3(256), 0, dev->compute, dw, gt,
                       row_start, perm, V, s.DV, s.lpr, s.colchunks);
    NK_LAUNCH_CHECK();
    if (chunked) {
        const unsigned grid = emb_grid((long long)list_cap * s.colchunks, s.lpr);
        hipLaunchKernelGGL((emb_chunksum_kernel<T>), dim3(grid), dim3(256), 0, dev->compute, partial, gt, row_start, perm, list, nlong, s.DV, s.lpr,
                           s.colchunks);
        NK_LAUNCH_CHECK();
        hipLaunchKernelGGL((emb_chunkadd_kernel<T, ASSIGN>), dim3(grid), dim3(256), 0, dev->compute, dw, partial, row_start, list, nlong, s.DV,
                           s.lpr, s.colchunks);
        NK_LAUNCH_CHECK();
    }
    return NK_OK;
}

template <bool ASSIGN>
int emb_bwd(nk_device* dev, float* dweight, const float* g, const float* idx, long long n, int V, int D, long long padding_idx) {
    const char* what = ASSIGN ? "nk_embedding_bwd_assign" : "nk_embedding_bwd";
    if (int rc = emb_check(dev, dweight, g, idx, n, V, D, what)) return rc;
    NK_USE(dev);
    if (n == 0) {  // nothing to add; the first-write form still covers its destination
        if (ASSIGN) NK_HIP(hipMemsetAsync(dweight, 0, (size_t)V * D * sizeof(float), dev->compute));
        return NK_OK;
    }
    const long long pad = padding_idx < 0 ? -1 : padding_idx;
    if (D % 4 == 0 && emb_al16(dweight) && emb_al16(g)) return emb_bwd_launch<float4, ASSIGN>(dev, dweight, g, idx, (int)n, V, D, pad);
    return emb_bwd_launch<float, ASSIGN>(dev, dweight, g, idx, (int)n, V, D, pad);
}

}  // namespace

extern "C" {

int nk_embedding_fwd(nk_device* dev, const float* weight, const float* idx, float* out, long long n, int V, int D) {
    if (int rc = emb_check(dev, weight, out, idx, n, V, D, "nk_embedding_fwd")) return rc;
    NK_USE(dev);
    if (n == 0) return NK_OK;
    const bool vec = D % 4 == 0 && emb_al16(weight) && emb_al16(out);
    const emb_geometry s = emb_geometry_of(D, vec);
    const dim3 grid(emb_grid(n, s.lpr)), block(256);
    if (vec)
        hipLaunchKernelGGL((emb_gather_kernel<float4>), grid, block, 0, dev->compute, reinterpret_cast<const float4*>(weight), idx,
                           reinterpret_cast<float4*>(out), n, V, s.DV, s.lpr);
    else
        hipLaunchKernelGGL((emb_gather_kernel<float>), grid, block, 0, dev->compute, weight, idx, out, n, V, s.DV, s.lpr);
    NK_LAUNCH_CHECK();
    return NK_OK;
}

int nk_embedding_bwd(nk_device* dev, float* dweight, const float* g, const float* idx, long long n, int V, int D, long long padding_idx) {
    return emb_bwd<false>(dev, dweight, g, idx, n, V, D, padding_idx);
}

int nk_embedding_bwd_assign(nk_device* dev, float* dweight, const float* g, const float* idx, long long n, int V, int D, long long padding_idx) {
    return emb_bwd<true>(dev, dweight, g, idx, n, V, D, padding_idx);
}

}  // extern "C"
