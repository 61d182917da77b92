// MoE token routing for gfx950: fused top-k + gates, and a stable counting
// sort of the (token, expert) pairs by expert. Replaces the torch chain of
// SparseMoE.forward (reference moe/base.py:96-127): topk, fp32 softmax,
// bincount, sort, floor-divide, gather and the index-put that builds `inv`,
// and the autograd chain behind them.
//
// The problem is tiny and regular: T*k pairs with keys in [0, E), E <= 64.
// Forward is three launches over 128-token tiles:
//   1. topk    — a lane group of W = pow2 >= E lanes owns a token (64/W tokens
//                per wave), one logit per lane in a register; k rounds of a
//                group arg-max through DPP / cross-row shuffles; fp32 softmax
//                over the k winners; per-tile expert histogram in LDS.
//   2. scan    — one workgroup: expert totals, their exclusive scan (offsets),
//                then each expert's exclusive scan over the tiles, which turns
//                the histogram in place into the tile's first slot per expert.
//   3. scatter — each tile walks its pairs in ascending pair order; a pair's
//                slot is the tile base plus its rank among the tile's earlier
//                pairs of the same expert (wave ballots + popcounts, per-wave
//                counts and a running per-expert base in LDS).
// No slot comes from an atomic counter and no float goes through an atomic,
// so the result is the stable sort's, bitwise reproducible. The only atomics
// are integer LDS adds into the histogram, whose sum has no order.
//
// Backward is one launch, a lane group per token again: it recomputes the
// fp32 gates from the k selected logits with the forward's own expression
// and writes the whole d_logits row, zeros included.

#include "common.h"

#include <math.h>

namespace {

constexpr int RT_TILE = 128;     // tokens per tile
constexpr int RT_THREADS = 256;  // topk / scatter / bwd workgroup
constexpr int RT_WAVES = RT_THREADS / WAVE;
constexpr int RT_MAXE = 64;
constexpr int RT_MAXK = 8;
constexpr int RT_SCAN_THREADS = 1024;

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}

// One butterfly step of the arg-max: keep the larger value, the lower index
// on equal values. (value, index) is a total order, so every lane of the
// group ends on the same pair whatever the step order.
__device__ __forceinline__ void argmax_take(float& v, int& i, float ov, int oi) {
    bool take = ov > v || (ov == v && oi < i);
    v = take ? ov : v;
    i = take ? oi : i;
}

template <int CTRL>
__device__ __forceinline__ void argmax_dpp(float& v, int& i) {
    float ov = __int_as_float(dpp_i32<CTRL>(__float_as_int(v)));
    int oi = dpp_i32<CTRL>(i);
    argmax_take(v, i, ov, oi);
}

__device__ __forceinline__ void argmax_xor(float& v, int& i, int off) {
    float ov = __shfl_xor(v, off, WAVE);
    int oi = __shfl_xor(i, off, WAVE);
    argmax_take(v, i, ov, oi);
}

// All-reduce over aligned groups of W lanes. Inside a 16-lane row the steps
// are DPP (pure VALU): quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror, row_mirror; rows are joined by two shuffles.
template <int W>
__device__ __forceinline__ void group_argmax(float& v, int& i) {
    if (W >= 2) argmax_dpp<0xB1>(v, i);
    if (W >= 4) argmax_dpp<0x4E>(v, i);
    if (W >= 8) argmax_dpp<0x141>(v, i);
    if (W >= 16) argmax_dpp<0x140>(v, i);
    if (W >= 32) argmax_xor(v, i, 16);
    if (W >= 64) argmax_xor(v, i, 32);
}

__device__ __forceinline__ float route_logit(float x) {
    return x == x ? x : -INFINITY;  // NaN routing is unspecified; keep it ordered
}

// fp32 softmax over the k selected logits, v[0] the largest. Forward and
// backward share it, so the backward's weights are the forward's before
// their rounding to the logits' dtype.
__device__ __forceinline__ void route_gates(const float (&v)[RT_MAXK], int k, float (&w)[RT_MAXK]) {
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < RT_MAXK; ++j) {
        w[j] = j < k ? expf(v[j] - v[0]) : 0.f;
        sum += w[j];
    }
#pragma unroll
    for (int j = 0; j < RT_MAXK; ++j) w[j] = w[j] / sum;
}

__device__ __forceinline__ int wave_incl_scan_i32(int x, int lane) {
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        int n = __shfl_up(x, d, WAVE);
        if (lane >= d) x += n;
    }
    return x;
}

// ---------------------------------------------------------------------------
// 1. top-k, gates, per-tile expert histogram
// ---------------------------------------------------------------------------
template <typename T, int W>
__global__ void __launch_bounds__(RT_THREADS) moe_route_topk_kernel(
    const T* __restrict__ logits, int32_t* __restrict__ selected, T* __restrict__ gates,
    int32_t* __restrict__ tile_counts, int64_t Tn, int E, int k) {
    constexpr int TPP = RT_THREADS / W;  // tokens per pass of the workgroup
    constexpr int PASSES = RT_TILE / TPP;
    static_assert(W >= 2 && W <= 64 && PASSES >= 1, "lane group width");

    __shared__ int cnt[RT_MAXE];
    const int tid = threadIdx.x;
    if (tid < RT_MAXE) cnt[tid] = 0;
    __syncthreads();

    const int e = tid & (W - 1);
    const int64_t t0 = (int64_t)blockIdx.x * RT_TILE + tid / W;

    auto fetch = [&](int pass) -> float {
        int64_t t = t0 + pass * TPP;
        if (e < E && t < Tn) return route_logit(load_as_f32<T>(logits + t * E + e));
        return -INFINITY;
    };

    float nxt = fetch(0);
    for (int pass = 0; pass < PASSES; ++pass) {
        if ((int64_t)blockIdx.x * RT_TILE + pass * TPP >= Tn) break;  // uniform
        float cv = nxt;
        if (pass + 1 < PASSES) nxt = fetch(pass + 1);  // in flight during the rounds
        const int64_t t = t0 + pass * TPP;

        // pad lanes (e >= E) and lanes already chosen sort after every live
        // expert: there is always one, since k <= E
        int ci = e < E ? e : RT_MAXE + e;
        float v[RT_MAXK];
        int s[RT_MAXK];
#pragma unroll
        for (int j = 0; j < RT_MAXK; ++j) {
            v[j] = 0.f;
            s[j] = 0;
            if (j < k) {
                float bv = cv;
                int bi = ci;
                group_argmax<W>(bv, bi);
                v[j] = bv;
                s[j] = bi;
                if (bi == e) {
                    cv = -INFINITY;
                    ci = 2 * RT_MAXE + e;
                }
            }
        }
        float w[RT_MAXK];
        route_gates(v, k, w);
        // lane j of the group stores pair j
#pragma unroll
        for (int j = 0; j < RT_MAXK; ++j) {
            if (j < k && e == j && t < Tn) {
                selected[t * k + j] = s[j];
                store_from_f32<T>(gates + t * k + j, w[j]);
                atomicAdd(&cnt[s[j]], 1);
            }
        }
    }
    __syncthreads();
    if (tid < E) tile_counts[(size_t)blockIdx.x * E + tid] = cnt[tid];
}

// ---------------------------------------------------------------------------
// 2. scan: counts[tile][e] -> first slot of (tile, e); totals and offsets
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(RT_SCAN_THREADS) moe_route_scan_kernel(
    int32_t* __restrict__ scratch, int64_t* __restrict__ num_tokens_per_expert,
    int32_t* __restrict__ offsets, int ntiles, int E) {
    __shared__ int tot[RT_MAXE];
    __shared__ int off[RT_MAXE];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    constexpr int NW = RT_SCAN_THREADS / WAVE;

    for (int e = wave; e < E; e += NW) {
        int s = 0;
        for (int tile = lane; tile < ntiles; tile += WAVE) s += scratch[(size_t)tile * E + e];
        s = wave_incl_scan_i32(s, lane);
        if (lane == WAVE - 1) tot[e] = s;
    }
    __syncthreads();
    if (wave == 0) {
        int c = lane < E ? tot[lane] : 0;
        int inc = wave_incl_scan_i32(c, lane);
        if (lane < E) {
            off[lane] = inc - c;
            offsets[lane] = inc - c;
            num_tokens_per_expert[lane] = c;
        }
        if (lane == E - 1) offsets[E] = inc;
    }
    __syncthreads();
    for (int e = wave; e < E; e += NW) {
        int carry = off[e];
        for (int b0 = 0; b0 < ntiles; b0 += WAVE) {
            const int tile = b0 + lane;
            int c = tile < ntiles ? scratch[(size_t)tile * E + e] : 0;
            int inc = wave_incl_scan_i32(c, lane);
            if (tile < ntiles) scratch[(size_t)tile * E + e] = carry + inc - c;
            carry += __shfl(inc, WAVE - 1, WAVE);
        }
    }
}

// ---------------------------------------------------------------------------
// 3. stable scatter
// ---------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(RT_THREADS) moe_route_scatter_kernel(
    const int32_t* __restrict__ selected, const T* __restrict__ gates,
    const int32_t* __restrict__ tile_base, int32_t* __restrict__ inv,
    int64_t* __restrict__ batch_index, T* __restrict__ batch_gates,
    int64_t n_pairs, int E, int k) {
    __shared__ int base[RT_MAXE];               // next free slot per expert
    __shared__ int wave_cnt[RT_WAVES][RT_MAXE];  // this chunk's pairs per (wave, expert)
    const int tid = threadIdx.x;
    const int lane = tid & (WAVE - 1);
    const int wave = tid / WAVE;

    if (tid < RT_MAXE) base[tid] = tid < E ? tile_base[(size_t)blockIdx.x * E + tid] : 0;

    const int tile_pairs = RT_TILE * k;
    const int64_t p0 = (int64_t)blockIdx.x * tile_pairs;
    for (int c0 = 0; c0 < tile_pairs; c0 += RT_THREADS) {
        if (p0 + c0 >= n_pairs) break;  // uniform
        wave_cnt[tid / RT_MAXE][tid % RT_MAXE] = 0;
        __syncthreads();  // also orders the base[] init / update before its readers

        const int64_t p = p0 + c0 + tid;
        const bool valid = c0 + tid < tile_pairs && p < n_pairs;
        const int e = valid ? selected[p] : 0;
        // lanes of this wave holding the same expert
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            const bool bit = (e >> b) & 1;
            unsigned long long m = __ballot(valid && bit);
            same &= bit ? m : ~m;
        }
        int rank = 0;
        if (valid) {
            rank = __popcll(same & ((1ull << lane) - 1ull));
            if ((same >> lane) == 1ull) wave_cnt[wave][e] = rank + 1;  // highest lane of the set
        }
        __syncthreads();
        if (valid) {
            int slot = base[e] + rank;
            for (int w = 0; w < wave; ++w) slot += wave_cnt[w][e];
            inv[p] = slot;
            batch_index[slot] = p / k;
            batch_gates[slot] = gates[p];
        }
        __syncthreads();
        if (tid < RT_MAXE) {
            int add = 0;
#pragma unroll
            for (int w = 0; w < RT_WAVES; ++w) add += wave_cnt[w][tid];
            base[tid] += add;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// 4. backward
// ---------------------------------------------------------------------------
template <typename T, int W>
__global__ void __launch_bounds__(RT_THREADS) moe_route_bwd_kernel(
    const T* __restrict__ d_batch_gates, const int32_t* __restrict__ inv,
    const int32_t* __restrict__ selected, const T* __restrict__ logits,
    T* __restrict__ d_logits, int64_t Tn, int E, int k) {
    constexpr int TPB = RT_THREADS / W;
    const int e = threadIdx.x & (W - 1);
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x / W;
    if (t >= Tn || e >= E) return;
    const int64_t last = Tn * k - 1;

    // every lane of the group reads the same k triples (one broadcast each)
    float v[RT_MAXK], g[RT_MAXK];
    int s[RT_MAXK];
#pragma unroll
    for (int j = 0; j < RT_MAXK; ++j) {
        v[j] = 0.f;
        g[j] = 0.f;
        s[j] = -1;
        if (j < k) {
            s[j] = min(max(selected[t * k + j], 0), E - 1);
            int64_t slot = min(max((int64_t)inv[t * k + j], (int64_t)0), last);
            v[j] = route_logit(load_as_f32<T>(logits + t * E + s[j]));
            g[j] = load_as_f32<T>(d_batch_gates + slot);
        }
    }
    float w[RT_MAXK];
    route_gates(v, k, w);
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < RT_MAXK; ++j) dot = fmaf(w[j], g[j], dot);
    float out = 0.f;
#pragma unroll
    for (int j = 0; j < RT_MAXK; ++j)
        if (s[j] == e) out = w[j] * (g[j] - dot) + 0.f;  // + 0: an exact zero is +0
    store_from_f32<T>(d_logits + t * E + e, out);
}

int route_check(int64_t T, int E, int k, int dtype) {
    if (dtype != DOLOMITE_F32 && dtype != DOLOMITE_BF16) return 9050;
    if (E < 1 || E > RT_MAXE || k < 1 || k > RT_MAXK || k > E) return 9051;
    if (T < 0 || T > (int64_t)INT32_MAX / k) return 9052;
    return 0;
}

inline int route_group_width(int E) {
    int W = 2;
    while (W < E) W <<= 1;
    return W;
}

template <typename T, int W>
void launch_topk(hipStream_t st, int ntiles, const void* logits, int32_t* selected, void* gates,
                 int32_t* scratch, int64_t Tn, int E, int k) {
    hipLaunchKernelGGL((moe_route_topk_kernel<T, W>), dim3(ntiles), dim3(RT_THREADS), 0, st,
                       (const T*)logits, selected, (T*)gates, scratch, Tn, E, k);
}

template <typename T, int W>
void launch_bwd(hipStream_t st, const void* dbg, const int32_t* inv, const int32_t* selected,
                const void* logits, void* d_logits, int64_t Tn, int E, int k) {
    constexpr int TPB = RT_THREADS / W;
    hipLaunchKernelGGL((moe_route_bwd_kernel<T, W>), dim3((uint32_t)((Tn + TPB - 1) / TPB)), dim3(RT_THREADS), 0, st,
                       (const T*)dbg, inv, selected, (const T*)logits, (T*)d_logits, Tn, E, k);
}

// call F<T, W>(args...) for the lane-group width W of E
#define ROUTE_BY_WIDTH(F, T, W, ...)                    \
    switch (W) {                                        \
        case 2: F<T, 2>(__VA_ARGS__); break;            \
        case 4: F<T, 4>(__VA_ARGS__); break;            \
        case 8: F<T, 8>(__VA_ARGS__); break;            \
        case 16: F<T, 16>(__VA_ARGS__); break;          \
        case 32: F<T, 32>(__VA_ARGS__); break;          \
        default: F<T, 64>(__VA_ARGS__); break;          \
    }

}  // namespace

extern "C" int64_t dolomite_moe_route_scratch_ints(int64_t T, int E, int top_k) {
    if (route_check(T, E, top_k, DOLOMITE_BF16) != 0) return -1;
    return (T + RT_TILE - 1) / RT_TILE * E;
}

extern "C" int dolomite_moe_route_fwd(dolomite_stream_t stream, const void* logits,
                                      int32_t* selected, void* gates, int32_t* inv,
                                      int64_t* batch_index, void* batch_gates,
                                      int64_t* num_tokens_per_expert, int32_t* offsets,
                                      int32_t* scratch, int64_t T, int E, int top_k, int dtype) {
    if (int err = route_check(T, E, top_k, dtype)) return err;
    if (T == 0) return 0;
    if (scratch == nullptr) return 9053;
    hipStream_t st = (hipStream_t)stream;
    const int ntiles = (int)((T + RT_TILE - 1) / RT_TILE);
    const int W = route_group_width(E);
    if (dtype == DOLOMITE_BF16) {
        ROUTE_BY_WIDTH(launch_topk, uint16_t, W, st, ntiles, logits, selected, gates, scratch, T, E, top_k)
    } else {
        ROUTE_BY_WIDTH(launch_topk, float, W, st, ntiles, logits, selected, gates, scratch, T, E, top_k)
    }
    hipLaunchKernelGGL(moe_route_scan_kernel, dim3(1), dim3(RT_SCAN_THREADS), 0, st,
                       scratch, num_tokens_per_expert, offsets, ntiles, E);
    const int64_t n_pairs = T * top_k;
    if (dtype == DOLOMITE_BF16) {
        hipLaunchKernelGGL(moe_route_scatter_kernel<uint16_t>, dim3(ntiles), dim3(RT_THREADS), 0, st,
                           selected, (const uint16_t*)gates, scratch, inv, batch_index,
                           (uint16_t*)batch_gates, n_pairs, E, top_k);
    } else {
        hipLaunchKernelGGL(moe_route_scatter_kernel<float>, dim3(ntiles), dim3(RT_THREADS), 0, st,
                           selected, (const float*)gates, scratch, inv, batch_index,
                           (float*)batch_gates, n_pairs, E, top_k);
    }
    return dol_last_error();
}

// The first launch alone: selected and gates in pair order, for callers that
// need no expert sort (the decode MLP of moe_decode.hip).
extern "C" int dolomite_moe_route_topk(dolomite_stream_t stream, const void* logits,
                                       int32_t* selected, void* gates, int32_t* scratch,
                                       int64_t T, int E, int top_k, int dtype) {
    if (int err = route_check(T, E, top_k, dtype)) return err;
    if (T == 0) return 0;
    if (scratch == nullptr) return 9053;
    hipStream_t st = (hipStream_t)stream;
    const int ntiles = (int)((T + RT_TILE - 1) / RT_TILE);
    const int W = route_group_width(E);
    if (dtype == DOLOMITE_BF16) {
        ROUTE_BY_WIDTH(launch_topk, uint16_t, W, st, ntiles, logits, selected, gates, scratch, T, E, top_k)
    } else {
        ROUTE_BY_WIDTH(launch_topk, float, W, st, ntiles, logits, selected, gates, scratch, T, E, top_k)
    }
    return dol_last_error();
}

extern "C" int dolomite_moe_route_bwd(dolomite_stream_t stream, const void* d_batch_gates,
                                      const int32_t* inv, const int32_t* selected,
                                      const void* logits, void* d_logits,
                                      int64_t T, int E, int top_k, int dtype) {
    if (int err = route_check(T, E, top_k, dtype)) return err;
    if (T == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int W = route_group_width(E);
    if (dtype == DOLOMITE_BF16) {
        ROUTE_BY_WIDTH(launch_bwd, uint16_t, W, st, d_batch_gates, inv, selected, logits, d_logits, T, E, top_k)
    } else {
        ROUTE_BY_WIDTH(launch_bwd, float, W, st, d_batch_gates, inv, selected, logits, d_logits, T, E, top_k)
    }
    return dol_last_error();
}
