// dolomite_hip — normalization / RoPE / cross-entropy / AdamW kernels for
// gfx950 (MI355X). C-ABI entry points declared in include/dolomite_hip.h.
//
// These are the MI355X-native replacements for (reference call sites):
//   RMSNorm   : modeling_utils/normalization/rmsnorm/base.py:18-25 semantics
//               (the reference's Triton torchtitan kernels are NOT ported)
//   LayerNorm : nn.LayerNorm ('layernorm'/'torch' implementation)
//   RoPE      : position_embedding/rope.py:104-121 applied at
//               attention/padding_free.py:38-40 on the packed c_attn layout
//   CE        : F.cross_entropy at model_wrapper/pretraining.py:125 /
//               gpt_dolomite/main.py:200
//   AdamW     : torch.optim.AdamW (optimization/optimizer.py:74)
//
// All HBM-bound: the design rules are coalesced wide loads (bf16x8 /
// float4), fp32 accumulation, one LDS stash per row to avoid re-reads.

#include "common.h"

#include <math.h>

#include <type_traits>

// ===========================================================================
// Host-side kernel selectors: each turns run-time arguments into the tags of
// one kernel instantiation and calls fn with them once; fn launches and
// returns the entry point's code. Every launch below goes through these, so
// its argument list is written once, with casts to the selected T.
// ===========================================================================

template <int N>
using Int = std::integral_constant<int, N>;

// fn(std::true_type / std::false_type)
template <typename Fn>
static int select_bool(bool b, Fn fn) {
    return b ? fn(std::true_type{}) : fn(std::false_type{});
}

// fn(T{}): uint16_t for DOLOMITE_BF16, float for any other dtype.
template <typename Fn>
static int select_dtype(int dtype, Fn fn) {
    return dtype == DOLOMITE_BF16 ? fn(uint16_t{}) : fn(float{});
}

// fn(T{}, Int<V>{}): the 16-byte vector width (8 bf16 / 4 fp32) when the
// extent n is a multiple of it, the scalar V=1 instantiation otherwise.
template <typename Fn>
static int select_dtype_vec(int dtype, int64_t n, Fn fn) {
    return select_dtype(dtype, [&](auto t) {
        constexpr int W = 16 / (int)sizeof(t);
        return n % W == 0 ? fn(t, Int<W>{}) : fn(t, Int<1>{});
    });
}

// fn(T{}, Int<V>{}, Int<ITMAX>{}) for a norm row of H elements: the smallest
// ITMAX bucket covering the ceil(H / (64*V)) vectors each lane owns, or 9002
// (without calling fn) for a row wider than 16 * 64 * V.
template <typename Fn>
static int select_norm(int dtype, int64_t H, Fn fn) {
    return select_dtype_vec(dtype, H, [&](auto t, auto v) {
        int it = ((int)H + 64 * v - 1) / (64 * v);
        if (it <= 2) return fn(t, v, Int<2>{});
        if (it <= 4) return fn(t, v, Int<4>{});
        if (it <= 5) return fn(t, v, Int<5>{});
        if (it <= 8) return fn(t, v, Int<8>{});
        if (it <= 16) return fn(t, v, Int<16>{});
        return 9002;
    });
}

// ===========================================================================
// RMSNorm / LayerNorm — wave-per-row, register-resident, no barriers.
// HBM-bound: one coalesced read of the row into VGPRs, wave-shuffle
// reductions, one coalesced write. (The first round's row-per-workgroup +
// LDS-stash version measured 0.75 TB/s on (32k, 2560) bf16; this structure
// removes the LDS round trip and both barriers.)
// Rows per workgroup = 4 (one per wave); lane owns elements lane*V + i*64*V.
// ===========================================================================

template <typename T, int V, int ITMAX, bool HAS_RES>
__global__ void __launch_bounds__(256) rmsnorm_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ res_in, const T* __restrict__ w,
    T* __restrict__ y, T* __restrict__ res_out, float* __restrict__ rstd_out,
    int64_t T_rows, int H, float eps) {
    int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T_rows) return;
    const int lane = threadIdx.x & 63;
    const T* xr = x + row * (int64_t)H;
    const T* rr = HAS_RES ? res_in + row * (int64_t)H : nullptr;

    float buf[ITMAX][V];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < ITMAX; ++i) {
        int c = (i * 64 + lane) * V;
        if (c < H) {
            VecIO<T, V>::load(xr + c, buf[i]);
            if (HAS_RES) {
                float rv[V];
                VecIO<T, V>::load(rr + c, rv);
#pragma unroll
                for (int kk = 0; kk < V; ++kk) {
                    // tensor-dtype residual add (layer.py:74,87): round the sum
                    float v = buf[i][kk] + rv[kk];
                    T tmp;
                    store_from_f32(&tmp, v);
                    buf[i][kk] = load_as_f32(&tmp);
                }
            }
#pragma unroll
            for (int kk = 0; kk < V; ++kk) ss += buf[i][kk] * buf[i][kk];
        }
    }
    float rstd = rsqrtf(wave_reduce_sum(ss) / (float)H + eps);
    if (lane == 0 && rstd_out) rstd_out[row] = rstd;

    T* yr = y + row * (int64_t)H;
    T* sr = HAS_RES ? res_out + row * (int64_t)H : nullptr;
#pragma unroll
    for (int i = 0; i < ITMAX; ++i) {
        int c = (i * 64 + lane) * V;
        if (c < H) {
            if (HAS_RES) VecIO<T, V>::store(sr + c, buf[i]);
            float wv[V], ov[V];
            VecIO<T, V>::load(w + c, wv);
#pragma unroll
            for (int kk = 0; kk < V; ++kk) {
                T tmp;
                store_from_f32(&tmp, buf[i][kk] * rstd);  // cast before weight (rmsnorm/base.py:23-25)
                ov[kk] = wv[kk] * load_as_f32(&tmp);
            }
            VecIO<T, V>::store(yr + c, ov);
        }
    }
}

extern "C" int dolomite_rmsnorm_fwd(dolomite_stream_t stream,
                                    const void* x, const void* res_in, const void* w,
                                    void* y, void* res_out, float* rstd,
                                    int64_t T_rows, int64_t H, float eps, int dtype) {
    if (T_rows == 0) return 0;
    dim3 grid((uint32_t)((T_rows + 3) / 4)), block(256);
    return select_norm(dtype, H, [&](auto t, auto v, auto it) {
        return select_bool(res_in != nullptr, [&](auto has_res) {
            using T = decltype(t);
            hipLaunchKernelGGL((rmsnorm_fwd_kernel<T, v, it, has_res>), grid, block, 0, (hipStream_t)stream,
                               (const T*)x, (const T*)res_in, (const T*)w, (T*)y, (T*)res_out, rstd,
                               T_rows, (int)H, eps);
            return dol_last_error();
        });
    });
}

// ---------------------------------------------------------------------------
// RMSNorm backward — wave-per-row, per-wave dw partials (fixed grid).
//   dx = rstd*(w*dy - s_hat * mean(w*dy*s_hat)),  s_hat = s_fp32*rstd
//   dw = sum_rows dy * cast_to_dtype(s_hat)          (fp32 partials)
// ---------------------------------------------------------------------------

#define RMS_BWD_BLOCKS 1024  // x4 waves = 4096 dw partial rows

extern "C" int dolomite_rmsnorm_bwd_nblocks(int64_t T_rows) {
    (void)T_rows;
    return RMS_BWD_BLOCKS * 4;
}

template <typename T, int V, int ITMAX, int MODE>  // MODE: bit0 = layernorm, bit1 = fused dres add
__global__ void __launch_bounds__(256) norm_bwd_kernel(
    const T* __restrict__ dy, const T* __restrict__ s, const T* __restrict__ w,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    T* __restrict__ dx, float* __restrict__ dw_partial,
    const T* __restrict__ dres,  // residual-stream grad: dx += dres (iff HAS_DRES)
    int64_t T_rows, int H) {
    constexpr bool IS_LN = (MODE & 1) != 0;
    constexpr bool HAS_DRES = (MODE & 2) != 0;
    const int lane = threadIdx.x & 63;
    const int64_t wslot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nslots = (int64_t)gridDim.x * 4;

    // Register budget is the occupancy lever here (HBM-bound kernel, one
    // wave per row): dw/db accumulate in PHASE 1 so neither the weight nor
    // the raw dy has to stay live across the cross-lane reduce — only
    // s_hat and dy*w survive to phase 2. ITMAX=5/V=8 drops ~40 VGPRs,
    // buying a third wave per SIMD to cover the phase-boundary stalls.
    float dw_acc[ITMAX][V], db_acc[IS_LN ? ITMAX : 1][IS_LN ? V : 1];
#pragma unroll
    for (int i = 0; i < ITMAX; ++i)
#pragma unroll
        for (int kk = 0; kk < V; ++kk) {
            dw_acc[i][kk] = 0.f;
            if (IS_LN) db_acc[i][kk] = 0.f;
        }

    for (int64_t row = wslot; row < T_rows; row += nslots) {
        const T* dyr = dy + row * (int64_t)H;
        const T* sr = s + row * (int64_t)H;
        float r = rstd[row];
        float mu = IS_LN ? mean[row] : 0.f;

        float sh[ITMAX][V], dyw[ITMAX][V];
        float d1 = 0.f, d2 = 0.f;
#pragma unroll
        for (int i = 0; i < ITMAX; ++i) {
            int c0 = (i * 64 + lane) * V;
            if (c0 < H) {
                float wv[V], dyv[V];
                VecIO<T, V>::load(w + c0, wv);  // L2-resident, re-read per row
                VecIO<T, V>::load_nt(sr + c0, sh[i]);
                VecIO<T, V>::load_nt(dyr + c0, dyv);
#pragma unroll
                for (int kk = 0; kk < V; ++kk) {
                    float shat = (sh[i][kk] - mu) * r;
                    float dw_ = dyv[kk] * wv[kk];
                    sh[i][kk] = shat;
                    dyw[i][kk] = dw_;
                    d2 += dw_ * shat;
                    if (IS_LN) {
                        d1 += dw_;
                        dw_acc[i][kk] += dyv[kk] * shat;
                        db_acc[i][kk] += dyv[kk];
                    } else {
                        // dw uses the CAST normalized value (reference casts
                        // before the weight multiply)
                        T tmp;
                        store_from_f32(&tmp, shat);
                        dw_acc[i][kk] += dyv[kk] * load_as_f32(&tmp);
                    }
                }
            } else {
#pragma unroll
                for (int kk = 0; kk < V; ++kk) { sh[i][kk] = 0.f; dyw[i][kk] = 0.f; }
            }
        }
        float m2 = wave_reduce_sum(d2) / (float)H;
        float m1 = IS_LN ? wave_reduce_sum(d1) / (float)H : 0.f;

        T* dxr = dx + row * (int64_t)H;
        const T* drr = HAS_DRES ? dres + row * (int64_t)H : nullptr;
#pragma unroll
        for (int i = 0; i < ITMAX; ++i) {
            int c0 = (i * 64 + lane) * V;
            if (c0 < H) {
                float dxv[V];
                float drv[V];
                if (HAS_DRES) VecIO<T, V>::load_nt(drr + c0, drv);
#pragma unroll
                for (int kk = 0; kk < V; ++kk)
                    dxv[kk] = IS_LN ? r * (dyw[i][kk] - m1 - sh[i][kk] * m2)
                                    : r * (dyw[i][kk] - sh[i][kk] * m2);
                if (HAS_DRES)
#pragma unroll
                    for (int kk = 0; kk < V; ++kk) dxv[kk] += drv[kk];
                VecIO<T, V>::store_nt(dxr + c0, dxv);
            }
        }
    }

    float* dwp = dw_partial + wslot * H;
    float* dbp = IS_LN ? dw_partial + (nslots + wslot) * H : nullptr;
#pragma unroll
    for (int i = 0; i < ITMAX; ++i) {
        int c0 = (i * 64 + lane) * V;
        if (c0 < H) {
#pragma unroll
            for (int kk = 0; kk < V; ++kk) {
                dwp[c0 + kk] = dw_acc[i][kk];
                if (IS_LN) dbp[c0 + kk] = db_acc[i][kk];
            }
        }
    }
}

// shared by dolomite_rmsnorm_bwd (mean = nullptr) and dolomite_layernorm_bwd
template <bool IS_LN>
static int launch_norm_bwd(dolomite_stream_t stream, const void* dy, const void* s, const void* w,
                           const float* mean, const float* rstd, void* dx, float* dw_partial,
                           const void* dres, int64_t T_rows, int64_t H, int dtype) {
    if (T_rows == 0) return 0;
    dim3 grid(RMS_BWD_BLOCKS), block(256);
    return select_norm(dtype, H, [&](auto t, auto v, auto it) {
        return select_bool(dres != nullptr, [&](auto has_dres) {
            using T = decltype(t);
            constexpr int MODE = (IS_LN ? 1 : 0) | (has_dres ? 2 : 0);
            hipLaunchKernelGGL((norm_bwd_kernel<T, v, it, MODE>), grid, block, 0, (hipStream_t)stream,
                               (const T*)dy, (const T*)s, (const T*)w, mean, rstd, (T*)dx, dw_partial,
                               (const T*)dres, T_rows, (int)H);
            return dol_last_error();
        });
    });
}

extern "C" int dolomite_rmsnorm_bwd(dolomite_stream_t stream,
                                    const void* dy, const void* s, const void* w,
                                    const float* rstd, void* dx, float* dw_partial,
                                    const void* dres, int64_t T_rows, int64_t H, int dtype) {
    return launch_norm_bwd<false>(stream, dy, s, w, nullptr, rstd, dx, dw_partial, dres, T_rows, H, dtype);
}

// ---------------------------------------------------------------------------
// LayerNorm forward (wave-per-row) and backward (shares norm_bwd_kernel).
//   y = cast((x32 - mu)*rstd*w32 + b32)    [torch F.layer_norm semantics]
// ---------------------------------------------------------------------------

template <typename T, int V, int ITMAX, bool HAS_RES>
__global__ void __launch_bounds__(256) layernorm_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ res_in,
    const T* __restrict__ w, const T* __restrict__ b,
    T* __restrict__ y, T* __restrict__ res_out,
    float* __restrict__ mean_out, float* __restrict__ rstd_out,
    int64_t T_rows, int H, float eps) {
    int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T_rows) return;
    const int lane = threadIdx.x & 63;
    const T* xr = x + row * (int64_t)H;
    const T* rr = HAS_RES ? res_in + row * (int64_t)H : nullptr;

    float buf[ITMAX][V];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < ITMAX; ++i) {
        int c = (i * 64 + lane) * V;
        if (c < H) {
            VecIO<T, V>::load(xr + c, buf[i]);
            if (HAS_RES) {
                float rv[V];
                VecIO<T, V>::load(rr + c, rv);
#pragma unroll
                for (int kk = 0; kk < V; ++kk) {
                    float v = buf[i][kk] + rv[kk];
                    T tmp;
                    store_from_f32(&tmp, v);
                    buf[i][kk] = load_as_f32(&tmp);
                }
            }
#pragma unroll
            for (int kk = 0; kk < V; ++kk) sum += buf[i][kk];
        }
    }
    float mu = wave_reduce_sum(sum) / (float)H;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < ITMAX; ++i) {
        int c = (i * 64 + lane) * V;
        if (c < H)
#pragma unroll
            for (int kk = 0; kk < V; ++kk) {
                float d = buf[i][kk] - mu;
                ss += d * d;
            }
    }
    float rstd = rsqrtf(wave_reduce_sum(ss) / (float)H + eps);
    if (lane == 0) {
        if (mean_out) mean_out[row] = mu;
        if (rstd_out) rstd_out[row] = rstd;
    }

    T* yr = y + row * (int64_t)H;
    T* sr = HAS_RES ? res_out + row * (int64_t)H : nullptr;
#pragma unroll
    for (int i = 0; i < ITMAX; ++i) {
        int c = (i * 64 + lane) * V;
        if (c < H) {
            if (HAS_RES) VecIO<T, V>::store(sr + c, buf[i]);
            float wv[V], bv[V], ov[V];
            VecIO<T, V>::load(w + c, wv);
            VecIO<T, V>::load(b + c, bv);
#pragma unroll
            for (int kk = 0; kk < V; ++kk) ov[kk] = (buf[i][kk] - mu) * rstd * wv[kk] + bv[kk];
            VecIO<T, V>::store(yr + c, ov);
        }
    }
}

extern "C" int dolomite_layernorm_fwd(dolomite_stream_t stream,
                                      const void* x, const void* res_in, const void* w, const void* b,
                                      void* y, void* res_out, float* mean, float* rstd,
                                      int64_t T_rows, int64_t H, float eps, int dtype) {
    if (T_rows == 0) return 0;
    dim3 grid((uint32_t)((T_rows + 3) / 4)), block(256);
    return select_norm(dtype, H, [&](auto t, auto v, auto it) {
        return select_bool(res_in != nullptr, [&](auto has_res) {
            using T = decltype(t);
            hipLaunchKernelGGL((layernorm_fwd_kernel<T, v, it, has_res>), grid, block, 0, (hipStream_t)stream,
                               (const T*)x, (const T*)res_in, (const T*)w, (const T*)b, (T*)y, (T*)res_out,
                               mean, rstd, T_rows, (int)H, eps);
            return dol_last_error();
        });
    });
}

extern "C" int dolomite_layernorm_bwd(dolomite_stream_t stream,
                                      const void* dy, const void* s, const void* w,
                                      const float* mean, const float* rstd,
                                      void* dx, float* dwdb_partial,
                                      const void* dres, int64_t T_rows, int64_t H, int dtype) {
    return launch_norm_bwd<true>(stream, dy, s, w, mean, rstd, dx, dwdb_partial, dres, T_rows, H, dtype);
}

// ===========================================================================
// Partials reduction: out[h] = sum_i partial[i*H + h], in a FIXED order (no
// atomics, so dw/db are bitwise reproducible run to run):
//   nsplit = min(32, ceil(nblocks / 128)),  chunk = ceil(nblocks / nsplit)
//   pass 1: thread (c, h) sums rows [c*chunk, min((c+1)*chunk, nblocks)) of
//           column h in ascending row order, starting from +0, and stores
//           the sum over partial[c*chunk*H + h] — the first element it read,
//           which no other thread touches;
//   pass 2: out[h] = the chunk sums added in ascending c, starting from +0.
// nsplit == 1 is pass 1 alone, storing straight into out (partial is then
// left intact). No chunk is empty: nblocks > 128*(nsplit-1) and, when the cap
// of 32 binds, nblocks > 31*31, so (nsplit-1)*chunk < nblocks either way.
// The C signature keeps `const float* partial` (ABI unchanged); the buffer
// is the caller's mutable scratch and the header says it is overwritten.
// Parallel over column blocks AND row chunks: the serial column-loop
// version filled only H/256 workgroups, 40 GB/s on (4096, 2560).
// ===========================================================================

#define REDUCE_MAX_SPLIT 32
#define REDUCE_ROWS_PER_SPLIT 128

__global__ void __launch_bounds__(256) reduce_partials_chunk_kernel(
    float* partial, float* out, int64_t nblocks, int64_t H, int64_t chunk) {
    int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    int64_t i0 = (int64_t)blockIdx.y * chunk;
    int64_t i1 = min(i0 + chunk, nblocks);
    const float* p = partial + h;
    float acc = 0.f;
    int64_t i = i0;
    // 8 independent loads in flight, then 8 adds in row order
    for (; i + 8 <= i1; i += 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = p[(i + k) * H];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += v[k];
    }
    for (; i < i1; ++i) acc += p[i * H];
    if (gridDim.y == 1)
        out[h] = acc;
    else if (i0 < i1)  // always true (no chunk is empty); keeps the store in bounds regardless
        partial[i0 * H + h] = acc;
}

__global__ void __launch_bounds__(256) reduce_partials_fold_kernel(
    const float* __restrict__ partial, float* __restrict__ out,
    int64_t H, int64_t chunk, int nsplit) {
    int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    float v[REDUCE_MAX_SPLIT];
#pragma unroll
    for (int c = 0; c < REDUCE_MAX_SPLIT; ++c)
        v[c] = c < nsplit ? partial[(int64_t)c * chunk * H + h] : 0.f;
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < REDUCE_MAX_SPLIT; ++c)
        if (c < nsplit) acc += v[c];
    out[h] = acc;
}

extern "C" int dolomite_reduce_partials(dolomite_stream_t stream,
                                        const float* partial, float* out,
                                        int64_t nblocks, int64_t H) {
    if (H <= 0) return 0;
    float* scratch = const_cast<float*>(partial);
    int64_t nsplit64 = (nblocks + REDUCE_ROWS_PER_SPLIT - 1) / REDUCE_ROWS_PER_SPLIT;
    int nsplit = (int)(nsplit64 > REDUCE_MAX_SPLIT ? REDUCE_MAX_SPLIT : nsplit64);
    if (nsplit < 1) nsplit = 1;
    int64_t chunk = (nblocks + nsplit - 1) / nsplit;
    dim3 grid((uint32_t)((H + 255) / 256), (uint32_t)nsplit), block(256);
    hipLaunchKernelGGL(reduce_partials_chunk_kernel, grid, block, 0, (hipStream_t)stream,
                       scratch, out, nblocks, H, chunk);
    if (nsplit > 1)
        hipLaunchKernelGGL(reduce_partials_fold_kernel, dim3(grid.x), block, 0, (hipStream_t)stream,
                           partial, out, H, chunk, nsplit);
    return dol_last_error();
}

// ===========================================================================
// RoPE on the packed QKV layout (in-place or same-offset out-of-place).
// One thread per (token, head, pair). position_embedding/rope.py:104-121.
// ===========================================================================

// vector variant: each thread rotates 8 consecutive pairs with two 16B
// loads/stores (requires (D/2) % 8 == 0 — true of every head dim here)
template <typename T>
__global__ void __launch_bounds__(256) rope_qkv_vec8_kernel(
    const T* __restrict__ qkv_in, T* __restrict__ qkv_out,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    int64_t total8, int64_t row_len, int H, int Hkv, int D, int G,
    int64_t q_gstride, int64_t k_off, int64_t kv_hstride, float dir) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total8) return;
    int halfD8 = (D >> 1) >> 3;
    int nheads = H + Hkv;
    int64_t per_tok = (int64_t)nheads * halfD8;
    int64_t t = idx / per_tok;
    int rem = (int)(idx % per_tok);
    int hh = rem / halfD8;
    int i0 = (rem % halfD8) * 8;

    int64_t base = t * row_len;
    if (hh < H)
        base += (int64_t)(hh / G) * q_gstride + (int64_t)(hh % G) * D;
    else
        base += k_off + (int64_t)(hh - H) * kv_hstride;

    float x1[8], x2[8], c1[8], s1[8], c2[8], s2[8], y1[8], y2[8];
    VecIO<T, 8>::load(qkv_in + base + i0, x1);
    VecIO<T, 8>::load(qkv_in + base + i0 + (D >> 1), x2);
    VecIO<float, 4>::load(cos_t + t * D + i0, c1);
    VecIO<float, 4>::load(cos_t + t * D + i0 + 4, c1 + 4);
    VecIO<float, 4>::load(sin_t + t * D + i0, s1);
    VecIO<float, 4>::load(sin_t + t * D + i0 + 4, s1 + 4);
    VecIO<float, 4>::load(cos_t + t * D + i0 + (D >> 1), c2);
    VecIO<float, 4>::load(cos_t + t * D + i0 + (D >> 1) + 4, c2 + 4);
    VecIO<float, 4>::load(sin_t + t * D + i0 + (D >> 1), s2);
    VecIO<float, 4>::load(sin_t + t * D + i0 + (D >> 1) + 4, s2 + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        y1[e] = x1[e] * c1[e] - x2[e] * (s1[e] * dir);
        y2[e] = x2[e] * c2[e] + x1[e] * (s2[e] * dir);
    }
    VecIO<T, 8>::store(qkv_out + base + i0, y1);
    VecIO<T, 8>::store(qkv_out + base + i0 + (D >> 1), y2);
}

template <typename T>
__global__ void __launch_bounds__(256) rope_qkv_kernel(
    const T* __restrict__ qkv_in, T* __restrict__ qkv_out,
    const float* __restrict__ cos_t, const float* __restrict__ sin_t,
    int64_t total, int64_t row_len, int H, int Hkv, int D, int G,
    int64_t q_gstride, int64_t k_off, int64_t kv_hstride, float dir) {
    int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    int halfD = D >> 1;
    int nheads = H + Hkv;
    int64_t pairs_per_tok = (int64_t)nheads * halfD;
    int64_t t = idx / pairs_per_tok;
    int rem = (int)(idx % pairs_per_tok);
    int hh = rem / halfD;
    int i = rem % halfD;

    int64_t base = t * row_len;
    if (hh < H) {
        base += (int64_t)(hh / G) * q_gstride + (int64_t)(hh % G) * D;
    } else {
        int j = hh - H;
        base += k_off + (int64_t)j * kv_hstride;
    }
    float c1 = cos_t[t * D + i];
    float s1 = sin_t[t * D + i] * dir;
    float c2 = cos_t[t * D + i + halfD];
    float s2 = sin_t[t * D + i + halfD] * dir;
    float x1 = load_as_f32(qkv_in + base + i);
    float x2 = load_as_f32(qkv_in + base + i + halfD);
    store_from_f32(qkv_out + base + i, x1 * c1 - x2 * s1);
    store_from_f32(qkv_out + base + i + halfD, x2 * c2 + x1 * s2);
}

extern "C" int dolomite_rope_qkv(dolomite_stream_t stream,
                                 const void* qkv_in, void* qkv_out,
                                 const float* cos_t, const float* sin_t,
                                 int64_t T_rows, int64_t row_len,
                                 int H, int Hkv, int D, int G,
                                 int64_t q_gstride, int64_t k_off, int64_t kv_hstride,
                                 int dir, int rotate_v_copy, int dtype) {
    (void)rotate_v_copy;
    if (D % 2 != 0) return 9003;
    float fdir = (dir >= 0) ? 1.f : -1.f;
    bool vec8 = (D / 2) % 8 == 0;
    // threads: one per 8 pairs (vec8) or one per pair
    int64_t total = T_rows * (int64_t)(H + Hkv) * (vec8 ? D / 2 / 8 : D / 2);
    if (total == 0) return 0;
    dim3 grid((uint32_t)((total + 255) / 256)), block(256);
    return select_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        if (vec8)
            hipLaunchKernelGGL((rope_qkv_vec8_kernel<T>), grid, block, 0, (hipStream_t)stream,
                               (const T*)qkv_in, (T*)qkv_out, cos_t, sin_t,
                               total, row_len, H, Hkv, D, G, q_gstride, k_off, kv_hstride, fdir);
        else
            hipLaunchKernelGGL((rope_qkv_kernel<T>), grid, block, 0, (hipStream_t)stream,
                               (const T*)qkv_in, (T*)qkv_out, cos_t, sin_t,
                               total, row_len, H, Hkv, D, G, q_gstride, k_off, kv_hstride, fdir);
        return dol_last_error();
    });
}

// ===========================================================================
// Fused cross entropy (mean, ignore_index): one workgroup per row.
// fwd: online max/sum -> lse, row_loss.  bwd: dlogits = (p - onehot)*gs.
// ===========================================================================

template <typename T, int V>
__global__ void __launch_bounds__(256) ce_fwd_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ labels,
    float* __restrict__ row_loss, float* __restrict__ lse_out,
    int64_t V_dim, int64_t row_stride, int ignore_index) {
    __shared__ float red[8];
    int64_t t = blockIdx.x;
    const T* xr = logits + t * row_stride;

    float m = -INFINITY, ssum = 0.f;
    for (int64_t c = threadIdx.x * V; c < V_dim; c += (int64_t)blockDim.x * V) {
        float xv[V];
        if (c + V <= V_dim) {
            VecIO<T, V>::load(xr + c, xv);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k) xv[k] = (c + k < V_dim) ? load_as_f32(xr + c + k) : -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float v = xv[k];
            if (v > m) {
                ssum *= __expf(m - v);
                m = v;
            }
            ssum += __expf(v - m);
        }
    }
    // block combine: global max then shift partial sums
    float mall = m;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mall = fmaxf(mall, __shfl_xor(mall, off, 64));
    int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) red[wid] = mall;
    __syncthreads();
    float gmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float shifted = (m == -INFINITY) ? 0.f : ssum * __expf(m - gmax);
    float total = block_reduce_sum(shifted, red, blockDim.x);
    float lse = gmax + __logf(total);

    if (threadIdx.x == 0) {
        lse_out[t] = lse;
        int64_t lab = labels[t];
        if (lab == ignore_index) {
            row_loss[t] = 0.f;
        } else {
            row_loss[t] = lse - load_as_f32(xr + lab);
        }
    }
}

extern "C" int dolomite_ce_fwd(dolomite_stream_t stream,
                               const void* logits, const int64_t* labels,
                               float* row_loss, float* lse,
                               int64_t T_rows, int64_t V_dim, int64_t row_stride,
                               int ignore_index, int dtype) {
    dim3 grid((uint32_t)T_rows), block(256);
    return select_dtype_vec(dtype, V_dim, [&](auto t, auto v) {
        using T = decltype(t);
        hipLaunchKernelGGL((ce_fwd_kernel<T, v>), grid, block, 0, (hipStream_t)stream,
                           (const T*)logits, labels, row_loss, lse, V_dim, row_stride, ignore_index);
        return dol_last_error();
    });
}

template <typename T, int V>
__global__ void __launch_bounds__(256) ce_bwd_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ labels,
    const float* __restrict__ lse, T* __restrict__ dlogits,
    const float* __restrict__ gs_dev,
    int64_t V_dim, int64_t row_stride, int ignore_index) {
    // device-side grad scale: removes the round-1 host sync that read
    // gout/n_valid back to the CPU before every CE backward launch
    const float gs = *gs_dev;
    int64_t t = blockIdx.x;
    const T* xr = logits + t * row_stride;
    T* dr = dlogits + t * row_stride;
    int64_t lab = labels[t];
    float l = lse[t];
    if (lab == ignore_index) {
        float zv[V] = {};
        for (int64_t c = threadIdx.x * V; c < V_dim; c += (int64_t)blockDim.x * V) {
            if (c + V <= V_dim)
                VecIO<T, V>::store(dr + c, zv);
            else
#pragma unroll
                for (int k = 0; k < V; ++k)
                    if (c + k < V_dim) store_from_f32(dr + c + k, 0.f);
        }
        return;
    }
    for (int64_t c = threadIdx.x * V; c < V_dim; c += (int64_t)blockDim.x * V) {
        if (c + V <= V_dim) {
            float xv[V], gv[V];
            VecIO<T, V>::load(xr + c, xv);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                float p = __expf(xv[k] - l);
                gv[k] = ((c + k == lab) ? (p - 1.f) : p) * gs;
            }
            VecIO<T, V>::store(dr + c, gv);
        } else {
#pragma unroll
            for (int k = 0; k < V; ++k)
                if (c + k < V_dim) {
                    float p = __expf(load_as_f32(xr + c + k) - l);
                    float g = (c + k == lab) ? (p - 1.f) : p;
                    store_from_f32(dr + c + k, g * gs);
                }
        }
    }
}

extern "C" int dolomite_ce_bwd(dolomite_stream_t stream,
                               const void* logits, const int64_t* labels, const float* lse,
                               void* dlogits, const float* grad_scale_dev,
                               int64_t T_rows, int64_t V_dim, int64_t row_stride,
                               int ignore_index, int dtype) {
    dim3 grid((uint32_t)T_rows), block(256);
    return select_dtype_vec(dtype, V_dim, [&](auto t, auto v) {
        using T = decltype(t);
        hipLaunchKernelGGL((ce_bwd_kernel<T, v>), grid, block, 0, (hipStream_t)stream,
                           (const T*)logits, labels, lse, (T*)dlogits, grad_scale_dev,
                           V_dim, row_stride, ignore_index);
        return dol_last_error();
    });
}

// ===========================================================================
// Fused AdamW on a flat fp32 master shard (torch.optim.AdamW semantics),
// with optional bf16 write-out. HBM-bound; 4 elems per thread, coalesced.
// ===========================================================================

typedef unsigned short us4_t __attribute__((ext_vector_type(4)));

template <int GRAD_BF16>
__global__ void __launch_bounds__(256) adamw_kernel(
    float* __restrict__ master, uint16_t* __restrict__ param_out,
    const void* __restrict__ grad_v, float* __restrict__ m, float* __restrict__ v,
    int64_t n, float lr, float b1, float b2, float eps, float wd,
    float bc1, float bc2, const float* __restrict__ gscale) {
    int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i0 >= n) return;
    // fused grad-clip scale: one device scalar read replaces a whole
    // read+write pass over the shard grads (reference clips then steps;
    // scaling at the point of use is the same arithmetic in fp32)
    const float gs = gscale ? *gscale : 1.f;
    if (i0 + 4 <= n) {  // vector fast path (16B loads/stores per stream)
        f4_t p4 = *(f4_t*)&master[i0];
        f4_t m4 = *(f4_t*)&m[i0];
        f4_t v4 = *(f4_t*)&v[i0];
        f4_t g4;
        if (GRAD_BF16) {
            us4_t gb = *(const us4_t*)&((const uint16_t*)grad_v)[i0];
#pragma unroll
            for (int k = 0; k < 4; ++k) g4[k] = bf16_to_f32((uint16_t)gb[k]);
        } else {
            g4 = *(const f4_t*)&((const float*)grad_v)[i0];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) g4[k] *= gs;
        us4_t o4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float p = p4[k] * (1.f - lr * wd);
            float mi = m4[k] * b1 + (1.f - b1) * g4[k];
            float vi = v4[k] * b2 + (1.f - b2) * g4[k] * g4[k];
            m4[k] = mi;
            v4[k] = vi;
            p -= (lr / bc1) * mi / (sqrtf(vi / bc2) + eps);
            p4[k] = p;
            o4[k] = f32_to_bf16(p);
        }
        *(f4_t*)&master[i0] = p4;
        *(f4_t*)&m[i0] = m4;
        *(f4_t*)&v[i0] = v4;
        if (param_out) *(us4_t*)&param_out[i0] = o4;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int64_t i = i0 + k;
        if (i >= n) return;
        float g = GRAD_BF16 ? bf16_to_f32(((const uint16_t*)grad_v)[i]) : ((const float*)grad_v)[i];
        g *= gs;
        float p = master[i];
        p *= (1.f - lr * wd);
        float mi = m[i] * b1 + (1.f - b1) * g;
        float vi = v[i] * b2 + (1.f - b2) * g * g;
        m[i] = mi;
        v[i] = vi;
        float denom = sqrtf(vi / bc2) + eps;
        p -= (lr / bc1) * mi / denom;
        master[i] = p;
        if (param_out) param_out[i] = f32_to_bf16(p);
    }
}

extern "C" int dolomite_adamw_step(dolomite_stream_t stream,
                                   float* master, void* param_out_bf16,
                                   const void* grad, int grad_dtype,
                                   float* m, float* v,
                                   int64_t n, float lr, float beta1, float beta2,
                                   float eps, float weight_decay, int step,
                                   const float* gscale) {
    if (n == 0) return 0;
    float bc1 = 1.f - powf(beta1, (float)step);
    float bc2 = 1.f - powf(beta2, (float)step);
    int64_t nthreads = (n + 3) / 4;
    dim3 grid((uint32_t)((nthreads + 255) / 256)), block(256);
    return select_bool(grad_dtype == DOLOMITE_BF16, [&](auto grad_bf16) {
        hipLaunchKernelGGL((adamw_kernel<grad_bf16>), grid, block, 0, (hipStream_t)stream,
                           master, (uint16_t*)param_out_bf16, grad, m, v, n, lr, beta1, beta2, eps,
                           weight_decay, bc1, bc2, gscale);
        return dol_last_error();
    });
}

// ===========================================================================
// Deterministic squared-sum (grad-norm input): fixed-order per-thread
// strided accumulation + a fixed LDS tree per block -> one fp32 partial per
// block, folded by one more fixed tree (sqsum_fold_kernel). Reading the
// bf16 flat grads directly halves the bytes of the fp32-cast-then-
// pow(2).sum() path, and the fixed reduction order keeps grad-norm (and so
// the clipped step) bit-deterministic for checkpoint-resume.
// ===========================================================================

#define SQSUM_BLOCKS 1024

// 8 elements per thread for BOTH dtypes: the thread->element mapping and
// per-thread accumulation order are then identical whether the grads are
// the bf16 flat bucket (world-1 plain path) or the fp32 reduce-scatter
// shard (collective path), so the two paths' grad norms agree BITWISE
// (the world-1 RCCL-equivalence test asserts exactly that).
template <typename T>
__global__ void __launch_bounds__(256) sqsum_kernel(
    const T* __restrict__ x, int64_t n, float* __restrict__ partials) {
    __shared__ float red[256];
    const int64_t stride = (int64_t)gridDim.x * 256 * 8;
    float acc = 0.f;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += stride) {
        float b[8];
        if (i + 8 <= n) {
            if constexpr (sizeof(T) == 2) {
                VecIO<uint16_t, 8>::load_nt((const uint16_t*)x + i, b);
            } else {
                VecIO<float, 4>::load_nt((const float*)x + i, b);
                VecIO<float, 4>::load_nt((const float*)x + i + 4, b + 4);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) b[k] = (i + k < n) ? load_as_f32(x + i + k) : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += b[k] * b[k];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int s_ = 128; s_ > 0; s_ >>= 1) {
        if ((int)threadIdx.x < s_) red[threadIdx.x] += red[threadIdx.x + s_];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(256) sqsum_fold_kernel(const float* __restrict__ partials,
                                                         float* __restrict__ out) {
    __shared__ float red[256];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < SQSUM_BLOCKS / 256; ++k) acc += partials[k * 256 + threadIdx.x];
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int s_ = 128; s_ > 0; s_ >>= 1) {
        if ((int)threadIdx.x < s_) red[threadIdx.x] += red[threadIdx.x + s_];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

extern "C" int dolomite_sqsum(dolomite_stream_t stream, const void* x, int64_t n,
                              float* partials, float* out, int dtype) {
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        (void)hipMemsetAsync(out, 0, sizeof(float), s);
        return dol_last_error();
    }
    int err = select_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((sqsum_kernel<T>), dim3(SQSUM_BLOCKS), dim3(256), 0, s, (const T*)x, n, partials);
        return dol_last_error();
    });
    if (err) return err;
    // one block, fixed tree (1024 scalars: not worth reduce_partials' two passes)
    hipLaunchKernelGGL((sqsum_fold_kernel), dim3(1), dim3(256), 0, s, partials, out);
    return dol_last_error();
}

// ===========================================================================
// Scalar scale in place (grad clip apply).
// ===========================================================================

template <typename T>
__global__ void __launch_bounds__(256) scale_kernel(T* __restrict__ buf, int64_t n, float s) {
    int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int64_t i = i0 + k;
        if (i < n) store_from_f32(buf + i, load_as_f32(buf + i) * s);
    }
}

extern "C" int dolomite_scale_inplace(dolomite_stream_t stream, void* buf, int64_t n,
                                      float scale, int dtype) {
    if (n == 0) return 0;
    int64_t nthreads = (n + 3) / 4;
    dim3 grid((uint32_t)((nthreads + 255) / 256)), block(256);
    return select_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((scale_kernel<T>), grid, block, 0, (hipStream_t)stream, (T*)buf, n, scale);
        return dol_last_error();
    });
}

extern "C" int dolomite_hip_abi_version(void) { return 2; }
