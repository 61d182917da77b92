// dolomite_hip — MFMA / tr16 tile helpers shared by the attention kernels
// (attention.hip fwd / dkv / dq, decode.hip) and, for the vector types,
// moe_gemm.hip. One copy each of the fragment types, the pipelined
// ds_read_b64_tr_b16 ladder, the guarded 16-byte load, the 4-lane row
// reductions, the transposed bf16 epilogue store and the K/V image geometry.
// Fragment layouts and the tr16 read semantics: see attention.hip.
#pragma once

#include <type_traits>

#include "common.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)

// ---------------------------------------------------------------------------
// Pipelined tr16 ladder (guide §5.7 forms (i)/(ii) + T3/T4 counted waits).
//
// Round 1 measured that per-fragment `lgkmcnt(0)` drains serialize the MFMA
// stream (each tr16 read's 50-cycle latency lands on the critical path).
// The ladder splits issue and wait: fragment i+1's reads are issued BEFORE
// waiting on fragment i with a counted `lgkmcnt(N)` (N = the just-issued
// reads), so LDS latency hides under the current fragment's MFMAs and the
// counter never drains to 0 inside the loop.
//
// Count discipline: the ladder's waits are exact only if no OTHER lgkm op
// is outstanding, so each region (a) opens with nothing in flight — every
// earlier LDS read has already been consumed by a score MFMA or the
// softmax — and (b) is fenced with sched_barrier(0)
// so the compiler cannot move its own ds/smem ops inside.
// ---------------------------------------------------------------------------

// Issue one B-fragment's two transpose reads (no wait): OFF = byte offset of
// the (rowbase, d0) chunk inside the image, a0/a1 = the lane's two row base
// addresses (computed once per kernel).
template <int OFF>
__device__ __forceinline__ void tr16_issue(unsigned a0, unsigned a1, bf16x4& lo, bf16x4& hi) {
    asm volatile(
        "ds_read_b64_tr_b16 %0, %2 offset:%c4\n\t"
        "ds_read_b64_tr_b16 %1, %3 offset:%c4"
        : "=&v"(lo), "=&v"(hi)
        : "v"(a0), "v"(a1), "i"(OFF)
        : "memory");
}

// Counted wait naming the registers it guarantees (guide §5.7 form (ii)).
template <int N>
__device__ __forceinline__ void lgkm_wait2(bf16x4& a, bf16x4& b) {
    asm volatile("s_waitcnt lgkmcnt(%c2)" : "+v"(a), "+v"(b) : "i"(N));
}

__device__ __forceinline__ bf16x8 tr16_join8(bf16x4 lo, bf16x4 hi) {
    bf16x8 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) { out[t] = lo[t]; out[4 + t] = hi[t]; }
    return out;
}

template <int DEPTH, int N, int I, typename Off, typename Mma>
__device__ __forceinline__ void tr16_ladder_step(unsigned a0, unsigned a1, bf16x4 (&lo)[DEPTH],
                                                 bf16x4 (&hi)[DEPTH], Off off, Mma& mma) {
    if constexpr (I < 0) {          // prologue: fragments 0 .. DEPTH-2
        constexpr int o = off(I + DEPTH - 1);
        tr16_issue<o>(a0, a1, lo[I + DEPTH - 1], hi[I + DEPTH - 1]);
        tr16_ladder_step<DEPTH, N, I + 1>(a0, a1, lo, hi, off, mma);
    } else if constexpr (I < N) {
        if constexpr (I + DEPTH - 1 < N) {
            constexpr int o = off(I + DEPTH - 1);
            tr16_issue<o>(a0, a1, lo[(I + DEPTH - 1) % DEPTH], hi[(I + DEPTH - 1) % DEPTH]);
        }
        constexpr int ahead = DEPTH - 1 < N - 1 - I ? DEPTH - 1 : N - 1 - I;  // fragments still in flight
        lgkm_wait2<2 * ahead>(lo[I % DEPTH], hi[I % DEPTH]);
        mma(std::integral_constant<int, I>{}, tr16_join8(lo[I % DEPTH], hi[I % DEPTH]));
        tr16_ladder_step<DEPTH, N, I + 1>(a0, a1, lo, hi, off, mma);
    }
}

// The ladder over N fragments, DEPTH-1 of them in flight at each wait:
// fragments 0 .. DEPTH-2 are issued up front; step i issues fragment
// i+DEPTH-1 (if any), waits until fragment i has landed — two reads per
// fragment still in flight stay outstanding — and hands it to
// mma(integral_constant<i>, frag). off(i) is fragment i's byte displacement
// (the ds_read immediate): a captureless lambda, evaluated at compile time.
template <int DEPTH, int N, typename Off, typename Mma>
__device__ __forceinline__ void tr16_ladder(unsigned a0, unsigned a1, Off off, Mma mma) {
    static_assert(DEPTH >= 1 && N >= DEPTH - 1, "prologue fragments must exist");
    __builtin_amdgcn_sched_barrier(0);
    bf16x4 lo[DEPTH], hi[DEPTH];
    tr16_ladder_step<DEPTH, N, 1 - DEPTH>(a0, a1, lo, hi, off, mma);
    __builtin_amdgcn_sched_barrier(0);
}

// Branchless guarded 16B load. Requires D % 8 == 0 (every head dim on this
// path): a chunk is then fully inside [0, D) or fully in the pad, so the
// guard reduces to ONE wave-divergent-free vector load from a clamped
// address plus per-element selects. (The original branchy version emitted
// 8 scalar loads + a vector load per fragment and forced hipcc to drain
// vmcnt(0) before every dependent MFMA — the dominant stall of round 1's
// backward kernel.)
__device__ __forceinline__ bf16x8 load_bf16x8_guard(const __bf16* p, int d0, int D, bool valid) {
    const __bf16* q = (d0 < D) ? p : (p - d0);  // clamp into the row
    bool ok = valid && (d0 < D);
    bf16x8 r = *(const bf16x8*)q;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = ok ? r[e] : (__bf16)0.f;
    return r;
}

// Store a transposed accumulator (head dim 16*dc + 4*lg + x on the
// registers, the row on l & 15) as bf16: 4 contiguous head-dim elements per
// lane and block, one 8-byte store. D % 8 == 0 on this path: a 4-wide group
// is all inside D or all pad.
template <int DCH>
__device__ __forceinline__ void fa_store_rowT_bf16(__bf16* row, const f32x4 (&acc)[DCH], float scale,
                                                   bool ok, int D, int lg) {
#pragma unroll
    for (int dc = 0; dc < DCH; ++dc) {
        const int d0 = dc * 16 + lg * 4;
        bf16x4 ov;
#pragma unroll
        for (int x = 0; x < 4; ++x) ov[x] = (__bf16)(acc[dc][x] * scale);
        if (ok && d0 < D) *(bf16x4*)&row[d0] = ov;
    }
}

// Reductions over the 4 lanes {l, l^16, l^32, l^48} that share one q row:
// v_permlane16_swap exchanges the odd 16-lane rows of its first operand with
// the even rows of its second, v_permlane32_swap the upper half-wave of the
// first with the lower half of the second. With both operands the same
// value each returned pair holds (own, partner) on every lane. Pure VALU.
__device__ __forceinline__ float qgroup_reduce_max(float v) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float qgroup_reduce_sum(float v) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// lane base addresses (reads h = 0, 1) of the permuted-key tr16 ladder over
// a natural-row image of stride S (attention.hip "Swapped-operand score
// tiles")
__device__ __forceinline__ void fa_tr16_perm_bases(const __bf16* img, int S, int lane,
                                                   unsigned& a0, unsigned& a1) {
    const int row = (lane >> 4) * 4 + ((lane >> 2) & 3);
    const int cc = (lane & 3) * 4;
    a0 = (unsigned)(size_t)(img + row * S + cc);
    a1 = (unsigned)(size_t)(img + (16 + row) * S + cc);
}

// ---------------------------------------------------------------------------
// 64-row LDS images of the 512-thread attention kernels: row-major
// [64][DPAD] bf16 at stride S = DPAD+16, rows in natural order. Stride chosen
// with tools_lds_sim.py (exact gfx950 bank model): the b128 row reads, the
// b128 staging writes and the key-permuted tr16 reads (8 consecutive rows per
// 32-lane pass) are all conflict-free.
// ---------------------------------------------------------------------------

// K/V image geometry shared by the fwd and dq kernels and their launchers:
// two 64-row images of stride S and, with dropout, the staged tile's 64
// keep-mask column words behind them — nothing else in dynamic LDS.
template <int DPAD>
struct FaKvLds {
    static constexpr int S = DPAD + 16;
    static constexpr size_t image_bytes = (size_t)2 * 64 * S * sizeof(__bf16);  // multiple of 256
    static constexpr size_t bytes(bool dropout) {
        return image_bytes + (dropout ? 64 * sizeof(uint32_t) : 0);
    }
};
