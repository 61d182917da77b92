// dolomite_hip — fp8 (OCP e4m3) weight-only linear for gfx950 (MI355X), many
// rows: the tiled W8A16 GEMM behind ops.fp8_linear above the skinny kernel's
// 64 rows (batched decode, chunked prefill, draft verification, short prompts).
//
//   y[M, N] = x[M, K] @ (Wq[N, K] * wscale[N, None])^T (+ bias[N]),  M >= 1
//
// x, bias, y bf16; Wq e4m3 bytes, dense (N, K); wscale fp32, one per output
// channel. The arithmetic is fp8_linear.hip's: e4m3 -> bf16 exactly in
// registers, bf16 MFMA, fp32 accumulate, the scale applied once to the
// accumulator, then the bias, then one rounding to bf16. The weight is read
// from HBM as fp8 only; no bf16 image of it is ever written to global memory.
//
// Work split: grid (ceil(N / 128), ceil(M / 128), nsplit), 256 threads. A
// workgroup owns a 128-row x 128-channel tile of y, its four waves a 2 x 2
// arrangement of 64 x 64 quadrants (wave & 1: channel half, wave >> 1: row
// half), a wave 4 x 4 accumulators of v_mfma_f32_16x16x32_bf16. Split c of the
// contraction owns k in [c*kper, min((c+1)*kper, K)), kper a multiple of the
// 128-wide k tile. Where the skinny kernel gives every wave one 16-channel
// slab and re-reads an x fragment from LDS for each MFMA, here an MFMA step
// reads 4 W fragments and 4 x fragments for 16 MFMAs: every converted W
// fragment feeds 4 row blocks, every x fragment 4 channel blocks.
//
// Operands: A = W (row = channel n0 + 16*cb + (lane & 15)), B = x (row =
// m0 + 16*rb + (lane & 15)), so accumulator (cb, rb) holds, on lane l and
// register r, channel n0 + 16*cb + 4*(l >> 4) + r of row m0 + 16*rb + (l & 15):
// four consecutive channels of one row per lane, one 8-byte bf16 store (or one
// 16-byte fp32 store into the split partials).
//
// Weight path: the tile's 128 rows x 128 bytes are 1024 16-byte pieces, four
// per thread; piece p = tid + 256*i is bytes 16*(p & 7) .. +16 of tile row
// p >> 3, so 8 consecutive lanes read the 128 contiguous bytes of one row's
// tile segment and a wave instruction 8 whole segments (the coalesced form that
// fp8_linear.hip measured at 2.65 TB/s against 2.0 for the per-row-scattered
// one). The pieces are stored to LDS as bytes ([128 rows][128 + 16], half the
// footprint of a bf16 tile) and converted at the fragment read: lane (row
// lane & 15, group g = lane >> 4) reads, per 64-wide chunk c, the 16 bytes at
// 64c + 16g with one b128 read, and each 8-byte half h gives, through
// e4m3x8_to_bf16x8, the A fragment of one MFMA step. A conversion serves 4
// MFMAs.
//
// k permutation (fp8_linear.hip's): MFMA step h of chunk c contracts, on lane
// group g and element e, the weight at k = 64c + 16g + 8h + e where the natural
// fragment holds 64c + 32h + 8g + e. The x image is written in that order (the
// 8-element piece at offset 16g + 8h of a chunk lands at 32h + 8g), so the B
// fragments are plain "row lane & 15, 8 contiguous at 32h + 8g" b128 reads and
// every product pairs x_k with w_k.
//
// Activations: the tile's 128 x 128 slice of x is 2048 16-byte pieces, eight
// per thread (piece p: row p >> 4, elements 8*(p & 15) .. +8), stored to a
// row-major image of stride 128 + 16 elements shared by the four waves.
//
// Pipelining: the W and x pieces of k tile t + 1 are loaded into registers
// (12 x 16 bytes per thread) before the MFMAs of tile t and stored to the one
// LDS buffer after them, between two barriers; no MFMA waits on a global load
// of its own tile. LDS: 18,432 B (W bytes) + 36,864 B (x) = 55,296 B, two
// workgroups per CU (registers allow two as well).
//
// Edges: rows at and beyond M and k at and beyond the split's end are staged
// as zeros (weight bytes of such k too; K % 16 == 0 and kper a multiple of 128
// make every 16-byte piece all inside or all outside), their loads redirected
// to an address inside the operands.
// Channels at and beyond N load weight row N - 1, which touches only their own
// accumulators, and are never stored; rows at and beyond M are never stored. x
// may be a row-strided view (unit last stride, row stride a multiple of 8,
// 16-byte aligned base).
//
// Filling the machine at small M: split-K, not a smaller tile (a 64 x 64 tile
// halves the reuse of every fragment for every M; the split leaves the inner
// loop alone). With nsplit > 1 each workgroup stores its fp32 partials
// exclusively into scratch[c][m][n] and a second launch sums them in ascending
// c, applies scale and bias and rounds: no atomics, bitwise reproducible for
// fixed arguments. dolomite_fp8_gemm_num_splits takes, among the counts of 1
// to min(ktiles / 2, 64) that leave no split empty, the one with the least
// estimated time (the smaller on a tie):
//   t(ns) = (kt + 1) * (r == 1 ? 1.9 : 1.33 r) + (ns > 1 ? 4 + ns (0.5 + p) : 0) us
// with kt = ceil(ktiles / ns) k tiles per split, r = ceil(tiles * ns / 256)
// workgroups on the busiest CU and p = 8 M N bytes at 4 TB/s. A lone workgroup
// on a CU (one wave per SIMD) takes 1.9 us per k tile, two or more that share
// it 1.33 us each (272 us at M = 4096 of mlp.c_fc: 10 per CU, 20 k tiles); a
// workgroup pays about one k tile to fill its pipeline, a join a launch and,
// per split, its partials written and read back. The first rule, min(ceil(256
// / tiles), ktiles / 2, K / (4 M)), was measured with half and twice its
// counts (first table of profiles/fp8_gemm_ab.txt); this estimate is a fit to
// those timings; with it the default is the fastest of every swept triple of
// the second table.
//
// Built as an object of its own with the flags of the other fp8 sources, whose
// conversion helper it shares.

#include "mfma_tiles.h"

#define F8G_BM 128                   // rows per workgroup tile
#define F8G_BN 128                   // channels per workgroup tile
#define F8G_BK 128                   // k per staged tile: 2 chunks of 64
#define F8G_WS (F8G_BK + 16)         // LDS row stride of the W image, bytes
#define F8G_XS (F8G_BK + 16)         // LDS row stride of the x image, elements
#define F8G_MAX_MTILES 65535

// The loads are branchless: a piece outside the operands (k at or beyond the
// split's end, a row at or beyond M) is loaded from a valid address instead
// (k = 0 of the row, or x itself) and replaced by zeros when it is staged, one
// tile later. A guarded load costs a branch per piece here, and the waits the
// compiler puts at their joins serialise the loads.

// The tile's four weight pieces of one thread: piece p = tid + 256*i is bytes
// k0 + 16*(p & 7) .. +16 of tile row p >> 3 (row pointers in wrow, clamped to
// N - 1).
__device__ __forceinline__ void f8g_load_w(const uint8_t* const (&wrow)[4], int k0, int k_end, u32x4 (&w)[4]) {
    const int k = k0 + (threadIdx.x & 7) * 16;
    const int kc = k < k_end ? k : 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = __builtin_nontemporal_load((const u32x4*)(wrow[i] + kc));
}

// The tile's eight x pieces of one thread: piece p = tid + 256*i is tile row
// p >> 4, elements k0 + 8*(p & 15) .. +8. xrow: x + row0*xs for the thread's
// first row row0 = m0 + (tid >> 4), formed but not read where row0 >= M.
__device__ __forceinline__ void f8g_load_x(const __bf16* x, const __bf16* xrow, int64_t xs, int row0, int M,
                                           int k0, int k_end, u32x4 (&xr)[8]) {
    const int k = k0 + (threadIdx.x & 15) * 8;
    const int kc = k < k_end ? k : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const __bf16* p = row0 + 16 * i < M ? xrow + 16 * i * xs : x;
        xr[i] = *(const u32x4*)(p + kc);
    }
}

__global__ void __launch_bounds__(256) fp8_gemm_kernel(
    const __bf16* __restrict__ x, const uint8_t* __restrict__ wq, const float* __restrict__ wscale,
    const __bf16* __restrict__ bias, __bf16* __restrict__ y, float* __restrict__ part,
    int M, int N, int K, int64_t xs, int kper, int nsplit) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lr = lane & 15;
    const int lg = lane >> 4;
    const int wn = wave & 1;   // channel half of the tile
    const int wm = wave >> 1;  // row half of the tile

    const int n0 = blockIdx.x * F8G_BN;
    const int m0 = blockIdx.y * F8G_BM;
    const int split = blockIdx.z;
    const int64_t kb64 = (int64_t)split * kper;
    const int k_begin = kb64 < K ? (int)kb64 : K;
    const int k_end = (kb64 + kper < K) ? (int)(kb64 + kper) : K;

    __shared__ __attribute__((aligned(16))) uint8_t Wl[F8G_BN * F8G_WS];
    __shared__ __attribute__((aligned(16))) __bf16 Xl[F8G_BM * F8G_XS];

    const uint8_t* wrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + (threadIdx.x >> 3) + 32 * i;
        wrow[i] = wq + (int64_t)(n < N ? n : N - 1) * K;
    }

    f32x4 acc[4][4];  // [channel block][row block]
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) acc[cb][rb] = {0.f, 0.f, 0.f, 0.f};

    u32x4 wr[4], xr[8];
    const int row0 = m0 + (threadIdx.x >> 4);
    const __bf16* xrow = x + (int64_t)row0 * xs;
    f8g_load_w(wrow, k_begin, k_end, wr);
    f8g_load_x(x, xrow, xs, row0, M, k_begin, k_end, xr);

    // staging offsets of the thread's pieces (row step: 32 rows of W, 16 of x)
    const int w_st = (threadIdx.x >> 3) * F8G_WS + (threadIdx.x & 7) * 16;
    const int xj = (threadIdx.x & 15) * 8;  // natural offset in the tile: 64c + 16g + 8h
    const int x_st = (threadIdx.x >> 4) * F8G_XS + ((xj & ~63) | ((xj & 8) << 2) | ((xj & 48) >> 1));  // 64c + 32h + 8g
    // fragment offsets of the lane
    const int w_fr = (wn * 64 + lr) * F8G_WS + lg * 16;
    const int x_fr = (wm * 64 + lr) * F8G_XS + lg * 8;

    for (int k0 = k_begin; k0 < k_end; k0 += F8G_BK) {
        __syncthreads();  // the previous tile's fragment reads are done
        const u32x4 zero = {0u, 0u, 0u, 0u};
        const bool w_in = k0 + (threadIdx.x & 7) * 16 < k_end;
        const bool x_in = k0 + xj < k_end;
#pragma unroll
        for (int i = 0; i < 4; ++i) *(u32x4*)&Wl[w_st + 32 * i * F8G_WS] = w_in ? wr[i] : zero;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            *(u32x4*)&Xl[x_st + 16 * i * F8G_XS] = (x_in && row0 + 16 * i < M) ? xr[i] : zero;
        __syncthreads();

        // next tile's loads first: they fly under this tile's MFMAs
        if (k0 + F8G_BK < k_end) {
            f8g_load_w(wrow, k0 + F8G_BK, k_end, wr);
            f8g_load_x(x, xrow, xs, row0, M, k0 + F8G_BK, k_end, xr);
        }

#pragma unroll
        for (int c = 0; c < F8G_BK / 64; ++c) {
            u32x4 wf[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) wf[cb] = *(const u32x4*)&Wl[w_fr + cb * 16 * F8G_WS + c * 64];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                bf16x8 a[4], b[4];
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    u32x2 half;
                    half[0] = wf[cb][2 * h];
                    half[1] = wf[cb][2 * h + 1];
                    a[cb] = e4m3x8_to_bf16x8(half);
                }
#pragma unroll
                for (int rb = 0; rb < 4; ++rb)
                    b[rb] = *(const bf16x8*)&Xl[x_fr + rb * 16 * F8G_XS + c * 64 + h * 32];
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) acc[cb][rb] = MFMA16(a[cb], b[rb], acc[cb][rb]);
            }
        }
    }

    // lane: channels nb .. nb + 3 (per channel block) of rows mr + 16*rb
    const bool vec = (N & 3) == 0;  // nb % 4 == 0: the 4 channels are inside N and the store aligned
    const int mr = m0 + wm * 64 + lr;

#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        const int nb = n0 + wn * 64 + cb * 16 + lg * 4;
        if (nb >= N) continue;
        float sc[4] = {}, bs[4] = {};
        if (nsplit == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = (nb + r < N) ? nb + r : N - 1;
                sc[r] = wscale[n];
                bs[r] = bias ? (float)bias[n] : 0.f;
            }
        }
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            const int m = mr + rb * 16;
            if (m >= M) continue;
            if (nsplit > 1) {
                float* dst = part + ((int64_t)split * M + m) * N + nb;
                if (vec) {
                    *(f32x4*)dst = acc[cb][rb];
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (nb + r < N) dst[r] = acc[cb][rb][r];
                }
                continue;
            }
            bf16x4 ov;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] = (__bf16)(acc[cb][rb][r] * sc[r] + bs[r]);
            __bf16* dst = y + (int64_t)m * N + nb;
            if (vec) {
                *(bf16x4*)dst = ov;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (nb + r < N) dst[r] = ov[r];
            }
        }
    }
}

// Join of the split partials (fp8_linear.hip's, a second copy: that file's
// build stays as it was measured): one thread per output element, ascending
// split order, then the one-split epilogue's scale, bias and rounding.
__global__ void __launch_bounds__(256) fp8_gemm_join_kernel(
    const float* __restrict__ part, const float* __restrict__ wscale, const __bf16* __restrict__ bias,
    __bf16* __restrict__ y, int64_t MN, int N, int nsplit) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= MN) return;
    const int n = (int)(i % N);
    float s = part[i];
    for (int c = 1; c < nsplit; ++c) s += part[(int64_t)c * MN + i];
    y[i] = (__bf16)(s * wscale[n] + (bias ? (float)bias[n] : 0.f));
}

static bool f8g_sizes_ok(int64_t M, int64_t N, int64_t K) {
    return N >= 1 && N < ((int64_t)1 << 31) && K <= ((int64_t)1 << 30) && M * N <= ((int64_t)1 << 38);
}

static bool f8g_dims_ok(int64_t M, int64_t N, int64_t K) {
    return M >= 1 && M <= (int64_t)F8G_MAX_MTILES * F8G_BM && K >= 16 && K % 16 == 0 && f8g_sizes_ok(M, N, K);
}

// Default split count: the candidate with the least estimated time, in us,
// the smaller count on a tie. The estimate is a fit to the first table of
// profiles/fp8_gemm_ab.txt (header: "Filling the machine").
extern "C" int dolomite_fp8_gemm_num_splits(int64_t M, int64_t N, int64_t K) {
    if (!f8g_dims_ok(M, N, K)) return -1;
    const int64_t tiles = ((N + F8G_BN - 1) / F8G_BN) * ((M + F8G_BM - 1) / F8G_BM);
    const int64_t ktiles = (K + F8G_BK - 1) / F8G_BK;
    const int64_t max_ns = ktiles / 2 < 64 ? ktiles / 2 : 64;  // two k tiles per split at least
    const double part_us = (double)M * (double)N * 8.0 / 4.0e6;  // a split's partials, written and read at 4 TB/s
    int best = 1;
    double best_t = 0.0;
    for (int64_t ns = 1; ns <= (max_ns > 1 ? max_ns : 1); ++ns) {
        const int64_t kt = (ktiles + ns - 1) / ns;           // k tiles per split
        if ((ktiles + kt - 1) / kt != ns) continue;          // no empty split
        const int64_t r = (tiles * ns + 255) / 256;          // workgroups on the busiest of the 256 CUs
        const double cu = (double)(kt + 1) * (r == 1 ? 1.9 : 1.33 * (double)r);
        const double t = cu + (ns > 1 ? 4.0 + (double)ns * (0.5 + part_us) : 0.0);
        if (ns == 1 || t < best_t) {
            best = (int)ns;
            best_t = t;
        }
    }
    return best;
}

extern "C" int64_t dolomite_fp8_gemm_scratch_floats(int64_t M, int64_t N, int64_t K, int nsplit) {
    if (!f8g_dims_ok(M, N, K) || nsplit < 1 || nsplit > 65535) return -1;
    return nsplit > 1 ? (int64_t)nsplit * M * N : 0;
}

extern "C" int dolomite_fp8_gemm(dolomite_stream_t stream, const void* x, const void* wq,
                                 const float* wscale, const void* bias, void* y, float* scratch,
                                 int64_t M, int64_t N, int64_t K, int64_t x_row_stride,
                                 int nsplit, int dtype) {
    if (dtype != DOLOMITE_BF16) return 9010;
    if (M < 1) return 9080;
    if (M > (int64_t)F8G_MAX_MTILES * F8G_BM) return 9081;
    if (K < 16 || K % 16 != 0) return 9082;
    if (!f8g_sizes_ok(M, N, K)) return 9083;
    if (x_row_stride < K || x_row_stride % 8 != 0 || ((uintptr_t)x & 15) || ((uintptr_t)wq & 15) ||
        ((uintptr_t)y & 7) || ((uintptr_t)scratch & 15))
        return 9084;
    if (nsplit < 1 || nsplit > 65535) return 9085;
    if (nsplit > 1 && scratch == nullptr) return 9086;
    if (!x || !wq || !wscale || !y) return 9087;

    hipStream_t s = (hipStream_t)stream;
    const int64_t ktiles = (K + F8G_BK - 1) / F8G_BK;
    const int kper = (int)((ktiles + nsplit - 1) / nsplit) * F8G_BK;
    const dim3 grid((unsigned)((N + F8G_BN - 1) / F8G_BN), (unsigned)((M + F8G_BM - 1) / F8G_BM), (unsigned)nsplit);
    hipLaunchKernelGGL(fp8_gemm_kernel, grid, dim3(256), 0, s, (const __bf16*)x, (const uint8_t*)wq, wscale,
                       (const __bf16*)bias, (__bf16*)y, scratch, (int)M, (int)N, (int)K, x_row_stride, kper,
                       nsplit);
    int err = dol_last_error();
    if (err != 0 || nsplit == 1) return err;

    const int64_t MN = M * N;
    hipLaunchKernelGGL(fp8_gemm_join_kernel, dim3((unsigned)((MN + 255) / 256)), dim3(256), 0, s,
                       (const float*)scratch, wscale, (const __bf16*)bias, (__bf16*)y, MN, (int)N, nsplit);
    return dol_last_error();
}
