// dolomite_hip — fp8 (OCP e4m3) weight-only linear for gfx950 (MI355X): the
// skinny GEMM of a decode / short extend step (W8A16).
//
//   y[M, N] = x[M, K] @ (Wq[N, K] * wscale[N, None])^T (+ bias[N]),  1 <= M <= 64
//
// x, bias, y bf16; Wq e4m3 bytes, dense (N, K); wscale fp32, one per output
// channel (the rule of quantize_weight_e4m3: amax / 448 per weight row). With
// so few rows every linear is bound by the HBM read of its weight, which this
// kernel halves; the design keeps that stream wide and deep, MFMA utilisation
// is not a goal.
//
// Work split: grid (ceil(N / 64), nsplit), 256 threads. A wave owns one slab
// of 16 output channels, a workgroup four consecutive slabs, and split c of
// the contraction owns k in [c*kper, min((c+1)*kper, K)), kper a multiple of
// the 64-wide chunk (dolomite_fp8_linear_num_splits picks nsplit; a split
// without k is legal and contributes zeros). A workgroup walks its k range in
// tiles of 256.
//
// Operands: v_mfma_f32_16x16x32_bf16 with A = the W slab (row = channel
// n0 + (lane & 15)) and B = a 16-row block of x (row = lane & 15), so the
// accumulator holds, on lane l and register r, channel n0 + 4*(l >> 4) + r of
// row l & 15: four consecutive channels per lane, one 8-byte bf16 store (or
// one 16-byte fp32 store into the split partials) per row block.
//
// Weight stream: per tile a lane issues four independent 16-byte nontemporal
// loads; load i takes bytes k0 + 16*(lane & 15) + [0, 16) of slab row
// 4i + (lane >> 4), so 16 consecutive lanes read 256 contiguous bytes of one
// row and a wave instruction four whole 256-byte row segments. The loads of
// tile t+1 (and the x pieces of tile t+1, below) are issued before the MFMAs
// of tile t, so no MFMA waits on a load of its own tile. The registers are
// stored to a wave-private LDS image of the slab ([16 rows][256 + 16 bytes])
// and read back as fragments: lane (row lane & 15, group g = lane >> 4) reads,
// per 64-wide chunk c, the 16 bytes at 64c + 16g with one b128 read. Each
// 8-byte half h is converted with e4m3x8_to_bf16x8 (exact) and feeds one MFMA;
// every one of the 1 to 4 row blocks of x reuses the same converted registers,
// so Wq is read once whatever M is.
//
// Why the LDS pass: the first version loaded the fragment form straight from
// HBM (lane = row lane & 15, 16 bytes at 64c + 16g: 64 contiguous bytes per
// row, 16 rows per wave instruction). Consecutive lanes then sit on different
// rows, every 16-byte lane request is a cache line of its own to the vector
// memory pipeline, and the kernel stopped near 2.0 TB/s (mlp.c_fc of the 3B
// config, M = 1: 12.6 us; 16.4 us before masked-off loads were skipped
// instead of redirected). The coalesced loads with the LDS pass took the same
// call to 9.9 us (2.65 TB/s) and won at every shape and M measured
// (profiles/fp8_linear_ab.txt). The 4 KB per wave and tile through LDS are
// small next to the x fragment reads.
//
// k permutation: MFMA h of chunk c contracts, on lane group g = lane >> 4 and
// element e, the weight at k = k0 + 64c + 16g + 8h + e, where the natural
// fragment would hold k0 + 64c + 32h + 8g + e. The x image in LDS is written
// in that permuted order — the 8-element piece at offset 16g + 8h of a chunk
// is stored at offset 32h + 8g — so the B fragments are plain
// "row lane & 15, 8 contiguous at 32h + 8g" b128 reads, the pattern (and the
// cols + 16 stride rule) of moe_gemm.hip, and each product pairs x_k with w_k.
//
// Activations: the tile's M x 256 slice of x is loaded as 16-byte pieces into
// registers one tile ahead, then stored to a row-major image of stride
// 256 + 16 and shared by the four waves. Rows at and beyond M, and k at and
// beyond the split's end, are not loaded and stored as zeros (the weight bytes
// of such k too), so nothing outside the operands reaches an accumulator.
// Channels at and beyond N load row N - 1 and are never stored.
//
// Split count (dolomite_fp8_linear_num_splits): about one workgroup per CU.
// The first rule aimed at two; a sweep over half / twice / four times the
// default at the 3B shapes, M = 1 .. 64, had half as many splits faster or
// equal at every shape (attn.c_attn M = 1: 6.4 us with 5 splits, 7.4 with 10,
// 9.9 with 20), so the target became 256 workgroups.
//
// Scale and bias: nothing is applied per element. The fp32 accumulator is
// multiplied by wscale[n] once, then the bias is added, then one rounding to
// bf16.
//
// Split-K join: with nsplit == 1 the kernel runs that epilogue itself. With
// nsplit > 1 each workgroup stores its fp32 partials exclusively into
// scratch[c][m][n] and a second launch sums them in ascending c, applies scale
// and bias and rounds: no atomics, bitwise reproducible for fixed arguments.
//
// Built as an object of its own with packed fp32 VALU ops off, the flags of
// the other fp8 kernels whose conversion helper it shares: its only fp32 VALU
// work is the epilogue's multiply-add per element, which packing cannot help,
// and the sources of the one-command build keep the build they were measured
// with.

#include "mfma_tiles.h"

#define F8L_WAVES 4                  // waves (= 16-channel slabs) per workgroup
#define F8L_CHUNK 64                 // k per 16-byte weight load of a wave row
#define F8L_TILE 256                 // k per staged x tile: 4 chunks
#define F8L_XS (F8L_TILE + 16)       // LDS row stride of the x image, elements
#define F8L_WS (F8L_TILE + 16)       // LDS row stride of a wave's W slab image, bytes
#define F8L_MAX_M 64

// The tile's four weight loads of one lane, coalesced: load i takes bytes
// k0 + 16*(lane & 15) + [0, 16) of slab row 4i + (lane >> 4), so 16 consecutive
// lanes read 256 contiguous bytes of one row. k at and beyond k_end is not
// loaded and gives zeros.
__device__ __forceinline__ void f8l_load_w(const uint8_t* const (&wrow)[4], int k0, int k_end, int lr,
                                           u32x4 (&w)[4]) {
    const int k = k0 + lr * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = u32x4{0u, 0u, 0u, 0u};
        if (k < k_end) w[i] = __builtin_nontemporal_load((const u32x4*)(wrow[i] + k));
    }
}

// The tile's x pieces of one thread: piece p = tid + 256*i is row p >> 5,
// elements 8*(p & 31) .. +8 of the tile. Rows >= M and k >= k_end are not
// loaded and give zeros.
template <int MB>
__device__ __forceinline__ void f8l_load_x(const __bf16* x, int64_t xs, int M, int k0, int k_end,
                                           u32x4 (&xr)[2 * MB]) {
#pragma unroll
    for (int i = 0; i < 2 * MB; ++i) {
        const int p = threadIdx.x + 256 * i;
        const int row = p >> 5;
        const int k = k0 + (p & 31) * 8;
        xr[i] = u32x4{0u, 0u, 0u, 0u};
        if (row < M && k < k_end) xr[i] = *(const u32x4*)(x + (int64_t)row * xs + k);
    }
}

template <int MB>
__global__ void __launch_bounds__(F8L_WAVES * 64) fp8_linear_kernel(
    const __bf16* __restrict__ x, const uint8_t* __restrict__ wq, const float* __restrict__ wscale,
    const __bf16* __restrict__ bias, __bf16* __restrict__ y, float* __restrict__ part,
    int M, int N, int K, int64_t xs, int kper, int nsplit) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lr = lane & 15;
    const int lg = lane >> 4;

    const int n0 = (blockIdx.x * F8L_WAVES + wave) * 16;
    const int split = blockIdx.y;
    const int64_t kb64 = (int64_t)split * kper;
    const int k_begin = kb64 < K ? (int)kb64 : K;
    const int k_end = (kb64 + kper < K) ? (int)(kb64 + kper) : K;

    __shared__ __attribute__((aligned(16))) __bf16 Xl[MB * 16 * F8L_XS];
    __shared__ __attribute__((aligned(16))) uint8_t Wl[F8L_WAVES * 16 * F8L_WS];
    uint8_t* Ww = Wl + wave * 16 * F8L_WS;  // the wave's own slab image

    const uint8_t* wrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + 4 * i + lg;
        wrow[i] = wq + (int64_t)(n < N ? n : N - 1) * K;
    }

    f32x4 acc[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[mb] = {0.f, 0.f, 0.f, 0.f};

    u32x4 wr[4], xr[2 * MB];
    f8l_load_w(wrow, k_begin, k_end, lr, wr);
    f8l_load_x<MB>(x, xs, M, k_begin, k_end, xr);

    for (int k0 = k_begin; k0 < k_end; k0 += F8L_TILE) {
        __syncthreads();  // the previous tile's fragment reads are done
#pragma unroll
        for (int i = 0; i < 2 * MB; ++i) {
            const int p = threadIdx.x + 256 * i;
            const int row = p >> 5;
            const int j = (p & 31) * 8;  // natural offset in the tile: 64c + 16g + 8h
            const int pos = (j & ~63) | ((j & 8) << 2) | ((j & 48) >> 1);  // 64c + 32h + 8g
            *(u32x4*)&Xl[row * F8L_XS + pos] = xr[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) *(u32x4*)&Ww[(4 * i + lg) * F8L_WS + lr * 16] = wr[i];
        __syncthreads();

        // next tile's loads first: they fly under this tile's MFMAs
        u32x4 wnx[4] = {};
        if (k0 + F8L_TILE < k_end) {
            f8l_load_w(wrow, k0 + F8L_TILE, k_end, lr, wnx);
            f8l_load_x<MB>(x, xs, M, k0 + F8L_TILE, k_end, xr);
        }

#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const u32x4 wf = *(const u32x4*)&Ww[lr * F8L_WS + c * F8L_CHUNK + lg * 16];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                u32x2 half;
                half[0] = wf[2 * h];
                half[1] = wf[2 * h + 1];
                const bf16x8 a = e4m3x8_to_bf16x8(half);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const bf16x8 b = *(const bf16x8*)&Xl[(mb * 16 + lr) * F8L_XS + c * 64 + h * 32 + lg * 8];
                    acc[mb] = MFMA16(a, b, acc[mb]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) wr[c] = wnx[c];
    }

    // lane: channels nb .. nb + 3 of rows mb*16 + lr
    const int nb = n0 + lg * 4;
    if (nb >= N) return;
    const bool vec = (N & 3) == 0;  // nb % 4 == 0: the 4 channels are inside N and the store aligned

    if (nsplit > 1) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int m = mb * 16 + lr;
            if (m >= M) continue;
            float* dst = part + ((int64_t)split * M + m) * N + nb;
            if (vec) {
                *(f32x4*)dst = acc[mb];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (nb + r < N) dst[r] = acc[mb][r];
            }
        }
        return;
    }

    float sc[4], bs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = (nb + r < N) ? nb + r : N - 1;
        sc[r] = wscale[n];
        bs[r] = bias ? (float)bias[n] : 0.f;
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int m = mb * 16 + lr;
        if (m >= M) continue;
        bf16x4 ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) ov[r] = (__bf16)(acc[mb][r] * sc[r] + bs[r]);
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

// Join of the split partials: one thread per output element, ascending split
// order, then the one-split epilogue's scale, bias and rounding.
__global__ void __launch_bounds__(256) fp8_linear_join_kernel(
    const float* __restrict__ part, const float* __restrict__ wscale, const __bf16* __restrict__ bias,
    __bf16* __restrict__ y, int64_t MN, int N, int nsplit) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= MN) return;
    const int n = (int)(i % N);
    float s = part[i];
    for (int c = 1; c < nsplit; ++c) s += part[(int64_t)c * MN + i];
    y[i] = (__bf16)(s * wscale[n] + (bias ? (float)bias[n] : 0.f));
}

static bool f8l_dims_ok(int64_t M, int64_t N, int64_t K) {
    return M >= 1 && M <= F8L_MAX_M && N >= 1 && N < ((int64_t)1 << 31) && K >= 16 &&
           K <= ((int64_t)1 << 30) && K % 16 == 0;
}

extern "C" int dolomite_fp8_linear_num_splits(int64_t M, int64_t N, int64_t K) {
    if (!f8l_dims_ok(M, N, K)) return -1;
    const int64_t groups = (N + 16 * F8L_WAVES - 1) / (16 * F8L_WAVES);
    const int64_t chunks = (K + F8L_CHUNK - 1) / F8L_CHUNK;
    const int64_t want = (256 + groups - 1) / groups;     // one workgroup on each of the 256 CUs (measured: header)
    const int64_t by_k = (chunks + 3) / 4;                 // a 256-wide tile per split at least
    const int64_t by_m = K / (8 * M) > 1 ? K / (8 * M) : 1;  // partials (written, read back) <= the weight bytes
    int64_t ns = want < by_k ? want : by_k;
    ns = ns < by_m ? ns : by_m;
    if (ns < 1) ns = 1;
    const int64_t kper = (chunks + ns - 1) / ns;           // chunks per split
    return (int)((chunks + kper - 1) / kper);              // no empty split
}

extern "C" int64_t dolomite_fp8_linear_scratch_floats(int64_t M, int64_t N, int64_t K, int nsplit) {
    if (!f8l_dims_ok(M, N, K) || nsplit < 1 || nsplit > 65535) return -1;
    return nsplit > 1 ? (int64_t)nsplit * M * N : 0;
}

extern "C" int dolomite_fp8_linear(dolomite_stream_t stream, const void* x, const void* wq,
                                   const float* wscale, const void* bias, void* y, float* scratch,
                                   int64_t M, int64_t N, int64_t K, int64_t x_row_stride,
                                   int nsplit, int dtype) {
    if (dtype != DOLOMITE_BF16) return 9010;
    if (M < 1) return 9070;
    if (M > F8L_MAX_M) return 9071;
    if (K < 16 || K % 16 != 0) return 9072;
    if (N < 1 || N >= ((int64_t)1 << 31) || K > ((int64_t)1 << 30)) return 9073;
    if (x_row_stride < K || x_row_stride % 8 != 0 || ((uintptr_t)x & 15) || ((uintptr_t)wq & 15) ||
        ((uintptr_t)y & 7) || ((uintptr_t)scratch & 15))
        return 9074;
    if (nsplit < 1 || nsplit > 65535) return 9075;
    if (nsplit > 1 && scratch == nullptr) return 9076;
    if (!x || !wq || !wscale || !y) return 9077;

    hipStream_t s = (hipStream_t)stream;
    const int64_t chunks = (K + F8L_CHUNK - 1) / F8L_CHUNK;
    const int kper = (int)((chunks + nsplit - 1) / nsplit) * F8L_CHUNK;
    const dim3 grid((unsigned)((N + 16 * F8L_WAVES - 1) / (16 * F8L_WAVES)), (unsigned)nsplit);
    const dim3 block(F8L_WAVES * 64);
    const int mb = (int)((M + 15) / 16);

#define F8L_LAUNCH(MB)                                                                            \
    hipLaunchKernelGGL(fp8_linear_kernel<MB>, grid, block, 0, s, (const __bf16*)x,                \
                       (const uint8_t*)wq, wscale, (const __bf16*)bias, (__bf16*)y, scratch,      \
                       (int)M, (int)N, (int)K, x_row_stride, kper, nsplit)
    switch (mb) {
        case 1: F8L_LAUNCH(1); break;
        case 2: F8L_LAUNCH(2); break;
        case 3: F8L_LAUNCH(3); break;
        default: F8L_LAUNCH(4); break;
    }
#undef F8L_LAUNCH
    int err = dol_last_error();
    if (err != 0 || nsplit == 1) return err;

    const int64_t MN = M * N;
    hipLaunchKernelGGL(fp8_linear_join_kernel, dim3((unsigned)((MN + 255) / 256)), dim3(256), 0, s,
                       (const float*)scratch, wscale, (const __bf16*)bias, (__bf16*)y, MN, (int)N, nsplit);
    return dol_last_error();
}
