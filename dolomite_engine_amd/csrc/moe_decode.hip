// dolomite_hip — fused expert MLP of a MoE decode / short extend step for
// gfx950 (MI355X): at most 64 tokens, top-k routed over E <= 64 experts.
//
//   out[t] = sum_j gates[t,j] * (W_proj[e] act(W_fc[e] x[t] + b_fc[e]) + b_proj[e]),
//   e = selected[t,j], summed in ascending j
//
// x, weights, biases, gates, out bf16; accumulation fp32; the intermediate h
// and the output are each rounded to bf16 once. With so few rows every live
// expert is bound by the HBM read of its two weight matrices, exactly as the
// dense linears of fp8_linear.hip are, so this file keeps that kernel's
// shape: a wide coalesced weight stream, MFMA only as the dot-product engine,
// and nothing else on the critical path. What is new is that the rows of an
// expert are found, gathered and scattered inside the kernel, so the step
// needs no expert sort, no host readback and no atomics:
//
//   A. fc + activation   grid (channel tiles of I, E)   h[pair, :]  bf16 (T*k, I)
//   B. proj              grid (channel tiles of H, E)   part[pair, :] fp32 (T*k, H)
//                        = (acc + b_proj) * gate[pair]
//   C. combine           out[t] = sum_j part[t*k + j], ascending j, one rounding
//
// A and B are one kernel template (MODE). Pair p = t*k + j is the only row
// order anywhere: h and part are pair-major, an expert-sorted order does not
// exist. Every element of h, part and out that a valid `selected` names is
// written exactly once by exactly one lane, so two calls with the same
// arguments are bitwise equal.
//
// Pair list: a workgroup of expert e scans the T*k <= 512 entries of
// `selected` (every wave scans for itself: 8 coalesced loads, a ballot and a
// popcount each, so the count is known without a barrier) and wave 0 writes
// the matching pairs in ascending pair order to a 64-entry list in LDS. An
// expert nobody chose returns there: a few hundred bytes read, none of its
// weight touched (and nothing of it multiplied by a zero gate). Ids in a row
// of `selected` are distinct, so a list holds at most T <= 64 pairs; entries
// past 64 (an invalid `selected`) are dropped, ids outside [0, E) match no
// expert, and neither can move an access out of bounds.
//
// Operands: v_mfma_f32_16x16x32_bf16 with A = a 16-channel weight slab (row =
// channel n0 + (lane & 15)) and B = a 16-row block of the expert's list (row =
// lane & 15), so lane l, register r holds channel n0 + 4*(l >> 4) + r of list
// row l & 15: four consecutive channels, one 8-byte bf16 store (A) or one
// 16-byte fp32 store (B) per row block. 1 to 4 row blocks reuse the same A
// fragment, so a slab is read from HBM once however many tokens chose e.
//
// Weight stream (the lesson of fp8_linear.hip: row-segment loads, not
// fragment-shaped ones): per 128-wide k tile a lane issues four 16-byte
// nontemporal loads per slab; load i takes elements k0 + 8*(lane & 15) + [0, 8)
// of slab row 4i + (lane >> 4), so 16 consecutive lanes read 256 contiguous
// bytes of one row. The loads of tile t+1 are issued before the MFMAs of tile
// t. The registers go to a wave-private LDS image ([16][128 + 8] bf16) and
// come back as natural fragments (row lane & 15, 8 elements at 32c + 8g: one
// b128 read per 32-wide chunk c); the stride of 68 dwords spreads the 16 rows
// of such a read over all 64 banks.
//
// GLU: the wave that owns channels [n, n + 16) of the `a` half also streams
// rows [I + n, I + n + 16) of the `b` half into a second image and a second
// accumulator, so the epilogue forms (a + bias_a) * act(b + bias_b) in fp32
// and h never exists in its 2I-wide form.
//
// Gather: the B operand's rows are x[list[r] / k] (launch A) or h[list[r]]
// (launch B). Each thread resolves the source rows of its 16-byte pieces once
// and loads them a tile ahead into registers, then stores them to a row-major
// LDS image ([16 MB][128 + 8]) shared by the workgroup's waves. Rows at and
// beyond the list's length and k at and beyond K are stored as zeros (so are
// the weight's), channels at and beyond N load row N - 1 and are never
// stored. Only K % 8 == 0 and N % 8 == 0 are required.
//
// Occupancy rule (md_waves): a workgroup is W in {4, 2, 1} waves = W slabs of
// 16 channels, and the grid has ceil(ceil(N / 16) / W) * E workgroups of which
// only those of live experts stream anything. At most min(E, T*k) experts are
// live, a bound that depends on the shapes alone, so W is the largest of
// 4, 2, 1 for which ceil(ceil(N / 16) / W) * min(E, T*k) reaches the 256 CUs,
// else 1. At T = 1, k = 2, N = 1024 that is W = 1: 128 one-wave workgroups
// instead of 32 four-wave ones. A split over the contraction was not taken:
// launch A applies a nonlinearity to the complete sum, so a split needs a
// fourth launch. The rule never looks at `selected`, so the launch and the
// summation order are functions of the shapes. Measured at E = 32, k = 2,
// H = I = 1024 with W forced (profiles/moe_decode_ab.txt; us per MLP call from
// Python, gate linear and routing included): T = 64, where the rule takes 4,
// W = 1 / 2 / 4 gave 86.5 / 64.7 / 64.7; at T = 1, 4, 16 (rule: 1, 2, 4) all
// three gave 64.8 to 65.2, the floor of the call's five launches as issued
// from Python, so those shapes do not separate the alternatives and the
// small-T end of the rule rests on the workgroup count alone.
//
// Built with packed fp32 VALU ops off, as fp8_linear.hip is: the fp32 VALU
// work is the epilogue alone.

#include "mfma_tiles.h"

#include <math.h>

#define MD_TILE 128              // k per staged tile: 4 MFMA chunks of 32
#define MD_LS (MD_TILE + 8)      // LDS row stride of both images, elements
#define MD_MAX_T 64
#define MD_MAX_E 64
#define MD_MAX_K 8

#define MD_FC 0                  // h = act(W x + b)
#define MD_FC_GLU 1              // h = (Wa x + ba) * act(Wb x + bb)
#define MD_PROJ 2                // part = (W h + b) * gate

// The forward halves of elementwise.hip's glu_act_grad, same expressions.
__device__ __forceinline__ float md_act(int act, float x) {
    switch (act) {
        case DOLOMITE_ACT_SILU:
            return x * __builtin_amdgcn_rcpf(1.f + expf(-x));
        case DOLOMITE_ACT_GELU_TANH: {
            const float k0 = 0.7978845608028654f, k1 = 0.044715f;
            const float u = k0 * x * (1.f + k1 * x * x);
            const float e = expf(-2.f * fabsf(u));
            const float r = __builtin_amdgcn_rcpf(1.f + e);
            return x * (u < 0.f ? e * r : r);
        }
        case DOLOMITE_ACT_GELU:
            return x * 0.5f * (1.f + erff(x * 0.7071067811865476f));
        default:
            return fmaxf(x, 0.f);
    }
}

// One slab's four weight loads of a lane for the tile at k0 (header: Weight
// stream). k at and beyond K is not loaded and gives zeros.
__device__ __forceinline__ void md_load_w(const __bf16* const (&wrow)[4], int k0, int K, int lr, u32x4 (&w)[4]) {
    const int k = k0 + lr * 8;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = u32x4{0u, 0u, 0u, 0u};
        if (k < K) w[i] = __builtin_nontemporal_load((const u32x4*)(wrow[i] + k));
    }
}

// The tile's gathered pieces of one thread: piece i sits at xsrc[i] + k0
// (xsrc already holds the piece's column offset), NULL for a row beyond the list.
template <int NP>
__device__ __forceinline__ void md_load_x(const __bf16* const (&xsrc)[NP], const int (&xcol)[NP], int k0, int K,
                                          u32x4 (&xr)[NP]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        xr[i] = u32x4{0u, 0u, 0u, 0u};
        if (xsrc[i] != nullptr && k0 + xcol[i] < K) xr[i] = *(const u32x4*)(xsrc[i] + k0);
    }
}

// MB: 16-row blocks the shapes allow (ceil(T / 16) rounded up to 1, 2, 4);
// W: waves per workgroup; MODE: MD_FC / MD_FC_GLU / MD_PROJ.
//   src: x (row stride K, row = pair / row_div with row_div = k) for the fc
//   modes, h (row = pair, row_div = 1) for MD_PROJ. w: (E, N or 2N, K),
//   bias (E, N or 2N) or NULL. Output row = pair: h_out (pairs, N) bf16 or
//   part_out (pairs, N) fp32.
template <int MB, int W, int MODE>
__global__ void __launch_bounds__(W * 64) moe_decode_kernel(
    const __bf16* __restrict__ src, int row_div, const int32_t* __restrict__ selected,
    const __bf16* __restrict__ gates, const __bf16* __restrict__ w, const __bf16* __restrict__ bias,
    __bf16* __restrict__ h_out, float* __restrict__ part_out, int n_pairs, int N, int K, int act) {
    constexpr int NT = W * 64;
    constexpr int NP = MB * 256 / NT;           // 16-byte x pieces per thread and tile
    constexpr int NS = MODE == MD_FC_GLU ? 2 : 1;  // slabs per wave
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int lr = lane & 15;
    const int lg = lane >> 4;
    const int e = blockIdx.y;

    __shared__ int plist[MD_MAX_T];
    __shared__ __attribute__((aligned(16))) __bf16 Xl[MB * 16 * MD_LS];
    __shared__ __attribute__((aligned(16))) __bf16 Wl[W * NS * 16 * MD_LS];

    // ---- the expert's pairs, ascending; every wave counts, wave 0 writes ----
    int cnt = 0;
    for (int c0 = 0; c0 < n_pairs; c0 += 64) {
        const int p = c0 + lane;
        const bool mine = p < n_pairs && selected[p] == e;
        const unsigned long long bal = __ballot(mine);
        if (wave == 0 && mine) {
            const int slot = cnt + __popcll(bal & ((1ull << lane) - 1ull));
            if (slot < MD_MAX_T) plist[slot] = p;
        }
        cnt += __popcll(bal);
    }
    if (cnt == 0) return;  // uniform over the workgroup: an idle expert reads no weight
    if (cnt > MD_MAX_T) cnt = MD_MAX_T;
    const int nblk = (cnt + 15) >> 4;  // live row blocks, <= MB

    const int n0 = (blockIdx.x * W + wave) * 16;
    const int wrows = NS * N;
    const __bf16* we = w + (int64_t)e * wrows * K;
    const __bf16* wrow[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + 4 * i + lg;
            wrow[s][i] = we + (int64_t)(s * N + (n < N ? n : N - 1)) * K;
        }

    u32x4 wr[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s) md_load_w(wrow[s], 0, K, lr, wr[s]);  // in flight across the barrier

    __syncthreads();  // plist
    const __bf16* xsrc[NP];
    int xcol[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int p = tid + NT * i;
        const int row = p >> 4;
        xcol[i] = (p & 15) * 8;
        xsrc[i] = nullptr;
        if (row < cnt) xsrc[i] = src + (int64_t)(plist[row] / row_div) * K + xcol[i];
    }
    u32x4 xr[NP];
    md_load_x<NP>(xsrc, xcol, 0, K, xr);

    f32x4 acc[NS][MB];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[s][mb] = {0.f, 0.f, 0.f, 0.f};

    __bf16* Ww = Wl + wave * NS * 16 * MD_LS;  // the wave's own slab images

    for (int k0 = 0; k0 < K; k0 += MD_TILE) {
        __syncthreads();  // the previous tile's fragment reads are done
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = tid + NT * i;
            *(u32x4*)&Xl[(p >> 4) * MD_LS + xcol[i]] = xr[i];
        }
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) *(u32x4*)&Ww[(s * 16 + 4 * i + lg) * MD_LS + lr * 8] = wr[s][i];
        __syncthreads();

        // next tile's loads first: they fly under this tile's MFMAs
        u32x4 wnx[NS][4] = {};
        if (k0 + MD_TILE < K) {
#pragma unroll
            for (int s = 0; s < NS; ++s) md_load_w(wrow[s], k0 + MD_TILE, K, lr, wnx[s]);
            md_load_x<NP>(xsrc, xcol, k0 + MD_TILE, K, xr);
        }

#pragma unroll
        for (int c = 0; c < MD_TILE / 32; ++c) {
            bf16x8 a[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) a[s] = *(const bf16x8*)&Ww[(s * 16 + lr) * MD_LS + c * 32 + lg * 8];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                if (mb < nblk) {
                    const bf16x8 b = *(const bf16x8*)&Xl[(mb * 16 + lr) * MD_LS + c * 32 + lg * 8];
#pragma unroll
                    for (int s = 0; s < NS; ++s) acc[s][mb] = MFMA16(a[s], b, acc[s][mb]);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i) wr[s][i] = wnx[s][i];
    }

    // lane: channels nb .. nb + 3 (N % 8 == 0: all inside N or all outside) of list rows mb*16 + lr
    const int nb = n0 + lg * 4;
    if (nb >= N) return;
    float bs[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) bs[s][r] = bias ? (float)bias[(int64_t)e * wrows + s * N + nb + r] : 0.f;

#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int row = mb * 16 + lr;
        if (row >= cnt) continue;
        const int pair = plist[row];
        if constexpr (MODE == MD_PROJ) {
            const float g = (float)gates[pair];
            f32x4 ov;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] = (acc[0][mb][r] + bs[0][r]) * g;
            *(f32x4*)(part_out + (int64_t)pair * N + nb) = ov;
        } else {
            bf16x4 ov;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (MODE == MD_FC_GLU)
                    ov[r] = (__bf16)((acc[0][mb][r] + bs[0][r]) * md_act(act, acc[1][mb][r] + bs[1][r]));
                else
                    ov[r] = (__bf16)md_act(act, acc[0][mb][r] + bs[0][r]);
            }
            *(bf16x4*)(h_out + (int64_t)pair * N + nb) = ov;
        }
    }
}

// Launch C: out[t, c .. c + 3] = sum_j part[t*k + j, c .. c + 3], ascending j.
__global__ void __launch_bounds__(256) moe_decode_combine_kernel(
    const float* __restrict__ part, __bf16* __restrict__ out, int T, int H, int k) {
    const int hv = H >> 2;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T * hv) return;
    const int t = i / hv;
    const int c = (i - t * hv) * 4;
    f32x4 s = *(const f32x4*)(part + (int64_t)t * k * H + c);
    for (int j = 1; j < k; ++j) s += *(const f32x4*)(part + ((int64_t)t * k + j) * H + c);
    bf16x4 ov;
#pragma unroll
    for (int r = 0; r < 4; ++r) ov[r] = (__bf16)s[r];
    *(bf16x4*)(out + (int64_t)t * H + c) = ov;
}

// The occupancy rule of the header.
static int md_waves(int T, int E, int k, int N) {
    const int live = E < T * k ? E : T * k;
    const int slabs = (N + 15) / 16;
    for (int W = 4; W > 1; W >>= 1)
        if ((slabs + W - 1) / W * live >= 256) return W;
    return 1;
}

template <int MB, int W>
static void md_launch_mode(hipStream_t s, int mode, dim3 grid, const __bf16* src, int row_div,
                           const int32_t* selected, const __bf16* gates, const __bf16* w, const __bf16* bias,
                           __bf16* h_out, float* part_out, int n_pairs, int N, int K, int act) {
#define MD_GO(MODE)                                                                                     \
    hipLaunchKernelGGL((moe_decode_kernel<MB, W, MODE>), grid, dim3(W * 64), 0, s, src, row_div, selected, \
                       gates, w, bias, h_out, part_out, n_pairs, N, K, act)
    if (mode == MD_FC) MD_GO(MD_FC);
    else if (mode == MD_FC_GLU) MD_GO(MD_FC_GLU);
    else MD_GO(MD_PROJ);
#undef MD_GO
}

template <int MB>
static void md_launch_waves(int W, hipStream_t s, int mode, dim3 grid, const __bf16* src, int row_div,
                            const int32_t* selected, const __bf16* gates, const __bf16* w, const __bf16* bias,
                            __bf16* h_out, float* part_out, int n_pairs, int N, int K, int act) {
    if (W == 4) md_launch_mode<MB, 4>(s, mode, grid, src, row_div, selected, gates, w, bias, h_out, part_out, n_pairs, N, K, act);
    else if (W == 2) md_launch_mode<MB, 2>(s, mode, grid, src, row_div, selected, gates, w, bias, h_out, part_out, n_pairs, N, K, act);
    else md_launch_mode<MB, 1>(s, mode, grid, src, row_div, selected, gates, w, bias, h_out, part_out, n_pairs, N, K, act);
}

// One of launches A / B: N output channels per pair, contraction K.
static void md_launch(hipStream_t s, int mode, int waves, int T, int E, int k, const __bf16* src, int row_div,
                      const int32_t* selected, const __bf16* gates, const __bf16* w, const __bf16* bias,
                      __bf16* h_out, float* part_out, int N, int K, int act) {
    const int W = waves > 0 ? waves : md_waves(T, E, k, N);
    const int slabs = (N + 15) / 16;
    const dim3 grid((unsigned)((slabs + W - 1) / W), (unsigned)E);
    const int n_pairs = T * k;
    if (T <= 16) md_launch_waves<1>(W, s, mode, grid, src, row_div, selected, gates, w, bias, h_out, part_out, n_pairs, N, K, act);
    else if (T <= 32) md_launch_waves<2>(W, s, mode, grid, src, row_div, selected, gates, w, bias, h_out, part_out, n_pairs, N, K, act);
    else md_launch_waves<4>(W, s, mode, grid, src, row_div, selected, gates, w, bias, h_out, part_out, n_pairs, N, K, act);
}

extern "C" int dolomite_moe_decode_mlp(dolomite_stream_t stream, const void* x, const int32_t* selected,
                                       const void* gates, const void* w_fc, const void* b_fc,
                                       const void* w_proj, const void* b_proj, void* h, float* part,
                                       void* out, int T, int E, int top_k, int H, int I, int act, int glu,
                                       int waves, int dtype) {
    if (dtype != DOLOMITE_BF16) return 9010;
    if (T < 1 || T > MD_MAX_T) return 9080;
    if (E < 1 || E > MD_MAX_E || top_k < 1 || top_k > MD_MAX_K || top_k > E) return 9081;
    if (H < 8 || I < 8 || H % 8 != 0 || I % 8 != 0 || H > (1 << 24) || I > (1 << 24)) return 9082;
    if (act < DOLOMITE_ACT_SILU || act > DOLOMITE_ACT_RELU) return 9083;
    if (waves != 0 && waves != 1 && waves != 2 && waves != 4) return 9084;
    if (!x || !selected || !gates || !w_fc || !w_proj || !h || !part || !out) return 9085;
    if (((uintptr_t)x & 15) || ((uintptr_t)w_fc & 15) || ((uintptr_t)w_proj & 15) || ((uintptr_t)h & 15) ||
        ((uintptr_t)part & 15) || ((uintptr_t)out & 7) || ((uintptr_t)b_fc & 1) || ((uintptr_t)b_proj & 1))
        return 9086;

    hipStream_t s = (hipStream_t)stream;
    md_launch(s, glu ? MD_FC_GLU : MD_FC, waves, T, E, top_k, (const __bf16*)x, top_k, selected,
              (const __bf16*)gates, (const __bf16*)w_fc, (const __bf16*)b_fc, (__bf16*)h, nullptr, I, H, act);
    if (int err = dol_last_error()) return err;
    md_launch(s, MD_PROJ, waves, T, E, top_k, (const __bf16*)h, 1, selected, (const __bf16*)gates,
              (const __bf16*)w_proj, (const __bf16*)b_proj, nullptr, part, H, I, act);
    if (int err = dol_last_error()) return err;
    const int nvec = T * (H / 4);
    hipLaunchKernelGGL(moe_decode_combine_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, s,
                       (const float*)part, (__bf16*)out, T, H, top_k);
    return dol_last_error();
}
