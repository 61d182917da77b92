// dolomite_hip — KV cache append and single-token decode attention for
// gfx950 (MI355X).
//
// The decode half of generation (the reference's dense flash path with a
// cache, attention/flash.py query_length == 1 branch): ONE query token per
// sequence attends over that sequence's cached keys. One query row per head
// makes the step HBM-bound on the K/V read, the opposite regime of
// attention.hip, so it has its own kernels here; the fragment types, the
// guarded load and the 4-lane reductions come from mfma_tiles.h.
//
// Design:
//   - grid (nsplit, batch, Hkv * head groups): split c of sequence b owns
//     keys [c*chunk, min((c+1)*chunk, cache_len[b])); the 4 waves of the
//     workgroup take its 64-key tiles round-robin and join through LDS.
//   - the G query heads of a kv head share ONE pass over its K/V: the
//     forward kernel's orientation with the group's heads in place of 16
//     consecutive query rows. S^T = K*Q^T with v_mfma_f32_16x16x32_bf16: a K
//     row segment of 8 bf16 is one lane's A fragment, loaded straight from
//     global memory (no LDS round trip: K is streamed once and shared with
//     no other wave); Q^T sits in registers as B; a lane owns one head.
//     G < 16 pads with zero heads whose results are discarded, 16 < G <= 32
//     is two head blocks on the same K/V fragments, G > 32 adds head groups
//     to grid.z.
//   - online softmax in fp32 with the scale folded into the exponent; P
//     packs to bf16 in registers as the B operand of O^T = V^T*P^T, whose A
//     operand is a ds_read_b64_tr_b16 of the wave's PRIVATE row-major V
//     image (no workgroup barrier in the key loop).
//   - keys at and beyond cache_len[b] are SELECTED out (scores to -inf, V
//     rows to zero), never multiplied by zero: the cache is uninitialised
//     memory and may hold NaN / Inf there.
//   - nsplit == 1 stores o directly; otherwise every workgroup stores fp32
//     partials (unnormalised O, row max, row sum) exclusively into caller
//     scratch and a second kernel combines the splits in ascending split
//     order. No atomics, no in-launch hand-off: bitwise reproducible.
//
// Fragment layouts: see attention.hip (verified by dolomite_mfma_probe and
// dolomite_tr16_probe).

#include "mfma_tiles.h"

#define DEC_LOG2E 1.44269504088896340736f

#define DEC_WAVES 4      // waves per workgroup
#define DEC_KTILE 64     // keys per wave step

// One V^T A-fragment: two transpose reads of the row-major image in the
// permuted key order of attention.hip "Swapped-operand score tiles". The
// reads and their wait live in one asm block (see attention.hip): the step is
// HBM-bound, so there is no lookahead and no use for the counted ladder of
// mfma_tiles.h (moving the reads onto it changed every instantiation's code).
template <int OFF>
__device__ __forceinline__ bf16x8 dec_tr16_frag(unsigned a0, unsigned a1) {
    bf16x4 lo, hi;
    asm volatile(
        "ds_read_b64_tr_b16 %0, %2 offset:%c4\n\t"
        "ds_read_b64_tr_b16 %1, %3 offset:%c4\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(lo), "=&v"(hi)
        : "v"(a0), "v"(a1), "i"(OFF)
        : "memory");
    bf16x8 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) { out[t] = lo[t]; out[4 + t] = hi[t]; }
    return out;
}

// Per-wave LDS region: the V image [64 key][DPAD+16] bf16 during the key
// loop, then the wave's join record (fp32 O^T fragments, m, l). The image is
// the larger of the two for every (DPAD, HB) instantiated.
template <int DPAD, int HB>
struct DecLds {
    static constexpr int S = DPAD + 16;
    static constexpr size_t image_bytes = (size_t)DEC_KTILE * S * sizeof(__bf16);
    static constexpr size_t join_bytes = (size_t)(HB * (DPAD / 16) * 4 + 2 * HB) * 64 * sizeof(float);
    static constexpr size_t wave_bytes = image_bytes > join_bytes ? image_bytes : join_bytes;
    static constexpr size_t bytes = DEC_WAVES * wave_bytes;
};

// ===========================================================================
// Decode attention
// ===========================================================================

template <int DPAD, int HB>
__global__ void __launch_bounds__(DEC_WAVES * 64, 2) fa_decode_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ kc, const __bf16* __restrict__ vc,
    __bf16* __restrict__ o, float* __restrict__ part_o, float* __restrict__ part_m,
    float* __restrict__ part_l, const int32_t* __restrict__ cache_len,
    int H, int D, int G, int nhg, int max_len, int chunk,
    int64_t q_ts, int64_t q_gs, int64_t k_bs, int64_t k_ts, int64_t k_hs,
    int64_t v_bs, int64_t v_ts, int64_t v_hs, float scale) {
    constexpr int KCH = DPAD / 32;   // contraction chunks of K*Q^T
    constexpr int DCH = DPAD / 16;   // output row blocks of O^T
    constexpr int SV = DecLds<DPAD, HB>::S;
    constexpr int HEADS = 16 * HB;   // q heads per workgroup

    const int split = blockIdx.x, b = blockIdx.y;
    const int kvh = blockIdx.z / nhg;
    const int g0 = (blockIdx.z % nhg) * HEADS;   // first head of the group handled here
    const int nsplit = gridDim.x;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15;
    const int lg = lane >> 4;

    // wave-uniform key range of this workgroup; cache_len is clamped into
    // [0, max_len] so a bad length can never address past the cache
    int len = __builtin_amdgcn_readfirstlane(cache_len[b]);
    len = min(max(len, 0), max_len);
    const int k0 = min(split * chunk, len);
    const int kend = min(k0 + chunk, len);
    const int ntiles = (kend - k0 + DEC_KTILE - 1) / DEC_KTILE;

    extern __shared__ char smem_raw[];
    char* wave_mem = smem_raw + (size_t)wave * DecLds<DPAD, HB>::wave_bytes;
    __bf16* Vlds = (__bf16*)wave_mem;

    // --- Q^T fragments (B layout: j = lr -> head, k = lg*8+e -> head dim);
    // heads >= G and pad dims are zero ---
    const __bf16* qrow = q + (int64_t)b * q_ts + (int64_t)kvh * q_gs;
    bf16x8 qf[HB][KCH];
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
        const int g = g0 + hb * 16 + lr;
        const bool hvalid = g < G;
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            const int d0 = c * 32 + lg * 8;
            qf[hb][c] = load_bf16x8_guard(qrow + (int64_t)(hvalid ? g : 0) * D + d0, d0, D, hvalid);
        }
    }

    float m_run[HB], l_run[HB];
    f32x4 o_acc[HB][DCH];           // O^T: d = dc*16 + lg*4 + x, head = lr
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
        m_run[hb] = -INFINITY;
        l_run[hb] = 0.f;
#pragma unroll
        for (int dc = 0; dc < DCH; ++dc) o_acc[hb][dc] = {0.f, 0.f, 0.f, 0.f};
    }

    // lane base addresses of the permuted-key tr16 reads (natural-row image)
    unsigned aV0, aV1;
    {
        const int row = lg * 4 + ((lane >> 2) & 3);
        const int cc = (lane & 3) * 4;
        aV0 = (unsigned)(size_t)(Vlds + row * SV + cc);
        aV1 = (unsigned)(size_t)(Vlds + (16 + row) * SV + cc);
    }

    const float scale2 = scale * DEC_LOG2E;
    const __bf16* kbase = kc + (int64_t)b * k_bs + (int64_t)kvh * k_hs;
    const __bf16* vbase = vc + (int64_t)b * v_bs + (int64_t)kvh * v_hs;

    constexpr int VPIECES = DEC_KTILE * DPAD / 8 / 64;  // 16B V pieces per lane and tile

    for (int t = wave; t < ntiles; t += DEC_WAVES) {
        const int ks = k0 + t * DEC_KTILE;

        // --- issue the whole tile's loads up front: K fragments straight to
        // registers (A layout: i = lr -> key, k = lg*8+e -> head dim), V
        // pieces for the LDS image. Keys >= kend read the row kend-1 (always
        // inside the cache) and are selected out below. ---
        bf16x8 kf[4][KCH];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int key = min(ks + cb * 16 + lr, kend - 1);
            const __bf16* kp = kbase + (int64_t)key * k_ts;
#pragma unroll
            for (int c = 0; c < KCH; ++c) {
                const int d0 = c * 32 + lg * 8;
                kf[cb][c] = load_bf16x8_guard(kp + d0, d0, D, true);
            }
        }
        bf16x8 vp[VPIECES];
#pragma unroll
        for (int j = 0; j < VPIECES; ++j) {
            const int pidx = lane + j * 64;
            const int key = pidx / (DPAD / 8);
            const int d0 = (pidx % (DPAD / 8)) * 8;
            const bool kvalid = ks + key < kend;
            const __bf16* p = vbase + (int64_t)min(ks + key, kend - 1) * v_ts + d0;
            vp[j] = load_bf16x8_guard(p, d0, D, kvalid);
        }

        // --- S^T = K*Q^T: sc[hb][cb][x] is (head g0+16hb+lr,
        // key ks + 16cb + 4lg + x) ---
        f32x4 sc[HB][4];
#pragma unroll
        for (int hb = 0; hb < HB; ++hb)
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                sc[hb][cb] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < KCH; ++c) sc[hb][cb] = MFMA16(kf[cb][c], qf[hb][c], sc[hb][cb]);
            }

        // V image: the previous tile's transpose reads were waited on inside
        // their asm blocks and LDS serves one wave's accesses in order, so
        // the wave-private image needs no barrier
#pragma unroll
        for (int j = 0; j < VPIECES; ++j) {
            const int pidx = lane + j * 64;
            const int key = pidx / (DPAD / 8);
            const int d0 = (pidx % (DPAD / 8)) * 8;
            *(bf16x8*)&Vlds[key * SV + d0] = vp[j];
        }

        // --- key-range select + online softmax (fp32), one head per lane ---
        bf16x8 pf[HB][2];
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            float mx = -INFINITY;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const int kpos = ks + cb * 16 + lg * 4 + x;
                    sc[hb][cb][x] = (kpos < kend) ? sc[hb][cb][x] : -INFINITY;
                    mx = fmaxf(mx, sc[hb][cb][x]);
                }
            const float rowmax = qgroup_reduce_max(mx);
            // every tile holds at least one key < kend, so mnew is finite
            // unless a score itself is -inf; the guard covers that
            float mnew = fmaxf(m_run[hb], rowmax * scale2);
            if (mnew == -INFINITY) mnew = 0.f;
            const float alpha = exp2f(m_run[hb] - mnew);
            m_run[hb] = mnew;
            float rsum = 0.f;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const float e = exp2f(fmaf(sc[hb][cb][x], scale2, -mnew));
                    pf[hb][cb >> 1][(cb & 1) * 4 + x] = (__bf16)e;
                    rsum += e;
                }
            l_run[hb] = l_run[hb] * alpha + rsum;
#pragma unroll
            for (int dc = 0; dc < DCH; ++dc) o_acc[hb][dc] *= alpha;
        }

        // --- O^T += V^T*P^T: one V fragment serves every head block ---
#define DEC_PV_STEP(i)                                                                   \
    if constexpr ((i) < 2 * DCH) {                                                       \
        constexpr int c2_ = (i) / DCH, dc_ = (i) % DCH;                                  \
        const bf16x8 vf_ = dec_tr16_frag<(c2_ * 32 * SV + dc_ * 16) * 2>(aV0, aV1);      \
        _Pragma("unroll") for (int hb = 0; hb < HB; ++hb)                                \
            o_acc[hb][dc_] = MFMA16(vf_, pf[hb][c2_], o_acc[hb][dc_]);                   \
    }
        DEC_PV_STEP(0) DEC_PV_STEP(1) DEC_PV_STEP(2) DEC_PV_STEP(3)
        DEC_PV_STEP(4) DEC_PV_STEP(5) DEC_PV_STEP(6) DEC_PV_STEP(7)
        DEC_PV_STEP(8) DEC_PV_STEP(9) DEC_PV_STEP(10) DEC_PV_STEP(11)
        DEC_PV_STEP(12) DEC_PV_STEP(13) DEC_PV_STEP(14) DEC_PV_STEP(15)
#undef DEC_PV_STEP
    }

    // --- join the workgroup's waves through LDS, in ascending wave order.
    // Record layout per wave: [HB*DCH*4 + 2*HB][64 lanes] fp32. ---
    float* rec = (float*)wave_mem;
    constexpr int REC_M = HB * DCH * 4;
#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
        const float l_head = qgroup_reduce_sum(l_run[hb]);
#pragma unroll
        for (int dc = 0; dc < DCH; ++dc)
#pragma unroll
            for (int x = 0; x < 4; ++x) rec[((hb * DCH + dc) * 4 + x) * 64 + lane] = o_acc[hb][dc][x];
        rec[(REC_M + hb) * 64 + lane] = m_run[hb];
        rec[(REC_M + HB + hb) * 64 + lane] = l_head;
    }
    __syncthreads();
    if (wave != 0) return;

#pragma unroll
    for (int hb = 0; hb < HB; ++hb) {
        float mw[DEC_WAVES];
        float m = -INFINITY;
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) {
            const float* rw = (const float*)(smem_raw + (size_t)w * DecLds<DPAD, HB>::wave_bytes);
            mw[w] = rw[(REC_M + hb) * 64 + lane];
            m = fmaxf(m, mw[w]);
        }
        const float mref = (m == -INFINITY) ? 0.f : m;   // no keys at all: weights are exp2(-inf) = 0
        float l = 0.f;
        f32x4 acc[DCH];
#pragma unroll
        for (int dc = 0; dc < DCH; ++dc) acc[dc] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < DEC_WAVES; ++w) {
            const float* rw = (const float*)(smem_raw + (size_t)w * DecLds<DPAD, HB>::wave_bytes);
            const float wgt = exp2f(mw[w] - mref);
            l += wgt * rw[(REC_M + HB + hb) * 64 + lane];
#pragma unroll
            for (int dc = 0; dc < DCH; ++dc)
#pragma unroll
                for (int x = 0; x < 4; ++x) acc[dc][x] += wgt * rw[((hb * DCH + dc) * 4 + x) * 64 + lane];
        }

        const int g = g0 + hb * 16 + lr;
        if (g >= G) continue;
        const int h = kvh * G + g;
        if (nsplit == 1) {
            // l == 0 only without keys: acc is +0 and the row is +0
            const float inv_l = (l > 0.f) ? 1.f / l : 0.f;
            __bf16* orow = o + ((int64_t)b * H + h) * D;
#pragma unroll
            for (int dc = 0; dc < DCH; ++dc) {
                const int d0 = dc * 16 + lg * 4;
                bf16x4 ov;
#pragma unroll
                for (int x = 0; x < 4; ++x) ov[x] = (__bf16)(acc[dc][x] * inv_l);
                if (d0 < D) *(bf16x4*)&orow[d0] = ov;
            }
        } else {
            const int64_t slot = ((int64_t)b * H + h) * nsplit + split;
            float* prow = part_o + slot * D;
#pragma unroll
            for (int dc = 0; dc < DCH; ++dc) {
                const int d0 = dc * 16 + lg * 4;
                if (d0 < D) *(f32x4*)&prow[d0] = acc[dc];
            }
            if (lg == 0) {
                part_m[slot] = m;
                part_l[slot] = l;
            }
        }
    }
}

// Combine the splits of one (sequence, head) in ascending split order.
// One workgroup of 32 lanes-worth of work per row: thread t owns dims
// [4t, 4t+4).
__global__ void __launch_bounds__(64) fa_decode_combine_kernel(
    const float* __restrict__ part_o, const float* __restrict__ part_m,
    const float* __restrict__ part_l, __bf16* __restrict__ o, int D, int nsplit) {
    const int64_t row = blockIdx.x;          // b*H + h
    const int d0 = threadIdx.x * 4;
    if (d0 >= D) return;
    const float* pm = part_m + row * nsplit;
    const float* pl = part_l + row * nsplit;
    float m = -INFINITY;
    for (int c = 0; c < nsplit; ++c) m = fmaxf(m, pm[c]);
    const float mref = (m == -INFINITY) ? 0.f : m;
    float l = 0.f;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nsplit; ++c) {
        const float wgt = exp2f(pm[c] - mref);
        l += wgt * pl[c];
        const f32x4 po = *(const f32x4*)&part_o[(row * nsplit + c) * D + d0];
#pragma unroll
        for (int x = 0; x < 4; ++x) acc[x] += wgt * po[x];
    }
    const float inv_l = (l > 0.f) ? 1.f / l : 0.f;
    bf16x4 ov;
#pragma unroll
    for (int x = 0; x < 4; ++x) ov[x] = (__bf16)(acc[x] * inv_l);
    *(bf16x4*)&o[row * D + d0] = ov;
}

extern "C" int64_t dolomite_fa_decode_scratch_floats(int batch, int H, int D, int nsplit) {
    if (batch < 0 || H < 0 || D < 0 || nsplit < 1) return -1;
    if (nsplit == 1) return 0;
    return (int64_t)batch * H * nsplit * (D + 2);
}

template <int DPAD, int HB>
static int launch_fa_decode(hipStream_t s, const __bf16* q, const __bf16* kc, const __bf16* vc, __bf16* o,
                            float* scratch, const int32_t* cache_len, int batch, int H, int Hkv, int D, int G,
                            int max_len, int nsplit, int chunk,
                            int64_t q_ts, int64_t q_gs, int64_t k_bs, int64_t k_ts, int64_t k_hs,
                            int64_t v_bs, int64_t v_ts, int64_t v_hs, float scale) {
    const int nhg = (G + 16 * HB - 1) / (16 * HB);
    const int64_t nslots = (int64_t)batch * H * nsplit;
    float* part_o = scratch;
    float* part_m = scratch ? scratch + nslots * D : nullptr;
    float* part_l = scratch ? part_m + nslots : nullptr;
    constexpr size_t lds = DecLds<DPAD, HB>::bytes;
    if (lds > 48 * 1024) {  // beyond the default dynamic-LDS limit: opt in (a cheap host-side call)
        hipError_t e = hipFuncSetAttribute((const void*)fa_decode_kernel<DPAD, HB>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    dim3 grid(nsplit, batch, Hkv * nhg), block(DEC_WAVES * 64);
    hipLaunchKernelGGL((fa_decode_kernel<DPAD, HB>), grid, block, lds, s,
                       q, kc, vc, o, part_o, part_m, part_l, cache_len, H, D, G, nhg, max_len, chunk,
                       q_ts, q_gs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs, scale);
    int rc = dol_last_error();
    if (rc != 0 || nsplit == 1) return rc;
    hipLaunchKernelGGL(fa_decode_combine_kernel, dim3((unsigned)(batch * H)), dim3(64), 0, s,
                       part_o, part_m, part_l, o, D, nsplit);
    return dol_last_error();
}

extern "C" int dolomite_fa_decode(dolomite_stream_t stream,
                                  const void* q, const void* k_cache, const void* v_cache, void* o,
                                  float* scratch, const int32_t* cache_len,
                                  int batch, int H, int Hkv, int D, int G,
                                  int max_len, int nsplit,
                                  int64_t q_tstride, int64_t q_gstride,
                                  int64_t k_bstride, int64_t k_tstride, int64_t k_hstride,
                                  int64_t v_bstride, int64_t v_tstride, int64_t v_hstride,
                                  float scale, int dtype) {
    if (dtype != DOLOMITE_BF16) return 9010;
    if (D > 128) return 9011;
    if (!(scale > 0.f)) return 9015;
    if (D <= 0 || D % 8 != 0) return 9031;
    if (batch < 0 || H <= 0 || Hkv <= 0 || G <= 0 || max_len < 0 || H != Hkv * G) return 9032;
    if (nsplit < 1 || nsplit > 65535 || batch > 65535) return 9033;
    if (nsplit > 1 && scratch == nullptr) return 9034;
    if (batch == 0) return 0;
    const int HBn = G > 16 ? 2 : 1;
    const int64_t gz = (int64_t)Hkv * ((G + 16 * HBn - 1) / (16 * HBn));
    if (gz > 65535 || (int64_t)batch * H > 0x7fffffff) return 9033;
    // keys per split: ceil(max_len / nsplit) rounded up to the key tile
    int chunk = (max_len + nsplit - 1) / nsplit;
    chunk = (chunk + DEC_KTILE - 1) / DEC_KTILE * DEC_KTILE;
    if (chunk == 0) chunk = DEC_KTILE;
    hipStream_t s = (hipStream_t)stream;
#define CASE(DP, HBV)                                                                                  \
    return launch_fa_decode<DP, HBV>(s, (const __bf16*)q, (const __bf16*)k_cache, (const __bf16*)v_cache, \
                                     (__bf16*)o, scratch, cache_len, batch, H, Hkv, D, G, max_len, nsplit, \
                                     chunk, q_tstride, q_gstride, k_bstride, k_tstride, k_hstride,     \
                                     v_bstride, v_tstride, v_hstride, scale)
    if (HBn == 1) {
        if (D <= 64) CASE(64, 1);
        if (D <= 96) CASE(96, 1);
        CASE(128, 1);
    }
    if (D <= 64) CASE(64, 2);
    if (D <= 96) CASE(96, 2);
    CASE(128, 2);
#undef CASE
}

// ===========================================================================
// KV cache append: K and V slots of packed qkv rows -> cache positions
// ===========================================================================

#define APP_ROWS 8   // qkv rows per workgroup

__global__ void __launch_bounds__(256) kv_cache_append_kernel(
    const uint16_t* __restrict__ qkv, const int32_t* __restrict__ src_begin,
    const int32_t* __restrict__ src_end, const int32_t* __restrict__ dst_pos,
    uint16_t* __restrict__ k_cache, uint16_t* __restrict__ v_cache,
    int Hkv, int D, int S_cap, int64_t row_ts, int64_t k_off, int64_t v_off, int64_t kv_hs,
    int64_t c_bs, int64_t c_ts, int64_t c_hs) {
    const int b = blockIdx.y;
    const int s0 = src_begin[b];
    const int n = src_end[b] - s0;
    const int p0 = dst_pos[b];
    const int r0 = blockIdx.x * APP_ROWS;
    if (r0 >= n) return;
    const int dp = D / 8;                 // 16B pieces per head
    const int per_row = 2 * Hkv * dp;     // K pieces then V pieces
    const int total = APP_ROWS * per_row;
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int i = r0 + idx / per_row;
        int rem = idx % per_row;
        const int is_v = rem >= Hkv * dp;
        if (is_v) rem -= Hkv * dp;
        const int j = rem / dp;
        const int d0 = (rem % dp) * 8;
        const int pos = p0 + i;
        if (i >= n || pos < 0 || pos >= S_cap) continue;   // beyond the cache: skipped, never written
        const uint16_t* src = qkv + (int64_t)(s0 + i) * row_ts + (is_v ? v_off : k_off) + (int64_t)j * kv_hs + d0;
        uint16_t* dst = (is_v ? v_cache : k_cache) + (int64_t)b * c_bs + (int64_t)pos * c_ts + (int64_t)j * c_hs + d0;
        *(us8_t*)dst = *(const us8_t*)src;
    }
}

extern "C" int dolomite_kv_cache_append(dolomite_stream_t stream, const void* qkv,
                                        const int32_t* src_begin, const int32_t* src_end,
                                        const int32_t* dst_pos, void* k_cache, void* v_cache,
                                        int batch, int max_rows, int Hkv, int D, int S_cap,
                                        int64_t row_tstride, int64_t k_off, int64_t v_off, int64_t kv_hstride,
                                        int64_t cache_bstride, int64_t cache_tstride, int64_t cache_hstride,
                                        int dtype) {
    if (dtype != DOLOMITE_BF16) return 9010;
    if (batch < 0 || max_rows < 0 || Hkv <= 0 || S_cap < 0 || batch > 65535) return 9030;
    // 16-byte pieces: head dim and every stride / offset in units of 8 elements
    if (D <= 0 || D % 8 != 0) return 9031;
    if ((row_tstride | k_off | v_off | kv_hstride | cache_bstride | cache_tstride | cache_hstride) % 8 != 0)
        return 9031;
    if (batch == 0 || max_rows == 0) return 0;
    dim3 grid((max_rows + APP_ROWS - 1) / APP_ROWS, batch), block(256);
    hipLaunchKernelGGL(kv_cache_append_kernel, grid, block, 0, (hipStream_t)stream,
                       (const uint16_t*)qkv, src_begin, src_end, dst_pos, (uint16_t*)k_cache, (uint16_t*)v_cache,
                       Hkv, D, S_cap, row_tstride, k_off, v_off, kv_hstride,
                       cache_bstride, cache_tstride, cache_hstride);
    return dol_last_error();
}
