// dolomite_hip — fp8 (OCP e4m3) KV cache for gfx950 (MI355X): the quantising
// append and the single-token decode attention that reads it.
//
// Storage (include/dolomite_hip.h): k_cache / v_cache hold e4m3 bytes,
// k_scale / v_scale one fp32 per (sequence, kv head, position), position-
// contiguous. One (position, kv head) slice x of D bf16 values is stored as
//   a = max(amax|x|, 2^-64), scale = a / 448, q = e4m3_rne(x * (448 / a))
// in fp32, so q * scale restores x to e4m3's 3 mantissa bits. A decode step
// reads half the bytes of the bf16 cache.
//
// Append: a group of D/8 lanes owns one (row, kv head, K|V) slice. Each lane
// loads 16 bytes (8 bf16), the amax is reduced inside the group with DPP
// (quad_perm, row_half_mirror, row_mirror: groups sit in slots of 1/2/4/8/16
// lanes, the lanes behind D/8 contribute 0), each lane converts with
// v_cvt_pk_fp8_f32 and stores 8 bytes, the group's first lane stores the
// scale. max is order-free: deterministic.
//
// Decode: decode.hip's kernel (grid, key split, 4-wave round-robin, LDS join,
// partials, combine — see there) with another movement of the bytes:
//   - a lane's K fragment is 8 e4m3 bytes of one key, ONE 8-byte global load,
//     converted to bf16x8 in registers (exact: every finite e4m3 value is a
//     bf16 value) for the same v_mfma_f32_16x16x32_bf16;
//   - the K scale never touches the operand: it multiplies the fp32 score.
//     Lane l loads the scales of key ks + l (clamped to the last valid key)
//     with one coalesced load per tile and array, parks them in 512 bytes of
//     wave-private LDS and reads back the four runs of 4 floats that belong
//     to its score registers (keys ks + 16cb + 4lg + x) as ds_read_b128;
//   - V pieces are 8 bytes = 8 head dims (a 16-byte piece would straddle rows
//     at D = 40 / 72), converted to bf16 before the store into the same
//     row-major image, read by the same ds_read_b64_tr_b16;
//   - the V scale is folded into P: the bf16 B operand holds e * v_scale[key],
//     l sums the unscaled e;
//   - keys at and behind cache_len[b] hold arbitrary bytes (0x7f is a NaN) and
//     arbitrary scales: no load goes there (rows and scale indices clamp to
//     the last valid key), scores are selected to -inf after the scale
//     multiply, P entries to +0, V rows to zero.

#include "mfma_tiles.h"

#define D8_LOG2E 1.44269504088896340736f
#define D8_WAVES 4      // waves per workgroup
#define D8_KTILE 64     // keys per wave step

// load_bf16x8_guard for 8 e4m3 bytes: one 8-byte load from an address clamped
// into the row, zero bytes (+0) in the pad or for an invalid row.
__device__ __forceinline__ u32x2 load_e4m3x8_guard(const uint8_t* p, int d0, int D, bool valid) {
    const uint8_t* q = (d0 < D) ? p : (p - d0);
    const bool ok = valid && (d0 < D);
    u32x2 r = *(const u32x2*)q;
    r[0] = ok ? r[0] : 0u;
    r[1] = ok ? r[1] : 0u;
    return r;
}

// Per-wave LDS region: decode.hip's (V image, then the join record) plus the
// tile's 64 K scales and 64 V scales behind it.
template <int DPAD, int HB>
struct Dec8Lds {
    static constexpr int S = DPAD + 16;
    static constexpr size_t image_bytes = (size_t)D8_KTILE * S * sizeof(__bf16);
    static constexpr size_t join_bytes = (size_t)(HB * (DPAD / 16) * 4 + 2 * HB) * 64 * sizeof(float);
    static constexpr size_t scale_off = image_bytes > join_bytes ? image_bytes : join_bytes;  // multiple of 16
    static constexpr size_t wave_bytes = scale_off + 2 * D8_KTILE * sizeof(float);
    static constexpr size_t bytes = D8_WAVES * wave_bytes;
};

// ===========================================================================
// Decode attention over the e4m3 cache
// ===========================================================================

template <int DPAD, int HB>
__global__ void __launch_bounds__(D8_WAVES * 64, 2) fa_decode_fp8_kernel(
    const __bf16* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    __bf16* __restrict__ o, float* __restrict__ part_o, float* __restrict__ part_m,
    float* __restrict__ part_l, const int32_t* __restrict__ cache_len,
    int H, int D, int G, int nhg, int max_len, int chunk,
    int64_t q_ts, int64_t q_gs, int64_t k_bs, int64_t k_ts, int64_t k_hs,
    int64_t v_bs, int64_t v_ts, int64_t v_hs, int64_t s_bs, int64_t s_hs, float scale) {
    constexpr int KCH = DPAD / 32;   // contraction chunks of K*Q^T
    constexpr int DCH = DPAD / 16;   // output row blocks of O^T
    constexpr int SV = Dec8Lds<DPAD, HB>::S;
    constexpr int HEADS = 16 * HB;   // q heads per workgroup

    const int split = blockIdx.x, b = blockIdx.y;
    const int kvh = blockIdx.z / nhg;
    const int g0 = (blockIdx.z % nhg) * HEADS;
    const int nsplit = gridDim.x;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15;
    const int lg = lane >> 4;

    // wave-uniform key range; cache_len clamped into [0, max_len]
    int len = __builtin_amdgcn_readfirstlane(cache_len[b]);
    len = min(max(len, 0), max_len);
    const int k0 = min(split * chunk, len);
    const int kend = min(k0 + chunk, len);
    const int ntiles = (kend - k0 + D8_KTILE - 1) / D8_KTILE;

    extern __shared__ char smem_raw[];
    char* wave_mem = smem_raw + (size_t)wave * Dec8Lds<DPAD, HB>::wave_bytes;
    __bf16* Vlds = (__bf16*)wave_mem;
    float* Slds = (float*)(wave_mem + Dec8Lds<DPAD, HB>::scale_off);   // [64] K scales, [64] V scales

    // --- Q^T fragments (B layout: j = lr -> head, k = lg*8+e -> head dim) ---
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

    unsigned aV0, aV1;
    fa_tr16_perm_bases(Vlds, SV, lane, aV0, aV1);

    const float scale2 = scale * D8_LOG2E;
    const uint8_t* kbase = kc + (int64_t)b * k_bs + (int64_t)kvh * k_hs;
    const uint8_t* vbase = vc + (int64_t)b * v_bs + (int64_t)kvh * v_hs;
    const float* ksbase = k_scale + (int64_t)b * s_bs + (int64_t)kvh * s_hs;
    const float* vsbase = v_scale + (int64_t)b * s_bs + (int64_t)kvh * s_hs;

    constexpr int VPIECES = D8_KTILE * DPAD / 8 / 64;  // 8-byte V pieces per lane and tile

    for (int t = wave; t < ntiles; t += D8_WAVES) {
        const int ks = k0 + t * D8_KTILE;

        // --- the whole tile's loads up front. Keys >= kend read row / scale
        // kend-1 (inside the cache for any S_cap) and are selected out. ---
        u32x2 kf[4][KCH];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int key = min(ks + cb * 16 + lr, kend - 1);
            const uint8_t* kp = kbase + (int64_t)key * k_ts;
#pragma unroll
            for (int c = 0; c < KCH; ++c) {
                const int d0 = c * 32 + lg * 8;
                kf[cb][c] = load_e4m3x8_guard(kp + d0, d0, D, true);
            }
        }
        const int skey = min(ks + lane, kend - 1);
        const float ks_lane = ksbase[skey];
        const float vs_lane = vsbase[skey];
        u32x2 vp[VPIECES];
#pragma unroll
        for (int j = 0; j < VPIECES; ++j) {
            const int pidx = lane + j * 64;
            const int key = pidx / (DPAD / 8);
            const int d0 = (pidx % (DPAD / 8)) * 8;
            const bool kvalid = ks + key < kend;
            const uint8_t* p = vbase + (int64_t)min(ks + key, kend - 1) * v_ts + d0;
            vp[j] = load_e4m3x8_guard(p, d0, D, kvalid);
        }

        // --- S^T = K*Q^T on the unscaled e4m3 values: sc[hb][cb][x] is
        // (head g0+16hb+lr, key ks + 16cb + 4lg + x) ---
        f32x4 sc[HB][4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            bf16x8 ka[KCH];
#pragma unroll
            for (int c = 0; c < KCH; ++c) ka[c] = e4m3x8_to_bf16x8(kf[cb][c]);
#pragma unroll
            for (int hb = 0; hb < HB; ++hb) {
                sc[hb][cb] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < KCH; ++c) sc[hb][cb] = MFMA16(ka[c], qf[hb][c], sc[hb][cb]);
            }
        }

        // Scales and V image into the wave's own LDS. The previous tile's
        // reads of both were waited on (the tr16 asm blocks, the scale reads'
        // consumers) and LDS serves one wave's accesses in order: no barrier.
        Slds[lane] = ks_lane;
        Slds[64 + lane] = vs_lane;
#pragma unroll
        for (int j = 0; j < VPIECES; ++j) {
            const int pidx = lane + j * 64;
            const int key = pidx / (DPAD / 8);
            const int d0 = (pidx % (DPAD / 8)) * 8;
            *(bf16x8*)&Vlds[key * SV + d0] = e4m3x8_to_bf16x8(vp[j]);
        }
        f32x4 ksv[4], vsv[4];       // the scales of this lane's 16 keys
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            ksv[cb] = *(const f32x4*)&Slds[cb * 16 + lg * 4];
            vsv[cb] = *(const f32x4*)&Slds[64 + cb * 16 + lg * 4];
        }

        // --- K scale, key-range select, online softmax (fp32) ---
        bf16x8 pf[HB][2];
#pragma unroll
        for (int hb = 0; hb < HB; ++hb) {
            float mx = -INFINITY;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const int kpos = ks + cb * 16 + lg * 4 + x;
                    sc[hb][cb][x] = (kpos < kend) ? sc[hb][cb][x] * ksv[cb][x] : -INFINITY;
                    mx = fmaxf(mx, sc[hb][cb][x]);
                }
            const float rowmax = qgroup_reduce_max(mx);
            float mnew = fmaxf(m_run[hb], rowmax * scale2);
            if (mnew == -INFINITY) mnew = 0.f;
            const float alpha = exp2f(m_run[hb] - mnew);
            m_run[hb] = mnew;
            float rsum = 0.f;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const int kpos = ks + cb * 16 + lg * 4 + x;
                    const float e = exp2f(fmaf(sc[hb][cb][x], scale2, -mnew));
                    // V scale folded into P; a key behind kend is +0, not 0 * scale
                    pf[hb][cb >> 1][(cb & 1) * 4 + x] = (__bf16)((kpos < kend) ? e * vsv[cb][x] : 0.f);
                    rsum += e;
                }
            l_run[hb] = l_run[hb] * alpha + rsum;
#pragma unroll
            for (int dc = 0; dc < DCH; ++dc) o_acc[hb][dc] *= alpha;
        }

        // --- O^T += V^T*P^T: one V fragment serves every head block ---
#define D8_PV_STEP(i)                                                                    \
    if constexpr ((i) < 2 * DCH) {                                                       \
        constexpr int c2_ = (i) / DCH, dc_ = (i) % DCH;                                  \
        const bf16x8 vf_ = dec_tr16_frag<(c2_ * 32 * SV + dc_ * 16) * 2>(aV0, aV1);      \
        _Pragma("unroll") for (int hb = 0; hb < HB; ++hb)                                \
            o_acc[hb][dc_] = MFMA16(vf_, pf[hb][c2_], o_acc[hb][dc_]);                   \
    }
        D8_PV_STEP(0) D8_PV_STEP(1) D8_PV_STEP(2) D8_PV_STEP(3)
        D8_PV_STEP(4) D8_PV_STEP(5) D8_PV_STEP(6) D8_PV_STEP(7)
        D8_PV_STEP(8) D8_PV_STEP(9) D8_PV_STEP(10) D8_PV_STEP(11)
        D8_PV_STEP(12) D8_PV_STEP(13) D8_PV_STEP(14) D8_PV_STEP(15)
#undef D8_PV_STEP
    }

    // --- join the workgroup's waves through LDS, in ascending wave order
    // (decode.hip's record: [HB*DCH*4 + 2*HB][64 lanes] fp32 per wave) ---
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
        float mw[D8_WAVES];
        float m = -INFINITY;
#pragma unroll
        for (int w = 0; w < D8_WAVES; ++w) {
            const float* rw = (const float*)(smem_raw + (size_t)w * Dec8Lds<DPAD, HB>::wave_bytes);
            mw[w] = rw[(REC_M + hb) * 64 + lane];
            m = fmaxf(m, mw[w]);
        }
        const float mref = (m == -INFINITY) ? 0.f : m;   // no keys at all: weights are exp2(-inf) = 0
        float l = 0.f;
        f32x4 acc[DCH];
#pragma unroll
        for (int dc = 0; dc < DCH; ++dc) acc[dc] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < D8_WAVES; ++w) {
            const float* rw = (const float*)(smem_raw + (size_t)w * Dec8Lds<DPAD, HB>::wave_bytes);
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
            const float inv_l = (l > 0.f) ? 1.f / l : 0.f;   // l == 0 only without keys: the row is +0
            fa_store_rowT_bf16<DCH>(o + ((int64_t)b * H + h) * D, acc, inv_l, true, D, lg);
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

template <int DPAD, int HB>
static int launch_fa_decode_fp8(hipStream_t s, const __bf16* q, const uint8_t* kc, const uint8_t* vc,
                                const float* k_scale, const float* v_scale, __bf16* o,
                                float* scratch, const int32_t* cache_len, int batch, int H, int Hkv, int D, int G,
                                int max_len, int nsplit, int chunk,
                                int64_t q_ts, int64_t q_gs, int64_t k_bs, int64_t k_ts, int64_t k_hs,
                                int64_t v_bs, int64_t v_ts, int64_t v_hs, int64_t s_bs, int64_t s_hs, float scale) {
    const int nhg = (G + 16 * HB - 1) / (16 * HB);
    const int64_t nslots = (int64_t)batch * H * nsplit;
    float* part_o = scratch;
    float* part_m = scratch ? scratch + nslots * D : nullptr;
    float* part_l = scratch ? part_m + nslots : nullptr;
    constexpr size_t lds = Dec8Lds<DPAD, HB>::bytes;
    if (lds > 48 * 1024) {  // beyond the default dynamic-LDS limit: opt in
        hipError_t e = hipFuncSetAttribute((const void*)fa_decode_fp8_kernel<DPAD, HB>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    dim3 grid(nsplit, batch, Hkv * nhg), block(D8_WAVES * 64);
    hipLaunchKernelGGL((fa_decode_fp8_kernel<DPAD, HB>), grid, block, lds, s,
                       q, kc, vc, k_scale, v_scale, o, part_o, part_m, part_l, cache_len,
                       H, D, G, nhg, max_len, chunk,
                       q_ts, q_gs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs, s_bs, s_hs, scale);
    int rc = dol_last_error();
    if (rc != 0 || nsplit == 1) return rc;
    return dol_fa_decode_combine(s, part_o, part_m, part_l, o, (int64_t)batch * H, D, nsplit);
}

extern "C" int dolomite_fa_decode_fp8(dolomite_stream_t stream,
                                      const void* q, const void* k_cache, const void* v_cache,
                                      const float* k_scale, const float* v_scale, void* o,
                                      float* scratch, const int32_t* cache_len,
                                      int batch, int H, int Hkv, int D, int G,
                                      int max_len, int nsplit,
                                      int64_t q_tstride, int64_t q_gstride,
                                      int64_t k_bstride, int64_t k_tstride, int64_t k_hstride,
                                      int64_t v_bstride, int64_t v_tstride, int64_t v_hstride,
                                      int64_t s_bstride, int64_t s_hstride,
                                      float scale, int dtype) {
    if (dtype != DOLOMITE_BF16) return 9010;
    if (D > 128) return 9011;
    if (!(scale > 0.f)) return 9015;
    if (D <= 0 || D % 8 != 0) return 9031;
    // 8-byte cache loads: every cache stride in units of 8 elements
    if ((k_bstride | k_tstride | k_hstride | v_bstride | v_tstride | v_hstride) % 8 != 0) return 9031;
    if (batch < 0 || H <= 0 || Hkv <= 0 || G <= 0 || max_len < 0 || H != Hkv * G) return 9032;
    if (nsplit < 1 || nsplit > 65535 || batch > 65535) return 9033;
    if (nsplit > 1 && scratch == nullptr) return 9034;
    if (batch == 0) return 0;
    const int HBn = G > 16 ? 2 : 1;
    const int64_t gz = (int64_t)Hkv * ((G + 16 * HBn - 1) / (16 * HBn));
    if (gz > 65535 || (int64_t)batch * H > 0x7fffffff) return 9033;
    // keys per split: ceil(max_len / nsplit) rounded up to the key tile
    int chunk = (max_len + nsplit - 1) / nsplit;
    chunk = (chunk + D8_KTILE - 1) / D8_KTILE * D8_KTILE;
    if (chunk == 0) chunk = D8_KTILE;
    hipStream_t s = (hipStream_t)stream;
#define CASE(DP, HBV)                                                                                   \
    return launch_fa_decode_fp8<DP, HBV>(s, (const __bf16*)q, (const uint8_t*)k_cache,                  \
                                         (const uint8_t*)v_cache, k_scale, v_scale, (__bf16*)o, scratch, \
                                         cache_len, batch, H, Hkv, D, G, max_len, nsplit, chunk,        \
                                         q_tstride, q_gstride, k_bstride, k_tstride, k_hstride,         \
                                         v_bstride, v_tstride, v_hstride, s_bstride, s_hstride, scale)
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
// Quantising KV cache append
// ===========================================================================

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// GL: lane slots per slice, the power of two >= D/8 (1 .. 16), so a group
// never crosses a 16-lane DPP row. 256 / GL slices per workgroup.
template <int GL>
__global__ void __launch_bounds__(256) kv_cache_append_fp8_kernel(
    const uint16_t* __restrict__ qkv, const int32_t* __restrict__ src_begin,
    const int32_t* __restrict__ src_end, const int32_t* __restrict__ dst_pos,
    uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache,
    float* __restrict__ k_scale, float* __restrict__ v_scale,
    int max_rows, int Hkv, int D, int S_cap, int64_t row_ts, int64_t k_off, int64_t v_off, int64_t kv_hs,
    int64_t c_bs, int64_t c_ts, int64_t c_hs, int64_t s_bs, int64_t s_hs) {
    constexpr int SLICES = 256 / GL;
    const int b = blockIdx.y;
    const int s0 = src_begin[b];
    const int n = min(src_end[b] - s0, max_rows);
    const int p0 = dst_pos[b];
    const int per_row = 2 * Hkv;                       // K slices then V slices
    if ((int)(blockIdx.x * SLICES / per_row) >= n) return;   // workgroup-uniform
    const int slice = blockIdx.x * SLICES + threadIdx.x / GL;
    const int gl = threadIdx.x % GL;
    const int i = slice / per_row;
    int j = slice % per_row;
    const bool is_v = j >= Hkv;
    if (is_v) j -= Hkv;
    const int pos = p0 + i;
    const int d0 = gl * 8;
    // beyond the span or the cache: skipped, never written. Every lane stays
    // in the DPP reduction; the idle ones contribute 0.
    const bool row_ok = i < n && pos >= 0 && pos < S_cap;
    const bool ok = row_ok && d0 < D;

    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = 0.f;
    if (ok) VecIO<uint16_t, 8>::load(qkv + (int64_t)(s0 + i) * row_ts + (is_v ? v_off : k_off) + (int64_t)j * kv_hs + d0, x);
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) a = fmaxf(a, fabsf(x[e]));
    if (GL > 1) a = fmaxf(a, dpp_f32<0xB1>(a));    // quad_perm [1,0,3,2]
    if (GL > 2) a = fmaxf(a, dpp_f32<0x4E>(a));    // quad_perm [2,3,0,1]
    if (GL > 4) a = fmaxf(a, dpp_f32<0x141>(a));   // row_half_mirror: the other quad of the 8
    if (GL > 8) a = fmaxf(a, dpp_f32<0x140>(a));   // row_mirror: the other 8 of the 16

    a = fmaxf(a, 0x1p-64f);
    const float scale = a / 448.0f;
    const float inv = 448.0f / a;
    if (!ok) return;
    u32x2 w;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int p = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * h] * inv, x[4 * h + 1] * inv, 0, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(x[4 * h + 2] * inv, x[4 * h + 3] * inv, p, true);
        w[h] = (uint32_t)p;
    }
    uint8_t* dst = (is_v ? v_cache : k_cache) + (int64_t)b * c_bs + (int64_t)pos * c_ts + (int64_t)j * c_hs + d0;
    *(u32x2*)dst = w;
    if (gl == 0) (is_v ? v_scale : k_scale)[(int64_t)b * s_bs + (int64_t)j * s_hs + pos] = scale;
}

extern "C" int dolomite_kv_cache_append_fp8(dolomite_stream_t stream, const void* qkv,
                                            const int32_t* src_begin, const int32_t* src_end,
                                            const int32_t* dst_pos, void* k_cache, void* v_cache,
                                            float* k_scale, float* v_scale,
                                            int batch, int max_rows, int Hkv, int D, int S_cap,
                                            int64_t row_tstride, int64_t k_off, int64_t v_off, int64_t kv_hstride,
                                            int64_t cache_bstride, int64_t cache_tstride, int64_t cache_hstride,
                                            int64_t scale_bstride, int64_t scale_hstride, int dtype) {
    if (dtype != DOLOMITE_BF16) return 9010;
    if (batch < 0 || max_rows < 0 || Hkv <= 0 || S_cap < 0 || batch > 65535) return 9030;
    // 16-byte loads, 8-byte stores: head dim and every stride / offset in
    // units of 8 elements; a slice is one group of at most 16 lanes
    if (D <= 0 || D % 8 != 0 || D > 128) return 9031;
    if ((row_tstride | k_off | v_off | kv_hstride | cache_bstride | cache_tstride | cache_hstride) % 8 != 0)
        return 9031;
    if (batch == 0 || max_rows == 0) return 0;
    const int gl = D <= 8 ? 1 : D <= 16 ? 2 : D <= 32 ? 4 : D <= 64 ? 8 : 16;
    const int64_t nblocks = ((int64_t)max_rows * 2 * Hkv * gl + 255) / 256;
    if (nblocks * 256 > 0x7fffffff) return 9030;   // the kernel's slice index is an int
    dim3 grid((unsigned)nblocks, batch), block(256);
#define CASE(GLV)                                                                                        \
    hipLaunchKernelGGL(kv_cache_append_fp8_kernel<GLV>, grid, block, 0, (hipStream_t)stream,             \
                       (const uint16_t*)qkv, src_begin, src_end, dst_pos, (uint8_t*)k_cache,             \
                       (uint8_t*)v_cache, k_scale, v_scale, max_rows, Hkv, D, S_cap,                     \
                       row_tstride, k_off, v_off, kv_hstride, cache_bstride, cache_tstride,              \
                       cache_hstride, scale_bstride, scale_hstride)
    switch (gl) {
        case 1: CASE(1); break;
        case 2: CASE(2); break;
        case 4: CASE(4); break;
        case 8: CASE(8); break;
        default: CASE(16); break;
    }
#undef CASE
    return dol_last_error();
}
