// dolomite_hip — extend attention over the fp8 (OCP e4m3) KV cache for gfx950
// (MI355X): several new query tokens per sequence attend causally over a
// cache that decode_fp8.hip's append has quantised (chunked prefill into an
// fp8 cache, a continued conversation, the verify pass over draft tokens).
//
// Semantics, work split and column mapping are extend.hip's, word for word:
// spans, cache_len including the new tokens, the bottom-right causal mask,
// r = i*G + g, 128 columns per 512-thread workgroup, one pass over the kv
// head's K/V, grid (nsplit, q-tiles * batch, Hkv), the wave-uniform ranges
// wmin / wmax / kmax, the split partials and the ascending-order combine.
// The cache layout is decode_fp8.hip's: e4m3 bytes and one fp32 scale per
// (sequence, kv head, position); the values attended are q8 * scale.
//
// What differs is how the bytes move:
//   - a staged piece is 8 head dims = 8 e4m3 bytes, ONE 8-byte global load (a
//     16-byte piece would straddle rows at D = 40 / 72), converted to bf16x8
//     in registers (exact: every finite e4m3 value is a bf16 value) and
//     stored as 16 bytes into the same FaKvLds images. The conversion happens
//     ONCE per workgroup and tile and serves all 128 columns; behind the
//     first barrier the b128 K reads, the tr16 ladder and the MFMAs see the
//     LDS bytes a bf16 cache of the unscaled values would have produced.
//   - the tile's 64 K scales and 64 V scales ride along: threads 0..63 load
//     k_scale[ks + t], threads 64..127 v_scale[ks + t] (coalesced, the index
//     clamped to kend - 1) into 512 bytes of LDS behind the images, under the
//     two barriers that bracket the tile anyway. A lane reads back the four
//     runs of 4 floats of its score registers (keys ks + 16cb + 4lg + x) as
//     ds_read_b128.
//   - the scales enter in fp32, never through a second bf16 rounding of K or
//     V: the K scale multiplies the fp32 score before the mask, the running
//     max and the exponent; the V scale is folded into P (the bf16 B operand
//     holds e * v_scale[key]) while l sums the unscaled e.
//   - bytes and scales behind cache_len are arbitrary (0x7f / 0xff are NaN):
//     no load goes there. Rows and scale indices at or beyond kend clamp to
//     kend - 1; such rows are selected to zero after the conversion and their
//     scores to -inf after the scale multiply, so their P is +0 times a
//     finite scale.

#include "extend_common.h"

template <int DPAD>
__global__ void __launch_bounds__(512, 4) fa_extend_fp8_kernel(
    const __bf16* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const float* __restrict__ k_scale, const float* __restrict__ v_scale,
    __bf16* __restrict__ o, float* __restrict__ part_o, float* __restrict__ part_m,
    float* __restrict__ part_l,
    const int32_t* __restrict__ seq_begin, const int32_t* __restrict__ seq_end,
    const int32_t* __restrict__ cache_len,
    int qtiles, int max_new, int T, int H, int D, int G, int max_len, int chunk,
    int64_t q_ts, int64_t q_gs, int64_t k_bs, int64_t k_ts, int64_t k_hs,
    int64_t v_bs, int64_t v_ts, int64_t v_hs, int64_t s_bs, int64_t s_hs, float scale) {
    constexpr int KCH = DPAD / 32;   // contraction chunks of K*Q^T
    constexpr int DCH = DPAD / 16;   // output row blocks of O^T
    constexpr int SK = FaKvLds<DPAD>::S;

    const int split = blockIdx.x, nsplit = gridDim.x;
    const int b = blockIdx.y / qtiles;
    const int r0 = (blockIdx.y % qtiles) * EXT_COLS;
    const int kvh = blockIdx.z;

    const ExtSeq sq = ext_seq(seq_begin, seq_end, cache_len, b, max_new, max_len, T);
    const int ncols = sq.n * G;
    if (r0 >= ncols) return;   // no column of this sequence here (n_b == 0 included)

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15;
    const int lg = lane >> 4;

    // causal bound of query i: keys [0, min(past + i + 1, len))
    auto bound_of = [&](int i) { return min(sq.past + i + 1, sq.len); };

    // wave-uniform key ranges, as in extend.hip
    const int kmax = bound_of(min((r0 + EXT_COLS - 1) / G, sq.n - 1));
    const int k0 = min(split * chunk, kmax);
    const int kend = min(k0 + chunk, kmax);
    const int ntiles = (kend - k0 + EXT_KTILE - 1) / EXT_KTILE;
    const int rw = r0 + wave * 16;
    const bool wave_full = rw + 16 <= ncols;
    const int wmin = rw < ncols ? min(bound_of(rw / G), kend) : 0;
    const int wmax = rw < ncols ? min(bound_of(min(rw + 15, ncols - 1) / G), kend) : 0;

    // --- this lane's column: query qi, head g of the kv head ---
    const int r = rw + lr;
    const bool cvalid = r < ncols;
    const int qi = cvalid ? r / G : 0;
    const int g = cvalid ? r - qi * G : 0;
    const int lim = cvalid ? min(bound_of(qi), kend) : 0;   // first key this column does not see

    extern __shared__ char smem_raw[];             // FaKvLds<DPAD>::image_bytes + 512
    __bf16* Klds = (__bf16*)smem_raw;              // [64 key][SK]
    __bf16* Vlds = Klds + 64 * SK;                 // [64 key][SK]
    float* Slds = (float*)(smem_raw + FaKvLds<DPAD>::image_bytes);   // [64] K scales, [64] V scales

    // Q^T fragments (B layout: j = lr -> column, k = lg*8+e -> head dim)
    bf16x8 qf[KCH];
    {
        const __bf16* qrow = q + (int64_t)(sq.s0 + qi) * q_ts + (int64_t)kvh * q_gs + (int64_t)g * D;
#pragma unroll
        for (int c = 0; c < KCH; ++c) {
            const int d0 = c * 32 + lg * 8;
            qf[c] = load_bf16x8_guard(qrow + d0, d0, D, cvalid);
        }
    }

    float m_run = -INFINITY, l_run = 0.f;
    f32x4 o_acc[DCH];              // O^T: d = dc*16 + lg*4 + x, column = lr
#pragma unroll
    for (int dc = 0; dc < DCH; ++dc) o_acc[dc] = {0.f, 0.f, 0.f, 0.f};

    unsigned aV0, aV1;
    fa_tr16_perm_bases(Vlds, SK, lane, aV0, aV1);

    if (D < DPAD) {  // pad columns zeroed once: staging only writes [0, D)
        const int padp = (DPAD - D) / 8;
        for (int pidx = threadIdx.x; pidx < 64 * padp; pidx += 512) {
            const int key = pidx / padp;
            const int d0 = D + (pidx % padp) * 8;
            bf16x8 z = {};
            *(bf16x8*)&Klds[key * SK + d0] = z;
            *(bf16x8*)&Vlds[key * SK + d0] = z;
        }
    }

    // tile-invariant staging coordinates: piece p of a tile is the 8 bytes of
    // head dims d0.. of key row p / (D/8); at most 2 pieces per thread
    const int dp = D / 8;
    int st_key[2], st_d0[2];
    bool st_on[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int pidx = (int)threadIdx.x + j * 512;
        st_on[j] = pidx < 64 * dp;
        const int pp = st_on[j] ? pidx : 0;
        st_key[j] = pp / dp;
        st_d0[j] = (pp % dp) * 8;
    }
    const uint8_t* kbase = kc + (int64_t)b * k_bs + (int64_t)kvh * k_hs;
    const uint8_t* vbase = vc + (int64_t)b * v_bs + (int64_t)kvh * v_hs;
    // waves 0 and 1 carry the tile's scales: K on threads 0..63, V on 64..127
    const bool sc_on = wave < 2;
    const float* sbase = (wave == 0 ? k_scale : v_scale) + (int64_t)b * s_bs + (int64_t)kvh * s_hs;

    const float scale2 = scale * EXT_LOG2E;  // exp2-domain scores

    // The loads of the tile at ks: rows and scales at or beyond kend read
    // position kend - 1 (inside the cache and below cache_len: the tile holds
    // a key below kend). 9 registers per thread, half the bf16 kernel's
    // pieces, so the NEXT tile's loads are issued before this tile's MFMAs
    // and fly under them.
    u32x2 kp[2], vp[2];
    float sv = 0.f;
    auto fetch = [&](int ks) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t row = min(ks + st_key[j], kend - 1);
            kp[j] = *(const u32x2*)(kbase + row * k_ts + st_d0[j]);
            vp[j] = *(const u32x2*)(vbase + row * v_ts + st_d0[j]);
        }
        if (sc_on) sv = sbase[min(ks + lane, kend - 1)];
    };
    if (ntiles > 0) fetch(k0);

    for (int t = 0; t < ntiles; ++t) {
        const int ks = k0 + t * EXT_KTILE;

        // --- stage keys [ks, ks + 64): convert, write rows at or beyond
        // kend as zeros ---
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool kvalid = ks + st_key[j] < kend;
            bf16x8 kb = e4m3x8_to_bf16x8(kp[j]);
            bf16x8 vb = e4m3x8_to_bf16x8(vp[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                kb[e] = kvalid ? kb[e] : (__bf16)0.f;
                vb[e] = kvalid ? vb[e] : (__bf16)0.f;
            }
            if (st_on[j]) {
                *(bf16x8*)&Klds[st_key[j] * SK + st_d0[j]] = kb;
                *(bf16x8*)&Vlds[st_key[j] * SK + st_d0[j]] = vb;
            }
        }
        if (sc_on) Slds[wave * 64 + lane] = sv;
        __syncthreads();
        if (t + 1 < ntiles) fetch(ks + EXT_KTILE);   // the next tile holds a key below kend

        // a tile at or above every bound of the wave: all of its P is +0
        if (ks < wmax) {
            // --- S^T = K*Q^T on the unscaled e4m3 values: sc[cb][x] is
            // (column r, key ks + 16cb + 4lg + x) ---
            f32x4 sc[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                sc[cb] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < KCH; ++c) {
                    const bf16x8 kf = *(const bf16x8*)&Klds[(cb * 16 + lr) * SK + c * 32 + lg * 8];
                    sc[cb] = MFMA16(kf, qf[c], sc[cb]);
                }
            }

            // --- K scale (fp32), then mask + online softmax, one column per
            // lane. Only a tile that crosses a bound of the wave compares per
            // element. ---
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const f32x4 ksv = *(const f32x4*)&Slds[cb * 16 + lg * 4];
#pragma unroll
                for (int x = 0; x < 4; ++x) sc[cb][x] *= ksv[x];
            }
            if (!(wave_full && ks + EXT_KTILE <= wmin)) {
#pragma unroll
                for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        const int kpos = ks + cb * 16 + lg * 4 + x;
                        sc[cb][x] = (kpos < lim) ? sc[cb][x] : -INFINITY;
                    }
            }
            float mx[4];
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
                mx[cb] = fmaxf(fmaxf(sc[cb][0], sc[cb][1]), fmaxf(sc[cb][2], sc[cb][3]));
            const float rowmax = qgroup_reduce_max(fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3])));
            // a column without a visible key so far keeps m_run = -inf (the
            // split join weighs by it); its exponent reference is 0, so
            // every weight is exp2(-inf) = +0 and nothing is NaN
            const float mnew = fmaxf(m_run, rowmax * scale2);
            const float mref = (mnew == -INFINITY) ? 0.f : mnew;
            const float alpha = exp2f(m_run - mref);
            m_run = mnew;

            // pf[c] element e is key 32c + 16*(e>>2) + 4*lg + (e&3): the
            // order the V^T ladder contracts in. The V scale rides on P; a
            // masked key is +0 times a finite scale (the index was clamped).
            bf16x8 pf[2];
            float rsum = 0.f;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const f32x4 vsv = *(const f32x4*)&Slds[64 + cb * 16 + lg * 4];
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const float e = exp2f(fmaf(sc[cb][x], scale2, -mref));
                    pf[cb >> 1][(cb & 1) * 4 + x] = (__bf16)(e * vsv[x]);
                    rsum += e;
                }
            }
            l_run = l_run * alpha + rsum;
            // exact skip: alpha is 1.0f wherever the running max did not move
            if (!__all(alpha == 1.0f)) {
#pragma unroll
                for (int dc = 0; dc < DCH; ++dc)
#pragma unroll
                    for (int x = 0; x < 4; ++x) o_acc[dc][x] *= alpha;
            }

            // --- O^T += V^T*P^T: the K and scale reads above were consumed by
            // the score MFMAs and the softmax, so no LDS op is outstanding
            // when the ladder opens ---
            tr16_ladder<3, 2 * DCH>(
                aV0, aV1, [](int i) { return ((i / DCH) * 32 * SK + (i % DCH) * 16) * 2; },
                [&](auto i, bf16x8 vf) {
                    constexpr int c2 = decltype(i)::value / DCH, dc = decltype(i)::value % DCH;
                    o_acc[dc] = MFMA16(vf, pf[c2], o_acc[dc]);
                });
        }
        __syncthreads();  // K/V images and scales reused by the next tile
    }

    // --- epilogue: join the column's 4 partial sums; store o, or the
    // split's partials (a split without keys stores m = -inf, l = 0, O = 0) ---
    const float l_col = qgroup_reduce_sum(l_run);
    const int h = kvh * G + g;
    if (nsplit == 1) {
        const float inv_l = (l_col > 0.f) ? 1.f / l_col : 0.f;
        __bf16* orow = o + ((int64_t)(sq.s0 + qi) * H + h) * D;
        fa_store_rowT_bf16<DCH>(orow, o_acc, inv_l, cvalid, D, lg);
    } else if (cvalid) {
        const int64_t slot = (((int64_t)b * max_new + qi) * H + h) * nsplit + split;
        float* prow = part_o + slot * D;
#pragma unroll
        for (int dc = 0; dc < DCH; ++dc) {
            const int d0 = dc * 16 + lg * 4;
            if (d0 < D) *(f32x4*)&prow[d0] = o_acc[dc];
        }
        if (lg == 0) {
            part_m[slot] = m_run;
            part_l[slot] = l_col;
        }
    }
}

template <int DPAD>
static int launch_fa_extend_fp8(hipStream_t s, const __bf16* q, const uint8_t* kc, const uint8_t* vc,
                                const float* k_scale, const float* v_scale, __bf16* o,
                                float* scratch, const int32_t* seq_begin, const int32_t* seq_end,
                                const int32_t* cache_len, int batch, int max_new, int T, int H, int Hkv, int D,
                                int G, int max_len, int nsplit, int chunk, int qtiles,
                                int64_t q_ts, int64_t q_gs, int64_t k_bs, int64_t k_ts, int64_t k_hs,
                                int64_t v_bs, int64_t v_ts, int64_t v_hs, int64_t s_bs, int64_t s_hs,
                                float scale) {
    const int64_t nrows = (int64_t)batch * max_new * H;
    const int64_t nslots = nrows * nsplit;
    float* part_o = scratch;
    float* part_m = scratch ? scratch + nslots * D : nullptr;
    float* part_l = scratch ? part_m + nslots : nullptr;
    // the two images, then the tile's 64 K scales and 64 V scales
    constexpr size_t lds = FaKvLds<DPAD>::image_bytes + 2 * EXT_KTILE * sizeof(float);
    static_assert(lds <= 48 * 1024, "within the default dynamic-LDS limit");
    dim3 grid(nsplit, qtiles * batch, Hkv), block(512);
    hipLaunchKernelGGL((fa_extend_fp8_kernel<DPAD>), grid, block, lds, s,
                       q, kc, vc, k_scale, v_scale, o, part_o, part_m, part_l, seq_begin, seq_end, cache_len,
                       qtiles, max_new, T, H, D, G, max_len, chunk,
                       q_ts, q_gs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs, s_bs, s_hs, scale);
    int rc = dol_last_error();
    if (rc != 0 || nsplit == 1) return rc;
    return dol_fa_extend_combine(s, part_o, part_m, part_l, o, seq_begin, seq_end, cache_len,
                                 nrows, max_new, max_len, T, H, D, nsplit);
}

extern "C" int dolomite_fa_extend_fp8(dolomite_stream_t stream,
                                      const void* qkv, const void* k_cache, const void* v_cache,
                                      const float* k_scale, const float* v_scale, void* o,
                                      float* scratch, const int32_t* seq_begin, const int32_t* seq_end,
                                      const int32_t* cache_len,
                                      int batch, int max_new, int64_t T, int H, int Hkv, int D, int G,
                                      int max_len, int nsplit,
                                      int64_t q_tstride, int64_t q_gstride,
                                      int64_t k_bstride, int64_t k_tstride, int64_t k_hstride,
                                      int64_t v_bstride, int64_t v_tstride, int64_t v_hstride,
                                      int64_t s_bstride, int64_t s_hstride,
                                      float scale, int dtype) {
    // dolomite_fa_extend's checks in its order, plus the scale arguments
    if (dtype != DOLOMITE_BF16) return 9010;
    if (D > 128) return 9011;
    if (!(scale > 0.f)) return 9015;
    if (D <= 0 || D % 8 != 0) return 9041;
    // 16-byte q loads, 8-byte cache loads: every stride in units of 8 elements
    if ((q_tstride | q_gstride | k_bstride | k_tstride | k_hstride | v_bstride | v_tstride | v_hstride) % 8 != 0)
        return 9041;
    if (batch < 0 || max_new < 0 || T < 0 || T > 0x7fffffff || max_len < 0 || H <= 0 || Hkv <= 0 || G <= 0 ||
        H != Hkv * G)
        return 9042;
    if (s_bstride < 0 || s_hstride < 0) return 9042;
    if (nsplit < 1 || nsplit > 65535 || Hkv > 65535 || batch >= 65535) return 9043;
    const int64_t qtiles = ((int64_t)max_new * G + EXT_COLS - 1) / EXT_COLS;
    if (qtiles * batch > 65535 || (int64_t)batch * max_new * H > 0x7fffffff) return 9043;
    if (nsplit > 1 && scratch == nullptr) return 9044;
    if (k_scale == nullptr || v_scale == nullptr) return 9045;
    // o's rows outside every span (disjoint from every row stored below)
    int rc = dolomite_fa_zero_gap_rows(stream, o, (int64_t)H * D * (int64_t)sizeof(__bf16),
                                       seq_begin, seq_end, batch, T);
    if (rc != 0) return rc;
    if (batch == 0 || max_new == 0) return 0;   // every row is a gap row
    // keys per split: ceil(max_len / nsplit) rounded up to the key tile
    int chunk = (max_len + nsplit - 1) / nsplit;
    chunk = (chunk + EXT_KTILE - 1) / EXT_KTILE * EXT_KTILE;
    if (chunk == 0) chunk = EXT_KTILE;
    hipStream_t s = (hipStream_t)stream;
#define CASE(DP)                                                                                          \
    return launch_fa_extend_fp8<DP>(s, (const __bf16*)qkv, (const uint8_t*)k_cache,                       \
                                    (const uint8_t*)v_cache, k_scale, v_scale, (__bf16*)o, scratch,       \
                                    seq_begin, seq_end, cache_len, batch, max_new, (int)T, H, Hkv, D, G,  \
                                    max_len, nsplit, chunk, (int)qtiles, q_tstride, q_gstride,            \
                                    k_bstride, k_tstride, k_hstride, v_bstride, v_tstride, v_hstride,     \
                                    s_bstride, s_hstride, scale)
    if (D <= 64) CASE(64);
    if (D <= 96) CASE(96);
    CASE(128);
#undef CASE
}
