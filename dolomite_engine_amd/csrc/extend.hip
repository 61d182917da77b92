// dolomite_hip — extend attention for gfx950 (MI355X): several new query
// tokens per sequence attend causally over that sequence's KV cache (the next
// turn of a cached conversation, a column chunk of a long prefill, the verify
// pass over 2-8 draft tokens).
//
// It sits between the two kernels the project already has: the forward flash
// kernel (attention.hip) takes q and k from the same rows of one buffer and
// cannot address the (B, S_cap, Hkv, D) cache; the decode kernel (decode.hip)
// has one query row per head and no causal mask.
//
// The cache ALREADY holds the new tokens' K/V (kv_cache_append has run): with
// n_b new tokens and past_b = cache_len[b] - n_b, query i of sequence b
// attends keys [0, past_b + i + 1) — the bottom-right-aligned causal mask.
//
// Design:
//   - the forward kernel's orientation, S^T = K*Q^T and O^T = V^T*P^T with
//     v_mfma_f32_16x16x32_bf16, on a column mapping of its own: the B-operand
//     columns are (query, q-head-of-this-kv-head) PAIRS, flattened query-major
//     for one (sequence, kv head): r = i*G + g. A workgroup (8 waves) owns 128
//     consecutive r, a wave 16 of them, a lane ONE: its q row, causal bound
//     and output row follow from r / G and r % G, computed once per lane.
//     G = 32 with 4 draft tokens fills a workgroup as G = 1 with 128 queries
//     does, and every column shares one pass over the kv head's K/V.
//   - K/V are read once per workgroup: 64-key tiles of the cache, by its
//     (batch, position, head) strides, staged with guarded 16-byte loads into
//     the row-major LDS images of mfma_tiles.h (FaKvLds) and shared by all
//     waves. K rows are the A operand by b128 reads, Q^T sits in registers; P
//     packs to bf16 in registers as the B operand of the second product,
//     whose A operand is the tr16 ladder over the V image.
//   - keys at or beyond the workgroup's last visible key are never staged as
//     they are: their image rows are SELECTED to zero (the cache behind
//     cache_len is uninitialised and may hold NaN / Inf) and their scores to
//     -inf. Keys in [bound, cache_len) are finite values of later queries of
//     the same chunk: their scores are selected to -inf, so P is exactly +0.
//   - masks are wave-uniform where they can be: a tile below the smallest
//     bound of the wave's columns takes the compare-free path, a tile at or
//     above the wave's largest bound is skipped by that wave, a tile at or
//     above the workgroup's largest bound is not staged at all.
//   - split-KV as in decode.hip: grid (nsplit, q-tiles * batch, Hkv), split c
//     owns keys [c*chunk, min((c+1)*chunk, kmax)) of the workgroup's largest
//     bound kmax. nsplit == 1 stores o directly; otherwise fp32 partials go
//     exclusively into caller scratch and a second kernel joins them in
//     ascending split order. No atomics: bitwise reproducible.
//
// Fragment layouts and "permuted key order": see attention.hip.

#include "extend_common.h"

template <int DPAD>
__global__ void __launch_bounds__(512, 4) fa_extend_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ kc, const __bf16* __restrict__ vc,
    __bf16* __restrict__ o, float* __restrict__ part_o, float* __restrict__ part_m,
    float* __restrict__ part_l,
    const int32_t* __restrict__ seq_begin, const int32_t* __restrict__ seq_end,
    const int32_t* __restrict__ cache_len,
    int qtiles, int max_new, int T, int H, int D, int G, int max_len, int chunk,
    int64_t q_ts, int64_t q_gs, int64_t k_bs, int64_t k_ts, int64_t k_hs,
    int64_t v_bs, int64_t v_ts, int64_t v_hs, float scale) {
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

    // wave-uniform key ranges: kmax is the workgroup's largest bound, the
    // wave's columns see at least wmin and at most wmax keys
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

    extern __shared__ char smem_raw[];             // FaKvLds<DPAD>::image_bytes
    __bf16* Klds = (__bf16*)smem_raw;              // [64 key][SK]
    __bf16* Vlds = Klds + 64 * SK;                 // [64 key][SK]

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

    // m_run is identical on the column's 4 lanes; l_run is this lane's
    // partial sum (its 16 keys per tile), joined in the epilogue
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

    // tile-invariant staging coordinates: piece p of a tile is 8 head-dim
    // elements d0.. of key row p / (D/8); at most 2 pieces per thread
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
    const __bf16* kbase = kc + (int64_t)b * k_bs + (int64_t)kvh * k_hs;
    const __bf16* vbase = vc + (int64_t)b * v_bs + (int64_t)kvh * v_hs;

    const float scale2 = scale * EXT_LOG2E;  // exp2-domain scores

    for (int t = 0; t < ntiles; ++t) {
        const int ks = k0 + t * EXT_KTILE;

        // --- stage keys [ks, ks + 64): rows at or beyond kend read the row
        // kend - 1 (inside the cache: the tile holds a key below kend) and
        // are written as zeros ---
        bf16x8 kp[2], vp[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t row = min(ks + st_key[j], kend - 1);
            kp[j] = *(const bf16x8*)(kbase + row * k_ts + st_d0[j]);
            vp[j] = *(const bf16x8*)(vbase + row * v_ts + st_d0[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const bool kvalid = ks + st_key[j] < kend;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                kp[j][e] = kvalid ? kp[j][e] : (__bf16)0.f;
                vp[j][e] = kvalid ? vp[j][e] : (__bf16)0.f;
            }
            if (st_on[j]) {
                *(bf16x8*)&Klds[st_key[j] * SK + st_d0[j]] = kp[j];
                *(bf16x8*)&Vlds[st_key[j] * SK + st_d0[j]] = vp[j];
            }
        }
        __syncthreads();

        // a tile at or above every bound of the wave: all of its P is +0
        if (ks < wmax) {
            // --- S^T = K*Q^T: sc[cb][x] is (column r, key ks + 16cb + 4lg + x) ---
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

            // --- mask + online softmax (fp32), one column per lane. Only a
            // tile that crosses a bound of the wave compares per element. ---
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
            // order the V^T ladder contracts in
            bf16x8 pf[2];
            float rsum = 0.f;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb)
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const float e = exp2f(fmaf(sc[cb][x], scale2, -mref));
                    pf[cb >> 1][(cb & 1) * 4 + x] = (__bf16)e;
                    rsum += e;
                }
            l_run = l_run * alpha + rsum;
            // exact skip: alpha is 1.0f wherever the running max did not move
            if (!__all(alpha == 1.0f)) {
#pragma unroll
                for (int dc = 0; dc < DCH; ++dc)
#pragma unroll
                    for (int x = 0; x < 4; ++x) o_acc[dc][x] *= alpha;
            }

            // --- O^T += V^T*P^T: the K reads above were consumed by the
            // score MFMAs, so no LDS op is outstanding when the ladder opens ---
            tr16_ladder<3, 2 * DCH>(
                aV0, aV1, [](int i) { return ((i / DCH) * 32 * SK + (i % DCH) * 16) * 2; },
                [&](auto i, bf16x8 vf) {
                    constexpr int c2 = decltype(i)::value / DCH, dc = decltype(i)::value % DCH;
                    o_acc[dc] = MFMA16(vf, pf[c2], o_acc[dc]);
                });
        }
        __syncthreads();  // K/V images reused by the next tile
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

// Join the splits of one (sequence, query, head) in ascending split order;
// thread t owns dims [4t, 4t + 4). Queries at or beyond n_b have no partials
// and no output row.
__global__ void __launch_bounds__(64) fa_extend_combine_kernel(
    const float* __restrict__ part_o, const float* __restrict__ part_m,
    const float* __restrict__ part_l, __bf16* __restrict__ o,
    const int32_t* __restrict__ seq_begin, const int32_t* __restrict__ seq_end,
    const int32_t* __restrict__ cache_len, int max_new, int max_len, int T, int H, int D, int nsplit) {
    const int64_t row = blockIdx.x;          // (b*max_new + i)*H + h
    const int h = (int)(row % H);
    const int i = (int)((row / H) % max_new);
    const int b = (int)(row / H / max_new);
    const ExtSeq sq = ext_seq(seq_begin, seq_end, cache_len, b, max_new, max_len, T);
    const int d0 = threadIdx.x * 4;
    if (i >= sq.n || d0 >= D) return;
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
    *(bf16x4*)&o[((int64_t)(sq.s0 + i) * H + h) * D + d0] = ov;
}

// Host side of the combine, shared with extend_fp8.hip (same partials).
int dol_fa_extend_combine(hipStream_t s, const float* part_o, const float* part_m, const float* part_l,
                          __bf16* o, const int32_t* seq_begin, const int32_t* seq_end,
                          const int32_t* cache_len, int64_t rows, int max_new, int max_len, int T, int H,
                          int D, int nsplit) {
    hipLaunchKernelGGL(fa_extend_combine_kernel, dim3((unsigned)rows), dim3(64), 0, s,
                       part_o, part_m, part_l, o, seq_begin, seq_end, cache_len,
                       max_new, max_len, T, H, D, nsplit);
    return dol_last_error();
}

extern "C" int64_t dolomite_fa_extend_scratch_floats(int batch, int max_new, int H, int D, int nsplit) {
    if (batch < 0 || max_new < 0 || H < 0 || D < 0 || nsplit < 1) return -1;
    if (nsplit == 1) return 0;
    return (int64_t)batch * max_new * H * nsplit * (D + 2);
}

template <int DPAD>
static int launch_fa_extend(hipStream_t s, const __bf16* q, const __bf16* kc, const __bf16* vc, __bf16* o,
                            float* scratch, const int32_t* seq_begin, const int32_t* seq_end,
                            const int32_t* cache_len, int batch, int max_new, int T, int H, int Hkv, int D,
                            int G, int max_len, int nsplit, int chunk, int qtiles,
                            int64_t q_ts, int64_t q_gs, int64_t k_bs, int64_t k_ts, int64_t k_hs,
                            int64_t v_bs, int64_t v_ts, int64_t v_hs, float scale) {
    const int64_t nrows = (int64_t)batch * max_new * H;
    const int64_t nslots = nrows * nsplit;
    float* part_o = scratch;
    float* part_m = scratch ? scratch + nslots * D : nullptr;
    float* part_l = scratch ? part_m + nslots : nullptr;
    dim3 grid(nsplit, qtiles * batch, Hkv), block(512);
    hipLaunchKernelGGL((fa_extend_kernel<DPAD>), grid, block, FaKvLds<DPAD>::image_bytes, s,
                       q, kc, vc, o, part_o, part_m, part_l, seq_begin, seq_end, cache_len,
                       qtiles, max_new, T, H, D, G, max_len, chunk,
                       q_ts, q_gs, k_bs, k_ts, k_hs, v_bs, v_ts, v_hs, scale);
    int rc = dol_last_error();
    if (rc != 0 || nsplit == 1) return rc;
    return dol_fa_extend_combine(s, part_o, part_m, part_l, o, seq_begin, seq_end, cache_len,
                                 nrows, max_new, max_len, T, H, D, nsplit);
}

extern "C" int dolomite_fa_extend(dolomite_stream_t stream,
                                  const void* qkv, const void* k_cache, const void* v_cache, void* o,
                                  float* scratch, const int32_t* seq_begin, const int32_t* seq_end,
                                  const int32_t* cache_len,
                                  int batch, int max_new, int64_t T, int H, int Hkv, int D, int G,
                                  int max_len, int nsplit,
                                  int64_t q_tstride, int64_t q_gstride,
                                  int64_t k_bstride, int64_t k_tstride, int64_t k_hstride,
                                  int64_t v_bstride, int64_t v_tstride, int64_t v_hstride,
                                  float scale, int dtype) {
    if (dtype != DOLOMITE_BF16) return 9010;
    if (D > 128) return 9011;
    if (!(scale > 0.f)) return 9015;
    if (D <= 0 || D % 8 != 0) return 9041;
    if ((q_tstride | q_gstride | k_bstride | k_tstride | k_hstride | v_bstride | v_tstride | v_hstride) % 8 != 0)
        return 9041;
    if (batch < 0 || max_new < 0 || T < 0 || T > 0x7fffffff || max_len < 0 || H <= 0 || Hkv <= 0 || G <= 0 ||
        H != Hkv * G)
        return 9042;
    if (nsplit < 1 || nsplit > 65535 || Hkv > 65535 || batch >= 65535) return 9043;
    const int64_t qtiles = ((int64_t)max_new * G + EXT_COLS - 1) / EXT_COLS;
    if (qtiles * batch > 65535 || (int64_t)batch * max_new * H > 0x7fffffff) return 9043;
    if (nsplit > 1 && scratch == nullptr) return 9044;
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
#define CASE(DP)                                                                                        \
    return launch_fa_extend<DP>(s, (const __bf16*)qkv, (const __bf16*)k_cache, (const __bf16*)v_cache,  \
                                (__bf16*)o, scratch, seq_begin, seq_end, cache_len, batch, max_new,     \
                                (int)T, H, Hkv, D, G, max_len, nsplit, chunk, (int)qtiles,              \
                                q_tstride, q_gstride, k_bstride, k_tstride, k_hstride,                  \
                                v_bstride, v_tstride, v_hstride, scale)
    if (D <= 64) CASE(64);
    if (D <= 96) CASE(96);
    CASE(128);
#undef CASE
}
