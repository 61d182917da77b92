// dolomite_hip — varlen causal flash attention for gfx950 (MI355X).
//
// Replaces flash_attn_varlen_func at the reference call site
// attention/padding_free.py:51-62 (and flash.py:112-123): causal attention
// over packed (total_q, heads, head_dim) with cu_seqlens, MHA/GQA/MQA head
// layouts addressed in place on the fused c_attn projection output
// (attention/base.py:72-81) via (t_stride, group_stride) addressing.
// Sequences need not be back to back: the kernels take per-sequence row
// spans [seq_begin[b], seq_end[b]) — (cu_seqlens, cu_seqlens + 1) for the
// packed case, one span per row of a padded (B, S) batch for the dense
// flash path of attention/flash.py ("Span entry points" below).
//
// Design (CDNA4-first):
//   - MFMA v_mfma_f32_16x16x32_bf16 for both products; 64-wide waves.
//   - forward: workgroup = 8 waves = 512 threads; q-tile 128 rows (16 per
//     wave), k-tile 64 keys streamed through LDS as two row-major [key][d]
//     images in natural row order (stride DPAD+16: the b128 row reads, the
//     staging writes and the transpose reads are all conflict-free).
//   - the score tile is computed TRANSPOSED, S^T = K*Q^T (K image row as
//     the A operand, the wave's Q register fragment as B), so a lane owns
//     ONE q row: 16 of its 64 scores per tile, the other 48 on the lanes
//     l^16, l^32, l^48 (see "Swapped-operand score tiles").
//   - online softmax in fp32 VGPRs with one m / alpha per lane; the row max
//     crosses the 4 lane groups with v_permlane16_swap + v_permlane32_swap
//     (VALU, no LDS); the row sum stays a per-lane partial until the
//     epilogue; the softmax scale is one FMA inside the exponent.
//   - P never touches LDS: the lane's 16 probabilities pack into the B
//     operand of O^T = V^T*P^T, whose A operand is a ds_read_b64_tr_b16 of
//     the V image in the matching (permuted) key order, through a depth-3
//     counted ladder. O^T leaves as one 8-byte store per lane and 16-wide
//     head-dim block.
//   - LSE (H,T) fp32 written for backward; backward recomputes P. dkv
//     writes per-q-head (T, H, D) fp32 partials (exclusive stores, no
//     atomics) reduced in fixed order by the finalize kernel —
//     deterministic gradients; dq uses the forward's orientation (S^T and
//     dP^T with the q row on the lane, dS packed in registers into
//     dQ^T = K^T*dS^T) and stores bf16 straight into the packed dqkv. dkv
//     contracts over q with the KEY on the lane (S = Q*K^T, dP = dO*V^T),
//     so its P / dS also pack in registers, into dV^T = dO^T*P and
//     dK^T = Q^T*dS — no kernel routes P or dS through LDS.
//   - attention dropout (flash_attn_varlen_func's dropout_p) is fused: the
//     keep-mask is a pure counter-based hash of (seed, q-head, global q
//     token, global k token) — see "Attention dropout keep-mask" below and
//     include/dolomite_hip.h — regenerated identically by fwd, dkv and dq
//     from their own lane->(q, k) mappings and never written to memory.
//     The kernels are templated on DROPOUT; p = 0 dispatches the
//     DROPOUT=false instantiations, which compile to the dropout-free code.
//
// Fragment layout assumption for mfma_f32_16x16x32_bf16 (verified on
// hardware by dolomite_mfma_probe, tests/test_gpu_kernels.py):
//   A[i][k]: lane l holds i = l&15, k = (l>>4)*8 + e   (e = 0..7)
//   B[k][j]: lane l holds k = (l>>4)*8 + e, j = l&15
//   C[r][c]: lane l, reg x holds r = (l>>4)*4 + x, c = l&15

// The parts all three hot kernels share — fragment types, the tr16 ladder,
// the guarded load, row reductions, the transposed epilogue store, the K/V
// image geometry — live in mfma_tiles.h (decode.hip uses some of them too).

#include "mfma_tiles.h"

// softmax runs in the exp2 domain: v_exp_f32 natively computes 2^x, so
// folding log2(e) into the softmax scale removes one multiply per element
#define DOL_LOG2E 1.44269504088896340736f
#define DOL_LN2 0.69314718055994530942f

// ---------------------------------------------------------------------------
// ds_read_b64_tr_b16 — gfx950 hardware transpose read (semantics pinned on
// HW by dolomite_tr16_probe): each lane reads 64b at its own 8B-aligned LDS
// address; within a 16-lane group, output lane l slot j receives element
// (l&3) of the word read by lane (l&48) + 4j + ((l>>2)&3).
//
// Feeding an MFMA B-fragment B[k=(l>>4)*8+e][j=l&15] for a 32-row
// contraction chunk at `rowbase`, 16-col block at `d0`, from a ROW-MAJOR
// image with stride S: lane l passes the address of
//   row = rowbase + 8*(l>>4) + 4h + ((l>>2)&3),  col = d0 + 4*(l&3)
// and read h delivers fragment elements e = 4h..4h+3.
//
// Conflicts (tools_lds_sim.py, validated against SQ_LDS_BANK_CONFLICT):
// with S=112 the natural row order 2-way conflicts for THIS row pattern
// (rows 0 and 8 alias); storing image rows with bits 2 and 3 SWAPPED makes
// both the tr reads and the b128 row-major B-frag reads conflict-free
// (lds_tr16_bfrag / dolomite_tr16_bfrag_probe keep that reader). The fwd /
// dq / dkv ladders read in the permuted order of "Swapped-operand score
// tiles" (8 consecutive rows per 32-lane pass), which is conflict-free in
// natural row order and 2-way conflicted under PI23: all three use natural
// rows.
// ---------------------------------------------------------------------------
#define PI23(q) (((q) & ~12) | ((((q) >> 2) & 1) << 3) | ((((q) >> 3) & 1) << 2))

// The reads and their waitcnt MUST live in one asm block: the compiler
// assumes an asm statement completes synchronously, so with a separate wait
// it is free to copy/shuffle the "ready" result registers before the data
// actually lands (observed as silent corruption of one of two fragments).
// Earlyclobber outputs keep the dest registers disjoint from the address
// operands of later reads in the same block.

// B-fragment from a PI23 row-major image: rowbase = 32-row chunk start
// (multiple of 32), d0 = 16-col block start.
__device__ __forceinline__ bf16x8 lds_tr16_bfrag(const __bf16* img, int rowbase, int S, int d0, int lane) {
    const int g8 = (lane >> 4) * 8;
    const int jj = (lane >> 2) & 3;
    const int cc = (lane & 3) * 4;
    unsigned a0 = (unsigned)(size_t)(img + PI23(rowbase + g8 + jj) * S + d0 + cc);
    unsigned a1 = (unsigned)(size_t)(img + PI23(rowbase + g8 + 4 + jj) * S + d0 + cc);
    bf16x4 lo, hi;
    asm volatile(
        "ds_read_b64_tr_b16 %0, %2\n\t"
        "ds_read_b64_tr_b16 %1, %3\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(lo), "=&v"(hi)
        : "v"(a0), "v"(a1)
        : "memory");
    bf16x8 out;
#pragma unroll
    for (int t = 0; t < 4; ++t) { out[t] = lo[t]; out[4 + t] = hi[t]; }
    return out;
}

// XCD-aware block remap (guide T1): the dispatcher places flat block id b on
// XCD b%8, so the raw grid (tile, seq, head) spreads one (seq, head)'s tiles
// over all 8 L2s and every tile re-fetches the same Q/dO/K/V slices from HBM
// (measured: 16 GB/launch vs ~1 GB algorithmic on the backward dkv kernel).
// Remap so ALL tiles of one (seq, head) stay on ONE XCD and run
// back-to-back: its ~1.3 MB working set then lives in that XCD's 4 MB L2.
// Pure permutation — correctness never depends on placement.
__device__ __forceinline__ void xcd_remap_tile_bh(int& tile, int& b, int& h) {
    const int ntile = gridDim.x, nb = gridDim.y, nh = gridDim.z;
    const int64_t nbh = (int64_t)nb * nh;
    if (nbh % 8 != 0) return;  // identity fallback for tiny grids
    int64_t raw = blockIdx.x + (int64_t)ntile * (blockIdx.y + (int64_t)nb * blockIdx.z);
    int xcd = (int)(raw % 8);
    int64_t idx = raw / 8;             // per-XCD sequence number
    int64_t pair_local = idx / ntile;  // which (seq, head) pair on this XCD
    tile = (int)(idx % ntile);
    int64_t pair = pair_local * 8 + xcd;
    b = (int)(pair % nb);
    h = (int)(pair / nb);
}

// ===========================================================================
// Attention dropout keep-mask (definition: include/dolomite_hip.h; Python
// restatement: ops/functional.py attention_dropout_keep_mask).
//
// keep(seed, h, t_q, t_k) is a pure function of the 64-bit seed, the q-head
// and the GLOBAL packed token indices, so fwd, dkv and dq — which hold P in
// three different lane layouts — regenerate the same bit without ever
// storing the mask. Per element and integer-only: the per-row word depends
// on (seed_lo, t_q), the per-column word on (seed_hi, h, t_k); whichever of
// the two is fixed for a lane is hoisted out of the tile loop, the other is
// computed once per 4 elements, and only drop_keep_words runs per element.
// ===========================================================================
#define DOL_DROP_CQ 0x9E3779B1u
#define DOL_DROP_CK 0x85EBCA77u
#define DOL_DROP_CH 0xC2B2AE3Du
#define DOL_DROP_M1 0x7FEB352Du
#define DOL_DROP_M2 0x846CA68Bu

__device__ __forceinline__ uint32_t drop_mix32(uint32_t x) {
    x ^= x >> 16;
    x *= DOL_DROP_M1;
    x ^= x >> 15;
    x *= DOL_DROP_M2;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t drop_head_word(uint32_t seed_hi, uint32_t h) {
    return drop_mix32(seed_hi ^ (h * DOL_DROP_CH));
}
__device__ __forceinline__ uint32_t drop_row_word(uint32_t seed_lo, uint32_t t_q) {
    return drop_mix32(seed_lo ^ (t_q * DOL_DROP_CQ));
}
__device__ __forceinline__ uint32_t drop_col_word(uint32_t head_word, uint32_t t_k) {
    return drop_mix32(head_word ^ (t_k * DOL_DROP_CK));
}
// the compare reads x from the top, so the mixer's last xorshift (which only
// folds high bits into the low half) is omitted
__device__ __forceinline__ bool drop_keep_words(uint32_t rw, uint32_t cw, uint32_t thr) {
    uint32_t x = rw ^ cw;
    x ^= x >> 16;
    x *= DOL_DROP_M1;
    x ^= x >> 15;
    x *= DOL_DROP_M2;
    return x >= thr;
}
__device__ __forceinline__ bool drop_keep(uint32_t seed_lo, uint32_t seed_hi, uint32_t h,
                                          uint32_t t_q, uint32_t t_k, uint32_t thr) {
    return drop_keep_words(drop_row_word(seed_lo, t_q),
                           drop_col_word(drop_head_word(seed_hi, h), t_k), thr);
}

// host: keep iff x >= floor(p * 2^32), p taken as the IEEE float32 it is
static inline uint32_t drop_threshold(float p_drop) {
    return (uint32_t)((double)p_drop * 4294967296.0);
}
static inline bool drop_p_valid(float p_drop) { return p_drop >= 0.f && p_drop < 1.f; }

// ===========================================================================
// Swapped-operand score tiles (fwd, dq): S^T = K*Q^T
//
// With the K image row as the MFMA A operand and the wave's Q register
// fragment as B (the A and B lane maps are symmetric, so the fragment is the
// one Q*K^T used), the C fragment of key block cb holds, on lane l reg x,
//   q row  l & 15            key  16*cb + 4*(l>>4) + x.
// One q row's 64 scores are then 16 registers on each of the 4 lanes
// {l, l^16, l^32, l^48}: the row statistics are one value per lane, and the
// 8 values of key blocks (2c, 2c+1) pack, with no lane movement and no LDS,
// into the B operand of the next product (O^T = V^T*P^T, dQ^T = K^T*dS^T).
// That fragment's element e on lane group g is key
//   32c + 16*(e>>2) + 4g + (e&3)                    ("permuted key order"),
// and the A operand of the next product must contract in the same order:
// it is a tr16 read of the row-major V (dq: K) image whose per-lane row
// address is 32c + 16h + 4g + ((l>>2)&3) for read h — fa_tr16_perm_bases.
// Outputs come out transposed (head-dim 16*dc + 4g + x on the registers,
// q on l & 15): 4 contiguous bf16 per lane and block, one 8-byte store.
// ===========================================================================

// ===========================================================================
// Forward
// ===========================================================================

template <int DPAD, bool DROPOUT>
__global__ void __launch_bounds__(512, 4) fa_fwd_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    __bf16* __restrict__ o, float* __restrict__ lse,
    const int32_t* __restrict__ seq_begin, const int32_t* __restrict__ seq_end,
    int H, int Hkv, int D, int G,
    int64_t q_ts, int64_t q_gs, int64_t k_ts, int64_t k_hs, int64_t v_ts, int64_t v_hs,
    int64_t o_ts, int64_t T_total, float scale,
    uint32_t seed_lo, uint32_t seed_hi, uint32_t drop_thr, float drop_rp) {
    constexpr int KCH = DPAD / 32;   // contraction chunks for QK^T
    constexpr int DCH = DPAD / 16;   // output row blocks of O^T
    constexpr int SK = FaKvLds<DPAD>::S;   // K/V LDS row stride (elems), conflict-free (mfma_tiles.h)

    int tile_id = blockIdx.x, b = blockIdx.y, h = blockIdx.z;
    xcd_remap_tile_bh(tile_id, b, h);
    // span-derived values are wave-uniform: pin them to SGPRs so per-lane
    // address arithmetic built on them does not hold VGPR pairs across the
    // main loop (measured: the compiler otherwise spills pointer pairs)
    const int s0 = __builtin_amdgcn_readfirstlane(seq_begin[b]);
    const int L = __builtin_amdgcn_readfirstlane(seq_end[b]) - s0;
    // heaviest tiles (largest qs -> most k-tiles) dispatch FIRST: in-order
    // dispatch otherwise schedules the long-pole causal workgroups last
    // 8 waves x 16 rows = 128 q rows per workgroup: K/V staging and
    // barriers amortize over twice the compute at the same per-wave
    // register budget
    const int ntile_seq = (L + 127) / 128;
    if (tile_id >= ntile_seq) return;
    const int qs = (ntile_seq - 1 - tile_id) * 128;

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lr = lane & 15;   // fragment col / A-row index
    const int lg = lane >> 4;   // fragment k-group / C-row group

    // Two double-buffered staging pipelines were built and MEASURED OUT:
    //   (a) register-staged issue-early/write-late: 5.44 -> 5.84 ms (the
    //       write pass serializes behind the MFMAs, guide T14's warning);
    //   (b) LDS-DMA (buffer_load..lds) into the inactive buffer: wall-time
    //       NEUTRAL (5.65 ms) and NUMERICALLY UNSAFE as compiled — hipcc
    //       waterfalls the buffer descriptors it cannot prove wave-uniform
    //       (T20) and issues some chunk DMAs under partial exec masks, so
    //       inactive lanes leave stale LDS in the image (flaky parity
    //       failures across runs; see git history for the full variant).
    // The (512, 4) bound (<= 128 VGPR, 4 waves/SIMD) keeps 2 of these
    // 8-wave workgroups on a CU: the co-resident workgroup already hides
    // staging latency, so the single-buffer two-barrier schedule stays.
    extern __shared__ char smem_raw[];             // FaKvLds<DPAD>::bytes(DROPOUT)
    __bf16* Klds = (__bf16*)smem_raw;              // [64 key][SK]
    __bf16* Vlds = Klds + 64 * SK;                 // [64 key][SK]
    uint32_t* Cw = (uint32_t*)(Vlds + 64 * SK);    // [64 key] column words (DROPOUT only)
    // V is stored row-major (coalesced staging) and consumed as the V^T
    // A-fragment via ds_read_b64_tr_b16 — no transposed image, no scatter.

    const int kvh = h / G;
    const int64_t q_hoff = (int64_t)(h / G) * q_gs + (int64_t)(h % G) * D;

    // --- load this wave's Q fragments (B-layout of Q^T: j = lr -> q row,
    // k = lg*8+e -> head dim) ---
    const int qrow = qs + wave * 16 + lr;
    const bool qvalid = qrow < L;
    bf16x8 qf[KCH];
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc) {
        int d0 = kc * 32 + lg * 8;
        const __bf16* p = q + (int64_t)(s0 + (qvalid ? qrow : 0)) * q_ts + q_hoff + d0;
        qf[kc] = load_bf16x8_guard(p, d0, D, qvalid);
    }

    // One q row (qrow) per lane: a single running max and alpha. m_run is
    // identical on the row's 4 lanes; l_run is this lane's PARTIAL row sum
    // (its 16 keys per tile) — alpha is shared, so the partials rescale
    // alike and are joined once, in the epilogue.
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 o_acc[DCH];              // O^T: d = dc*16 + lg*4 + x, q = lr
#pragma unroll
    for (int dc = 0; dc < DCH; ++dc) o_acc[dc] = {0.f, 0.f, 0.f, 0.f};

    // dropout: the lane's q row is fixed for the kernel, so its row word is
    // hoisted. A lane's 16 scores per tile are 16 different keys, so the
    // tile's 64 column words are mixed ONCE per workgroup (wave 0, one key
    // per lane, next to the staging) and read back as four broadcast b128
    // loads — 16 mixes per lane and tile would cost more than the mask test
    uint32_t drop_rw = 0;
    uint32_t drop_hw = 0;
    if constexpr (DROPOUT) {
        drop_hw = drop_head_word(seed_hi, (uint32_t)h);
        drop_rw = drop_row_word(seed_lo, (uint32_t)(s0 + qrow));
    }

    // lane base addresses for the PV tr16 ladder (permuted key order; the
    // per-step (chunk, d0) displacement goes in the ds_read immediate)
    unsigned aV0, aV1;
    fa_tr16_perm_bases(Vlds, SK, lane, aV0, aV1);

    const int kend = min(L, qs + 128);
    const int ntiles = (kend + 63) / 64;

    if (D < DPAD) {  // pad columns zeroed once (see dkv note)
        for (int pidx = threadIdx.x; pidx < 64 * (DPAD - D) / 8; pidx += 512) {
            int key = pidx / ((DPAD - D) / 8);
            int d0 = D + (pidx % ((DPAD - D) / 8)) * 8;
            bf16x8 z = {};
            *(bf16x8*)&Klds[key * SK + d0] = z;
            *(bf16x8*)&Vlds[key * SK + d0] = z;
        }
    }

    // tile-invariant staging piece coordinates (see dkv note)
    int st_koff[2], st_voff[2];
    int st_klds[2], st_vlds[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        int pidx = (int)threadIdx.x + j * 512;
        int pp = pidx < 64 * D / 8 ? pidx : 0;
        int key = pp / (D / 8);
        int d0 = (pp % (D / 8)) * 8;
        st_koff[j] = (int)(key * k_ts + kvh * k_hs) + d0;   // fits 32 bits
        st_voff[j] = (int)(key * v_ts + kvh * v_hs) + d0;
        st_klds[j] = key * SK + d0;
        st_vlds[j] = key * SK + d0;
    }

    // T5 static priority: the later-dispatched half of an 8-wave workgroup
    // loses VALU arbitration; one setprio for it, no per-cluster flips.
    if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256) __builtin_amdgcn_s_setprio(1);

    constexpr int PIECES = 64 * DPAD / 8;  // 8-elem staging pieces

    // direct cooperative staging
    auto stage_direct = [&](int ks_, __bf16* Kw, __bf16* Vw) {
        if (ks_ + 64 <= kend) {
            const int64_t disp = (int64_t)(s0 + ks_);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if ((int)threadIdx.x + j * 512 < 64 * D / 8) {
                    *(bf16x8*)&Kw[st_klds[j]] = *(const bf16x8*)(k + disp * k_ts + st_koff[j]);
                    *(bf16x8*)&Vw[st_vlds[j]] = *(const bf16x8*)(v + disp * v_ts + st_voff[j]);
                }
            }
        } else {
            for (int pidx = threadIdx.x; pidx < PIECES; pidx += 512) {
                int key = pidx / (DPAD / 8);
                int d0 = (pidx % (DPAD / 8)) * 8;
                bool kv_valid = (ks_ + key) < kend;
                const __bf16* kp = k + (int64_t)(s0 + (kv_valid ? ks_ + key : 0)) * k_ts + (int64_t)kvh * k_hs + d0;
                *(bf16x8*)&Kw[key * SK + d0] = load_bf16x8_guard(kp, d0, D, kv_valid);
                const __bf16* vp = v + (int64_t)(s0 + (kv_valid ? ks_ + key : 0)) * v_ts + (int64_t)kvh * v_hs + d0;
                *(bf16x8*)&Vw[key * SK + d0] = load_bf16x8_guard(vp, d0, D, kv_valid);
            }
        }
    };


    // softmax scale folded into the exponent as one FMA per score; the row
    // max is taken on the raw scores, which orders them alike for scale > 0
    // (the dispatcher rejects anything else)
    const float scale2 = scale * DOL_LOG2E;  // exp2-domain scores

    auto compute_tile = [&](const __bf16* Kb, unsigned aV0c, unsigned aV1c, int ks) {
        // --- S^T = K*Q^T: 4 key-blocks of 16, accumulate over KCH chunks;
        // sc[cb][x] is (q = qrow, key = ks + 16*cb + 4*lg + x) ---
        f32x4 sc[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            sc[cb] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KCH; ++kc) {
                bf16x8 kf = *(const bf16x8*)&Kb[(cb * 16 + lr) * SK + kc * 32 + lg * 8];
                sc[cb] = MFMA16(kf, qf[kc], sc[cb]);
            }
        }

        // --- mask + online softmax (fp32), one q row per lane.
        // Wave-uniform mask split: full tiles skip the per-element compare
        // chain entirely (the kernel is issue-bound). No -INFINITY select
        // guards: v_exp_f32(-inf) is exactly +0, and mnew is never -inf
        // after the fully-masked-row force, so exp2f does the zeroing. ---
        const bool edge_tile =
            !((ks + 63 <= qs + wave * 16) && (ks + 64 <= kend) && (qs + wave * 16 + 16 <= L));
        if (__builtin_amdgcn_readfirstlane(edge_tile ? 1 : 0)) {
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const int kpos = ks + cb * 16 + lg * 4 + x;
                    if (kpos > qrow || kpos >= kend || qrow >= L) sc[cb][x] = -INFINITY;
                }
            }
        }
        float mx[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
            mx[cb] = fmaxf(fmaxf(sc[cb][0], sc[cb][1]), fmaxf(sc[cb][2], sc[cb][3]));
        const float rowmax = qgroup_reduce_max(fmaxf(fmaxf(mx[0], mx[1]), fmaxf(mx[2], mx[3])));
        float mnew = fmaxf(m_run, rowmax * scale2);
        if (mnew == -INFINITY) mnew = 0.f;  // fully-masked row guard
        const float alpha = exp2f(m_run - mnew);
        m_run = mnew;

        // dropout touches ONLY the packed bf16 P: the online softmax
        // (rsum / l_run / m_run, hence lse) sees the undropped e.
        // pf[c] element e is key 32c + 16*(e>>2) + 4*lg + (e&3) — the order
        // the V^T ladder below contracts in.
        bf16x8 pf[2];
        float rsum = 0.f;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            u32x4 cw = {};
            if constexpr (DROPOUT) cw = *(const u32x4*)&Cw[cb * 16 + lg * 4];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const float e = exp2f(fmaf(sc[cb][x], scale2, -mnew));
                float ek = e;
                if constexpr (DROPOUT) ek = drop_keep_words(drop_rw, cw[x], drop_thr) ? e : 0.f;
                pf[cb >> 1][(cb & 1) * 4 + x] = (__bf16)ek;
                rsum += e;
            }
        }
        l_run = l_run * alpha + rsum;
        // exact skip: alpha is 1.0f wherever the running max did not move
        if (!__all(alpha == 1.0f)) {
#pragma unroll
            for (int dc = 0; dc < DCH; ++dc) o_acc[dc] *= alpha;
        }

        // --- O^T += V^T*P^T: B = packed P (registers), A via the pipelined
        // tr16 ladder over the row-major V image (issue frag i+1,
        // counted-wait frag i, MFMA — LDS latency hides under the matrix
        // pipe). The K reads above were consumed by the score MFMAs, so no
        // LDS op is outstanding when the ladder opens. ---
        // depth-3 pipeline: two fragments stay in flight — ONE MFMA
        // (~17 cyc) does not cover the ~50-cycle LDS read latency that
        // depth-2 exposed at every counted wait
        tr16_ladder<3, 2 * DCH>(
            aV0c, aV1c, [](int i) { return ((i / DCH) * 32 * SK + (i % DCH) * 16) * 2; },
            [&](auto i, bf16x8 vf) {
                constexpr int kc2 = decltype(i)::value / DCH, dc = decltype(i)::value % DCH;
                o_acc[dc] = MFMA16(vf, pf[kc2], o_acc[dc]);
            });
    };

    for (int kt = 0; kt < ntiles; ++kt) {
        stage_direct(kt * 64, Klds, Vlds);
        if constexpr (DROPOUT) {
            if (__builtin_amdgcn_readfirstlane(threadIdx.x) < 64)
                Cw[lane] = drop_col_word(drop_hw, (uint32_t)(s0 + kt * 64 + lane));
        }
        __syncthreads();
        compute_tile(Klds, aV0, aV1, kt * 64);
        __syncthreads();  // K/V LDS reused next tile
    }

    // --- epilogue: join the row's 4 partial sums, normalize, store O^T
    // (4 contiguous head-dim elements per lane and block) and LSE ---
    const float l_row = qgroup_reduce_sum(l_run);
    float inv_l = (l_row > 0.f) ? 1.f / l_row : 0.f;
    if constexpr (DROPOUT) inv_l *= drop_rp;  // kept P scaled by 1/(1-p)
    if (lg == 0 && qvalid)
        lse[(int64_t)h * T_total + s0 + qrow] = (m_run + log2f(l_row)) * DOL_LN2;
    __bf16* orow = o + (int64_t)(s0 + (qvalid ? qrow : 0)) * o_ts + (int64_t)h * D;
    fa_store_rowT_bf16<DCH>(orow, o_acc, inv_l, qvalid, D, lg);
}

// One causal-attention problem over the row spans [seq_begin[b], seq_end[b]),
// as the six fa_varlen_* / fa_spans_* entry points receive it, in the order
// the backward ones list it. The forward leaves dout .. dv_acc and do_ts
// empty, the backward leaves o empty; lse is written by the forward and read
// by the backward. The varlen entry points (back-to-back sequences) fill
// (cu_seqlens, cu_seqlens + 1) and no p_drop (0: always valid).
struct FaProblem {
    dolomite_stream_t stream;
    const void *q, *k, *v;
    void* o;
    const void* dout;
    float* lse;
    const float* delta;
    void* dqkv_q;
    float *dk_acc, *dv_acc;
    const int32_t *seq_begin, *seq_end;
    int batch, max_seqlen;
    int64_t T;
    int H, Hkv, D, G;
    int64_t q_ts, q_gs, k_ts, k_hs, v_ts, v_hs, do_ts;
    float scale;
    int dtype;
    float p_drop;
    uint64_t seed;
    bool gaps;  // rows outside every span may exist (the fa_spans_* entry points)
};

// The entry points' argument checks, in their order of precedence; only the
// forward checks the scale (its row max is taken before scaling).
static int fa_check_args(const FaProblem& p, bool fwd) {
    if (!drop_p_valid(p.p_drop)) return 9013;  // p_drop outside [0, 1) (NaN included)
    if (p.dtype != DOLOMITE_BF16) return 9010;  // bf16 only (north-star dtype)
    if (p.D > 128) return 9011;
    if (fwd && !(p.scale > 0.f)) return 9015;
    return 0;
}

// launch(integral_constant DPAD, bool_constant DROPOUT): the head dim rounded
// up to a kernel instantiation; p_drop == 0 runs the DROPOUT=false ones (the
// dropout-free code).
template <typename Launch>
static int fa_select_kernel(const FaProblem& p, Launch launch) {
    auto by_dpad = [&](auto drop) {
        if (p.D <= 32) return launch(std::integral_constant<int, 32>{}, drop);
        if (p.D <= 64) return launch(std::integral_constant<int, 64>{}, drop);
        if (p.D <= 96) return launch(std::integral_constant<int, 96>{}, drop);
        return launch(std::integral_constant<int, 128>{}, drop);
    };
    return p.p_drop > 0.f ? by_dpad(std::true_type{}) : by_dpad(std::false_type{});
}

// grid.x = tiles of the longest sequence; shorter sequences' surplus
// workgroups exit on the span-length check.
static dim3 fa_grid(const FaProblem& p) { return dim3((p.max_seqlen + 127) / 128, p.batch, p.H); }

template <int DPAD, bool DROPOUT>
static int launch_fa_fwd(const FaProblem& p) {
    hipLaunchKernelGGL((fa_fwd_kernel<DPAD, DROPOUT>), fa_grid(p), dim3(512), FaKvLds<DPAD>::bytes(DROPOUT),
                       (hipStream_t)p.stream, (const __bf16*)p.q, (const __bf16*)p.k, (const __bf16*)p.v,
                       (__bf16*)p.o, p.lse, p.seq_begin, p.seq_end, p.H, p.Hkv, p.D, p.G,
                       p.q_ts, p.q_gs, p.k_ts, p.k_hs, p.v_ts, p.v_hs, (int64_t)p.H * p.D, p.T, p.scale,
                       (uint32_t)p.seed, (uint32_t)(p.seed >> 32), drop_threshold(p.p_drop),
                       1.f / (1.f - p.p_drop));
    return dol_last_error();
}

// shared by every forward entry point
static int fa_spans_fwd_dispatch(const FaProblem& p) {
    int err = fa_check_args(p, true);
    if (err) return err;
    if (p.gaps) {
        // o's gap rows (disjoint from every row the attention kernel stores)
        err = dolomite_fa_zero_gap_rows(p.stream, p.o, (int64_t)p.H * p.D * (int64_t)sizeof(__bf16),
                                        p.seq_begin, p.seq_end, p.batch, p.T);
        if (err) return err;
        if (p.batch == 0 || p.max_seqlen <= 0) return 0;  // every row is a gap row
    }
    return fa_select_kernel(p, [&](auto dpad, auto drop) {
        return launch_fa_fwd<decltype(dpad)::value, decltype(drop)::value>(p);
    });
}

extern "C" int dolomite_fa_varlen_fwd(dolomite_stream_t stream,
                                      const void* q, const void* k, const void* v,
                                      void* o, float* lse,
                                      const int32_t* cu_seqlens, int batch, int max_seqlen, int64_t T,
                                      int H, int Hkv, int D, int G,
                                      int64_t q_tstride, int64_t q_gstride,
                                      int64_t k_tstride, int64_t k_hstride,
                                      int64_t v_tstride, int64_t v_hstride,
                                      float scale, int dtype) {
    return fa_spans_fwd_dispatch({stream, q, k, v, o, nullptr, lse, nullptr, nullptr, nullptr, nullptr,
                                  cu_seqlens, cu_seqlens + 1, batch, max_seqlen, T, H, Hkv, D, G,
                                  q_tstride, q_gstride, k_tstride, k_hstride, v_tstride, v_hstride, 0,
                                  scale, dtype, 0.f, 0, false});
}

extern "C" int dolomite_fa_varlen_fwd_dropout(dolomite_stream_t stream,
                                              const void* q, const void* k, const void* v,
                                              void* o, float* lse,
                                              const int32_t* cu_seqlens, int batch, int max_seqlen, int64_t T,
                                              int H, int Hkv, int D, int G,
                                              int64_t q_tstride, int64_t q_gstride,
                                              int64_t k_tstride, int64_t k_hstride,
                                              int64_t v_tstride, int64_t v_hstride,
                                              float scale, int dtype, float p_drop, uint64_t seed) {
    return fa_spans_fwd_dispatch({stream, q, k, v, o, nullptr, lse, nullptr, nullptr, nullptr, nullptr,
                                  cu_seqlens, cu_seqlens + 1, batch, max_seqlen, T, H, Hkv, D, G,
                                  q_tstride, q_gstride, k_tstride, k_hstride, v_tstride, v_hstride, 0,
                                  scale, dtype, p_drop, seed, false});
}

// ===========================================================================
// Backward pass 1: delta[h,t] = sum_d dO[t,h,d] * O[t,h,d]   (one wave/row)
// ===========================================================================

template <typename T>
__global__ void __launch_bounds__(256) fa_bwd_preprocess_kernel(
    const T* __restrict__ o, const T* __restrict__ dout, float* __restrict__ delta,
    int64_t T_total, int H, int D, int64_t o_ts, int64_t do_ts) {
    int64_t row = ((int64_t)blockIdx.x * 4) + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (row >= T_total * H) return;
    int64_t t = row / H;
    int h = (int)(row % H);
    const T* op = o + t * o_ts + (int64_t)h * D;
    const T* dp = dout + t * do_ts + (int64_t)h * D;
    float acc = 0.f;
    // element pairs per lane: coalesced 4-byte loads instead of scalar b16
    for (int d = lane * 2; d + 1 < D; d += 128) {
        float o0[2], d0[2];
        VecIO<T, 2>::load(op + d, o0);
        VecIO<T, 2>::load(dp + d, d0);
        acc += o0[0] * d0[0] + o0[1] * d0[1];
    }
    if (D & 1) {  // odd head dim tail (not on any named config)
        int d = D - 1;
        if (lane == 0) acc += load_as_f32(op + d) * load_as_f32(dp + d);
    }
    acc = wave_reduce_sum(acc);
    if (lane == 0) delta[(int64_t)h * T_total + t] = acc;
}

// Fast path for the contiguous bf16 layout (every named config): the
// one-wave-per-(t,h) kernel above issues only two b32 loads per lane for an
// 80-element row — far too shallow to cover HBM latency (measured 0.36 ms
// vs 0.11 ms algorithmic). Here a block streams a TOK-token tile with b128
// loads (8-element groups never cross a head boundary since D % 8 == 0),
// parks one fp32 partial dot per group in LDS, then one thread per (t, h)
// slot sums its D/8 contiguous partials in FIXED ascending order — the
// reduction stays bit-deterministic for the resume tests.
__global__ void __launch_bounds__(256) fa_bwd_preprocess_tiled(
    const __bf16* __restrict__ o, const __bf16* __restrict__ dout, float* __restrict__ delta,
    int64_t T_total, int H, int D, int TOK) {
    extern __shared__ float part[];  // [TOK*H*D/8]
    const int64_t hd = (int64_t)H * D;
    const int64_t base = (int64_t)blockIdx.x * TOK * hd;
    const int64_t total = T_total * hd;
    const int np = (int)(TOK * hd / 8);
#pragma unroll 4
    for (int p = threadIdx.x; p < np; p += 256) {
        int64_t flat = base + (int64_t)p * 8;
        float acc = 0.f;
        if (flat + 8 <= total) {
            bf16x8 ov = *(const bf16x8*)(o + flat);
            bf16x8 dv = *(const bf16x8*)(dout + flat);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc += (float)ov[e] * (float)dv[e];
        }
        part[p] = acc;
    }
    __syncthreads();
    const int slots = TOK * H;
    const int dp8 = D / 8;
    for (int s = threadIdx.x; s < slots; s += 256) {
        float a = 0.f;
        const float* ps = &part[s * dp8];
        for (int i = 0; i < dp8; ++i) a += ps[i];
        int tl = s / H, h = s - tl * H;
        int64_t t = (int64_t)blockIdx.x * TOK + tl;
        if (t < T_total) delta[(int64_t)h * T_total + t] = a;
    }
}

extern "C" int dolomite_fa_bwd_preprocess(dolomite_stream_t stream,
                                          const void* o, const void* dout, float* delta,
                                          int64_t T, int H, int D,
                                          int64_t o_tstride, int64_t do_tstride, int dtype) {
    const int64_t hd = (int64_t)H * D;
    int TOK = 16;
    while (TOK > 1 && TOK * hd * 4 / 8 > 65536) TOK /= 2;  // LDS partial budget
    if (dtype == DOLOMITE_BF16 && D % 8 == 0 && o_tstride == hd && do_tstride == hd && T > 0 &&
        TOK * hd * 4 / 8 <= 65536) {
        dim3 grid((uint32_t)((T + TOK - 1) / TOK)), block(256);
        size_t shmem = (size_t)(TOK * hd / 8) * sizeof(float);
        hipLaunchKernelGGL((fa_bwd_preprocess_tiled), grid, block, shmem, (hipStream_t)stream,
                           (const __bf16*)o, (const __bf16*)dout, delta, T, H, D, TOK);
        return dol_last_error();
    }
    int64_t rows = T * H;
    dim3 grid((uint32_t)((rows + 3) / 4)), block(256);
    if (dtype == DOLOMITE_BF16)
        hipLaunchKernelGGL((fa_bwd_preprocess_kernel<uint16_t>), grid, block, 0, (hipStream_t)stream,
                           (const uint16_t*)o, (const uint16_t*)dout, delta, T, H, D, o_tstride, do_tstride);
    else
        hipLaunchKernelGGL((fa_bwd_preprocess_kernel<float>), grid, block, 0, (hipStream_t)stream,
                           (const float*)o, (const float*)dout, delta, T, H, D, o_tstride, do_tstride);
    return dol_last_error();
}

// ===========================================================================
// Backward pass 2: per (kv-tile, seq, kv-head) workgroup.
// ===========================================================================

// Backward is split FA2-style into two kernels (each recomputes P from
// q/k/lse — cheaper than the atomics+barriers a fused version needs):
//   fa_bwd_dkv_kernel : grid (kv-tile, seq, q-head); dK/dV accumulate in
//     registers over the q-tile loop and are stored once into per-q-head
//     fp32 partials (G q-head contributors per kv strip, reduced in fixed
//     order by fa_grad_finalize).
//   fa_bwd_dq_kernel  : grid (q-tile, seq, q-head); dQ^T accumulates in
//     registers over the kv-tile loop — no atomics at all — and is stored
//     once. Row-major K and V images, staged per kv tile; dS stays in
//     registers (see "Swapped-operand score tiles").

// dkv structure: the key on the lane, P and dS in registers. A wave owns 16
// keys of the workgroup's 128-key strip and holds their K / V rows as
// register fragments for the whole kernel; the Q / dO tile (64 queries) is
// staged as two row-major LDS images in natural row order (stride DPAD+16,
// the fwd / dq geometry), read two ways:
//   - S = Q*K^T and dP = dO*V^T: the image row is the A operand (b128 row
//     reads), the K / V register fragment the B operand (the A and B lane
//     maps are symmetric), so C block cb holds, on lane l reg x,
//       key  l & 15            query  16*cb + 4*(l>>4) + x;
//   - the 8 values of query blocks (2c, 2c+1) pack, with no lane movement
//     and no LDS, into the B operand of dV^T += dO^T*P and dK^T += Q^T*dS
//     over a 32-query chunk. Element e on lane group g is query
//     32c + 16*(e>>2) + 4g + (e&3); the A operands are tr16 reads of the
//     same images in that order (fa_tr16_perm_bases, as the fwd / dq
//     ladders do for keys). One chunk at a time: 4 + 4 packed registers
//     of P / dS are live, then that chunk's 2*DCH ladder MFMAs.
// The per-query lse and delta (and, with dropout, the row words of the keep
// mask) are staged once per tile into 64-entry LDS arrays by one wave each:
// a lane needs 4 consecutive query rows per block and the packed row offset
// s0 is arbitrary, so the global rows are only 4-byte aligned, while the LDS
// arrays are tile-relative and read as one b128 (broadcast over the 16 lanes
// of a group). Rows >= L are staged as 0 and masked. -delta is the INITIAL
// accumulator of the dP chain (no dropout), and the softmax scale of dS is
// applied once to dK at the store.
// Outputs come out transposed (head-dim 16*dc + 4g + x on the registers, key
// on l & 15): one 16-byte non-temporal store per lane, block and buffer.
// __launch_bounds__(512, 4) (<= 128 VGPR) gives 2 workgroups/CU at
// DPAD <= 96: while one workgroup stages Q/dO from HBM the co-resident one
// runs its MFMA segments. DPAD = 128 keeps the looser bound of its parent.
// Dropout (DROPOUT=true): the P fragment feeding dV holds M ? P : 0 and dV is
// scaled by rp = 1/(1-p) once at the store; dS uses the UNDROPPED P with the
// masked, scaled dP: dS = P * ((M ? dP*rp : 0) - delta) * scale (delta =
// rowsum(dO*O) already equals sum_j P_ij * dP_ij under dropout). The lane's
// key is fixed -> one hoisted column word; 4 row words per block from LDS.

// P = 2^(s*scale*log2e - lse*log2e) as ONE v_exp_f32: exp2f() wraps the
// instruction in a 5-instruction rescale so that results below 2^-126 come
// out as denormals; such a probability is 0 in every product it enters here,
// and the bare instruction returns exactly that. The issue-bound softmax
// body drops from ~10 to ~5 VALU instructions per score.
__device__ __forceinline__ float dkv_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

template <int DPAD>
struct FaDkvLds {
    static constexpr int S = FaKvLds<DPAD>::S;  // the fwd / dq image stride
    static constexpr size_t image_bytes = (size_t)2 * 64 * S * sizeof(__bf16);  // multiple of 256
    static constexpr size_t bytes(bool dropout) {
        return image_bytes + 2 * 64 * sizeof(float) + (dropout ? 64 * sizeof(uint32_t) : 0);
    }
};

template <int DPAD, bool DROPOUT>
__global__ void __launch_bounds__(512, DPAD <= 96 ? 4 : 2) fa_bwd_dkv_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    const __bf16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    float* __restrict__ dk_acc, float* __restrict__ dv_acc,
    const int32_t* __restrict__ seq_begin, const int32_t* __restrict__ seq_end,
    int H, int Hkv, int D, int G,
    int64_t q_ts, int64_t q_gs, int64_t k_ts, int64_t k_hs, int64_t v_ts, int64_t v_hs,
    int64_t do_ts, int64_t T_total, float scale,
    uint32_t seed_lo, uint32_t seed_hi, uint32_t drop_thr, float drop_rp) {
    constexpr int KCH = DPAD / 32;
    constexpr int DCH = DPAD / 16;

    int tile_id = blockIdx.x, b = blockIdx.y, h = blockIdx.z;
    xcd_remap_tile_bh(tile_id, b, h);
    const int kvh = h / G;
    // span-derived values are wave-uniform: pin them to SGPRs so per-lane
    // address arithmetic built on them does not hold VGPR pairs across the
    // main loop (measured: the compiler otherwise spills pointer pairs)
    const int s0 = __builtin_amdgcn_readfirstlane(seq_begin[b]);
    const int L = __builtin_amdgcn_readfirstlane(seq_end[b]) - s0;
    // 8 waves x 16 keys = 128-key strip per workgroup
    const int ks = tile_id * 128;
    if (ks >= L) return;

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lr = lane & 15;
    const int lg = lane >> 4;

    constexpr int SQ = FaDkvLds<DPAD>::S;      // image stride
    extern __shared__ char smem_raw[];         // FaDkvLds<DPAD>::bytes(DROPOUT)
    __bf16* Qlds = (__bf16*)smem_raw;          // [64 q][SQ]
    __bf16* dOl = Qlds + 64 * SQ;              // [64 q][SQ]
    float* Lsel = (float*)(dOl + 64 * SQ);     // [64 q] lse * log2(e)
    float* NDel = Lsel + 64;                   // [64 q] -delta
    uint32_t* Rw = (uint32_t*)(NDel + 64);     // [64 q] row words (DROPOUT only)

    const int kend = min(L, ks + 128);

    // this wave's K and V fragments (B-layout of K^T / V^T: j = lr -> key)
    const int krow = ks + wave * 16 + lr;
    const bool kvalid = krow < kend;
    bf16x8 kfr[KCH], vfr[KCH];
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc) {
        int d0 = kc * 32 + lg * 8;
        const __bf16* kp = k + (int64_t)(s0 + (kvalid ? krow : 0)) * k_ts + (int64_t)kvh * k_hs + d0;
        kfr[kc] = load_bf16x8_guard(kp, d0, D, kvalid);
        const __bf16* vp = v + (int64_t)(s0 + (kvalid ? krow : 0)) * v_ts + (int64_t)kvh * v_hs + d0;
        vfr[kc] = load_bf16x8_guard(vp, d0, D, kvalid);
    }

    f32x4 dvr[DCH], dkr[DCH];
#pragma unroll
    for (int dc = 0; dc < DCH; ++dc) {
        dvr[dc] = {0.f, 0.f, 0.f, 0.f};
        dkr[dc] = {0.f, 0.f, 0.f, 0.f};
    }

    // dropout: a lane owns ONE key for the whole kernel, so its column word
    // is hoisted; the tile's 64 row words are mixed once per workgroup (Rw)
    uint32_t drop_cw = 0;
    if constexpr (DROPOUT)
        drop_cw = drop_col_word(drop_head_word(seed_hi, (uint32_t)h), (uint32_t)(s0 + krow));

    // lane base addresses for the dK^T/dV^T tr16 ladders (permuted query
    // order). One pair serves both images: dOl sits 64*SQ elements above
    // Qlds, a displacement that fits the 16-bit ds_read immediate.
    unsigned aQ0, aQ1;
    fa_tr16_perm_bases(Qlds, SQ, lane, aQ0, aQ1);
    constexpr int DO_IMM = 64 * SQ * 2;        // dOl = Qlds + this (bytes)
    static_assert(DO_IMM + 32 * SQ * 2 + DPAD * 2 < 65536, "ds offset range");
    const float scale2 = scale * DOL_LOG2E;

    // T5 static priority (guide §5.5): the later-dispatched half of an
    // 8-wave workgroup loses VALU arbitration to the older half; one
    // setprio(1) for that half removes its start-of-segment penalty.
    // The guard must be provably wave-uniform (readfirstlane) or s_setprio
    // is emitted unconditionally.
    if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256) __builtin_amdgcn_s_setprio(1);

    const int qt0 = ks / 64;
    const int nqt = (L + 63) / 64;
    const int64_t q_hoff = (int64_t)(h / G) * q_gs + (int64_t)(h % G) * D;
    const int64_t do_hoff = (int64_t)h * D;

    if (D < DPAD) {
        for (int pidx = threadIdx.x; pidx < 64 * (DPAD - D) / 8; pidx += 512) {
            int qq = pidx / ((DPAD - D) / 8);
            int d0 = D + (pidx % ((DPAD - D) / 8)) * 8;
            bf16x8 z = {};
            *(bf16x8*)&Qlds[qq * SQ + d0] = z;
            *(bf16x8*)&dOl[qq * SQ + d0] = z;
        }
    }

    // One 32-query chunk c of the staged tile. Per 16-query block: S = Q*K^T
    // and dP = dO*V^T MFMAs (element x is key = krow, query = qs + 16*cb +
    // 4*lg + x), then that block's P and dS packed into half of the chunk's
    // fragments — one C-pair live. Then dV^T += dO^T*P and dK^T += Q^T*dS
    // through ONE depth-3 tr16 ladder over the dO image and then the Q
    // image; the image and statistics reads above were consumed by the
    // score MFMAs / the softmax, so no LDS op is outstanding when it opens.
    auto dkv_chunk = [&](auto cc, const int qs, const int full) {
        constexpr int c = decltype(cc)::value;
        bf16x8 pf, dsf;
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
            const int cb = 2 * c + hb;
            // -delta: the dP chain's initial accumulator, or (dropout, where
            // dP is masked first) an addend read after the chain
            f32x4 st = {0.f, 0.f, 0.f, 0.f};
            f32x4 dpt = {0.f, 0.f, 0.f, 0.f};
            if constexpr (!DROPOUT) dpt = *(const f32x4*)&NDel[cb * 16 + lg * 4];
#pragma unroll
            for (int kc = 0; kc < KCH; ++kc) {
                int d0 = kc * 32 + lg * 8;
                bf16x8 qa = *(const bf16x8*)&Qlds[(cb * 16 + lr) * SQ + d0];
                st = MFMA16(qa, kfr[kc], st);
                bf16x8 da = *(const bf16x8*)&dOl[(cb * 16 + lr) * SQ + d0];
                dpt = MFMA16(da, vfr[kc], dpt);
            }
            const f32x4 ls = *(const f32x4*)&Lsel[cb * 16 + lg * 4];
            u32x4 rw = {};
            f32x4 nd = {};
            if constexpr (DROPOUT) {
                rw = *(const u32x4*)&Rw[cb * 16 + lg * 4];
                nd = *(const f32x4*)&NDel[cb * 16 + lg * 4];
            }
            if (full) {
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    float pv = dkv_exp2(fmaf(st[x], scale2, -ls[x]));
                    if constexpr (DROPOUT) {
                        const bool keep = drop_keep_words(rw[x], drop_cw, drop_thr);
                        pf[hb * 4 + x] = (__bf16)(keep ? pv : 0.f);
                        dsf[hb * 4 + x] = (__bf16)(pv * fmaf(keep ? dpt[x] : 0.f, drop_rp, nd[x]));
                    } else {
                        pf[hb * 4 + x] = (__bf16)pv;
                        dsf[hb * 4 + x] = (__bf16)(pv * dpt[x]);
                    }
                }
            } else {
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const int qpos = qs + cb * 16 + lg * 4 + x;
                    const bool ok = kvalid && qpos < L && krow <= qpos;
                    float pv = ok ? dkv_exp2(fmaf(st[x], scale2, -ls[x])) : 0.f;
                    if constexpr (DROPOUT) {
                        const bool keep = drop_keep_words(rw[x], drop_cw, drop_thr);
                        float ds = ok ? pv * fmaf(keep ? dpt[x] : 0.f, drop_rp, nd[x]) : 0.f;
                        pf[hb * 4 + x] = (__bf16)(keep ? pv : 0.f);
                        dsf[hb * 4 + x] = (__bf16)ds;
                    } else {
                        float ds = ok ? pv * dpt[x] : 0.f;
                        pf[hb * 4 + x] = (__bf16)pv;
                        dsf[hb * 4 + x] = (__bf16)ds;
                    }
                }
            }
        }

        // fragments 0 .. DCH-1 walk the dO image (dV), DCH .. 2*DCH-1 the Q
        // image (dK), both from the chunk's 32 image rows at c * 32 * SQ * 2 bytes
        tr16_ladder<3, 2 * DCH>(
            aQ0, aQ1,
            [](int i) { return c * 32 * SQ * 2 + (i / DCH ? 0 : DO_IMM) + (i % DCH) * 32; },
            [&](auto i, bf16x8 af) {
                constexpr int dc = decltype(i)::value % DCH;
                if constexpr (decltype(i)::value / DCH == 0) dvr[dc] = MFMA16(af, pf, dvr[dc]);
                else dkr[dc] = MFMA16(af, dsf, dkr[dc]);
            });
    };

    // (hoisting the staging coordinates like dq/fwd costs 3 scratch
    // pointer reloads per iteration at dkv's 128-VGPR cap and measured
    // slower than recomputing addresses — dkv recomputes, with the
    // runtime division replaced by an exact magic multiply: pidx < 2048
    // and D/8 <= 16, so (pidx * (2^22/(D/8) + 1)) >> 22 is exact)
    const unsigned st_magic = (1u << 22) / (unsigned)(D / 8) + 1;
    for (int qt = qt0; qt < nqt; ++qt) {
        const int qs = qt * 64;
        __syncthreads();  // previous iteration's image reads done
        {
            const int pieces = 64 * DPAD / 8;
            if (qs + 64 <= L) {
                // full interior tile: guard-free staging of the real D cols
                for (int pidx = threadIdx.x; pidx < 64 * D / 8; pidx += 512) {
                    int qq = (int)(((unsigned)pidx * st_magic) >> 22);
                    int d0 = (pidx - qq * (D / 8)) * 8;
                    *(bf16x8*)&Qlds[qq * SQ + d0] =
                        *(const bf16x8*)(q + (int64_t)(s0 + qs + qq) * q_ts + q_hoff + d0);
                    *(bf16x8*)&dOl[qq * SQ + d0] =
                        *(const bf16x8*)(dout + (int64_t)(s0 + qs + qq) * do_ts + do_hoff + d0);
                }
            } else {
                for (int pidx = threadIdx.x; pidx < pieces; pidx += 512) {
                    int qq = pidx / (DPAD / 8);
                    int d0 = (pidx % (DPAD / 8)) * 8;
                    bool valid = (qs + qq) < L;
                    const __bf16* qp = q + (int64_t)(s0 + (valid ? qs + qq : 0)) * q_ts + q_hoff + d0;
                    *(bf16x8*)&Qlds[qq * SQ + d0] = load_bf16x8_guard(qp, d0, D, valid);
                    const __bf16* dp = dout + (int64_t)(s0 + (valid ? qs + qq : 0)) * do_ts + do_hoff + d0;
                    *(bf16x8*)&dOl[qq * SQ + d0] = load_bf16x8_guard(dp, d0, D, valid);
                }
            }
            // the tile's per-query statistics, one wave each; rows >= L are
            // never read from memory and hold 0 (the mask drops them)
            const int swave = __builtin_amdgcn_readfirstlane(wave);
            const bool sok = qs + lane < L;
            const int64_t sidx = (int64_t)h * T_total + s0 + (sok ? qs + lane : 0);
            if (swave == 0) {
                Lsel[lane] = sok ? lse[sidx] * DOL_LOG2E : 0.f;
            } else if (swave == 1) {
                NDel[lane] = sok ? -delta[sidx] : 0.f;
            } else if (swave == 2) {
                if constexpr (DROPOUT) Rw[lane] = drop_row_word(seed_lo, (uint32_t)(s0 + qs + lane));
            }
        }
        __syncthreads();

        // The kernels are ISSUE-bound (SQ counters): the causal-mask
        // compare/select chain runs only on diagonal/edge tiles via a
        // wave-uniform branch: a wave takes the maskless body when its 16
        // keys lie inside the strip, none is above the tile's first query
        // and the 64-query tile is interior (at L = 4096 every tile but
        // the strip's own two diagonal ones).
        const bool full_tile = (ks + wave * 16 + 16 <= qs + 1) && (ks + wave * 16 + 16 <= kend) && (qs + 64 <= L);
        const int full = __builtin_amdgcn_readfirstlane(full_tile ? 1 : 0);
        dkv_chunk(std::integral_constant<int, 0>{}, qs, full);
        dkv_chunk(std::integral_constant<int, 1>{}, qs, full);
    }

    // Deterministic join: each (kv-tile, q-head) workgroup owns its keys'
    // (t, h) slot of the per-head partial buffers exclusively, so dK/dV
    // are plain stores (half the traffic of atomic RMW); fa_grad_finalize
    // reduces the G q-head contributions in a FIXED order. The round-1
    // fp32 atomicAdd join was arrival-order nondeterministic, which made
    // bit-exact checkpoint resume a coin flip.
    // A lane holds 4 consecutive head-dim elements of its key per block: one
    // 16-byte store per buffer (D % 8 == 0, so a group is all inside D or
    // all pad, and every (t, h) row starts 16-byte aligned).
    const int64_t rowoff = ((int64_t)(s0 + (kvalid ? krow : 0)) * H + h) * D;
#pragma unroll
    for (int dc = 0; dc < DCH; ++dc) {
        const int d0 = dc * 16 + lg * 4;
        if (kvalid && d0 < D) {
            // non-temporal: the 1.3 GB of fp32 partials per launch must
            // not evict the XCD-resident Q/dO slices (PMC: dkv read
            // traffic 3.6 GB/launch vs ~1.4 GB ideal with plain stores)
            f32x4 dkv4 = dkr[dc] * scale;
            __builtin_nontemporal_store(dkv4, (f32x4*)&dk_acc[rowoff + d0]);
            f32x4 dvv4 = dvr[dc];
            if constexpr (DROPOUT) dvv4 *= drop_rp;
            __builtin_nontemporal_store(dvv4, (f32x4*)&dv_acc[rowoff + d0]);
        }
    }
}

// Occupancy bound: the dropout-free DPAD=128 variant already sits at the
// 128-VGPR cap (4 spills); the mask words push the DROPOUT one to 10 spills
// under that cap, so it alone takes the looser 1-workgroup/CU bound and
// compiles spill-free. Every other instantiation keeps (512, 4).
template <int DPAD, bool DROPOUT>
__global__ void __launch_bounds__(512, (DROPOUT && DPAD > 96) ? 2 : 4) fa_bwd_dq_kernel(
    const __bf16* __restrict__ q, const __bf16* __restrict__ k, const __bf16* __restrict__ v,
    const __bf16* __restrict__ dout, const float* __restrict__ lse, const float* __restrict__ delta,
    __bf16* __restrict__ dqkv_q,
    const int32_t* __restrict__ seq_begin, const int32_t* __restrict__ seq_end,
    int H, int Hkv, int D, int G,
    int64_t q_ts, int64_t q_gs, int64_t k_ts, int64_t k_hs, int64_t v_ts, int64_t v_hs,
    int64_t do_ts, int64_t T_total, float scale,
    uint32_t seed_lo, uint32_t seed_hi, uint32_t drop_thr, float drop_rp) {
    constexpr int KCH = DPAD / 32;
    constexpr int DCH = DPAD / 16;

    int tile_id = blockIdx.x, b = blockIdx.y, h = blockIdx.z;
    xcd_remap_tile_bh(tile_id, b, h);
    const int kvh = h / G;
    // span-derived values are wave-uniform: pin them to SGPRs so per-lane
    // address arithmetic built on them does not hold VGPR pairs across the
    // main loop (measured: the compiler otherwise spills pointer pairs)
    const int s0 = __builtin_amdgcn_readfirstlane(seq_begin[b]);
    const int L = __builtin_amdgcn_readfirstlane(seq_end[b]) - s0;
    // 8 waves x 16 rows = 128 q rows per workgroup; heaviest tiles first
    const int ntile_seq = (L + 127) / 128;
    if (tile_id >= ntile_seq) return;
    const int qs = (ntile_seq - 1 - tile_id) * 128;

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lr = lane & 15;
    const int lg = lane >> 4;

    // Same orientation as the forward (see "Swapped-operand score tiles"):
    // S^T and dP^T put the q row on the lane, dS^T packs in registers into
    // the B operand of dQ^T = K^T*dS^T, and the K^T A-fragments come from
    // the row-major K image via the permuted-key tr16 ladder. Both images
    // keep natural row order (conflict-free for the b128 row reads, the
    // staging writes and the tr16 reads at stride DPAD+16).
    constexpr int SQ = FaKvLds<DPAD>::S;       // image stride
    extern __shared__ char smem_raw[];         // FaKvLds<DPAD>::bytes(DROPOUT)
    __bf16* Klds = (__bf16*)smem_raw;          // [64 key][SQ]
    __bf16* Vlds = Klds + 64 * SQ;             // [64 key][SQ]
    uint32_t* Cw = (uint32_t*)(Vlds + 64 * SQ);  // [64 key] column words (DROPOUT only)

    const int64_t q_hoff = (int64_t)(h / G) * q_gs + (int64_t)(h % G) * D;
    const int64_t do_hoff = (int64_t)h * D;

    // lane base addresses for the dQ tr16 ladder over Klds
    unsigned aK0, aK1;
    fa_tr16_perm_bases(Klds, SQ, lane, aK0, aK1);

    // this wave's Q and dO fragments (B-layout of Q^T/dO^T: j = lr -> q row)
    const int qrow = qs + wave * 16 + lr;
    const bool qvalid = qrow < L;
    bf16x8 qfr[KCH], dfr[KCH];
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc) {
        int d0 = kc * 32 + lg * 8;
        const __bf16* qp = q + (int64_t)(s0 + (qvalid ? qrow : 0)) * q_ts + q_hoff + d0;
        qfr[kc] = load_bf16x8_guard(qp, d0, D, qvalid);
        const __bf16* dp = dout + (int64_t)(s0 + (qvalid ? qrow : 0)) * do_ts + do_hoff + d0;
        dfr[kc] = load_bf16x8_guard(dp, d0, D, qvalid);
    }

    // one q row per lane: one lse and one delta
    const float lsev = qvalid ? lse[(int64_t)h * T_total + s0 + qrow] * DOL_LOG2E : 0.f;
    const float delv = qvalid ? delta[(int64_t)h * T_total + s0 + qrow] : 0.f;
    const float scale2 = scale * DOL_LOG2E;

    f32x4 dq[DCH];                 // dQ^T: d = dc*16 + lg*4 + x, q = lr
#pragma unroll
    for (int dc = 0; dc < DCH; ++dc) dq[dc] = {0.f, 0.f, 0.f, 0.f};

    // dropout: same dS formula as dkv with the fwd lane mapping (the lane's
    // q row is fixed -> hoisted row word; the tile's 64 column words are
    // mixed once per workgroup into Cw, see the forward)
    uint32_t drop_rw = 0;
    uint32_t drop_hw = 0;
    if constexpr (DROPOUT) {
        drop_hw = drop_head_word(seed_hi, (uint32_t)h);
        drop_rw = drop_row_word(seed_lo, (uint32_t)(s0 + qrow));
    }

    if (D < DPAD) {  // pad columns zeroed once (see dkv note)
        for (int pidx = threadIdx.x; pidx < 64 * (DPAD - D) / 8; pidx += 512) {
            int key = pidx / ((DPAD - D) / 8);
            int d0 = D + (pidx % ((DPAD - D) / 8)) * 8;
            bf16x8 z = {};
            *(bf16x8*)&Klds[key * SQ + d0] = z;
            *(bf16x8*)&Vlds[key * SQ + d0] = z;
        }
    }

    // tile-invariant staging piece coordinates (see dkv note)
    int st_koff[2], st_voff[2];
    int st_klds[2], st_vlds[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        int pidx = (int)threadIdx.x + j * 512;
        int pp = pidx < 64 * D / 8 ? pidx : 0;
        int key = pp / (D / 8);
        int d0 = (pp % (D / 8)) * 8;
        st_koff[j] = (int)(key * k_ts + kvh * k_hs) + d0;   // fits 32 bits
        st_voff[j] = (int)(key * v_ts + kvh * v_hs) + d0;
        st_klds[j] = key * SQ + d0;
        st_vlds[j] = key * SQ + d0;
    }

    const int kend_total = min(L, qs + 128);
    const int nkt = (kend_total + 63) / 64;

    // T5 static priority for the younger workgroup half (see dkv note)
    if (__builtin_amdgcn_readfirstlane(threadIdx.x) >= 256) __builtin_amdgcn_s_setprio(1);

    for (int kt = 0; kt < nkt; ++kt) {
        const int ks = kt * 64;
        __syncthreads();  // previous tile's image reads done
        // stage row-major K + V images, cooperative
        {
            const int pieces = 64 * DPAD / 8;
            if (ks + 64 <= kend_total) {
                const int64_t disp = (int64_t)(s0 + ks);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if ((int)threadIdx.x + j * 512 < 64 * D / 8) {
                        *(bf16x8*)&Klds[st_klds[j]] = *(const bf16x8*)(k + disp * k_ts + st_koff[j]);
                        *(bf16x8*)&Vlds[st_vlds[j]] = *(const bf16x8*)(v + disp * v_ts + st_voff[j]);
                    }
                }
            } else {
                for (int pidx = threadIdx.x; pidx < pieces; pidx += 512) {
                    int key = pidx / (DPAD / 8);
                    int d0 = (pidx % (DPAD / 8)) * 8;
                    bool valid = (ks + key) < kend_total;
                    const __bf16* kp = k + (int64_t)(s0 + (valid ? ks + key : 0)) * k_ts + (int64_t)kvh * k_hs + d0;
                    *(bf16x8*)&Klds[key * SQ + d0] = load_bf16x8_guard(kp, d0, D, valid);
                    const __bf16* vp = v + (int64_t)(s0 + (valid ? ks + key : 0)) * v_ts + (int64_t)kvh * v_hs + d0;
                    *(bf16x8*)&Vlds[key * SQ + d0] = load_bf16x8_guard(vp, d0, D, valid);
                }
            }
        }
        if constexpr (DROPOUT) {
            if (__builtin_amdgcn_readfirstlane(threadIdx.x) < 64)
                Cw[lane] = drop_col_word(drop_hw, (uint32_t)(s0 + ks + lane));
        }
        __syncthreads();

        // Per key block: S^T = K*Q^T and dP^T = V*dO^T MFMAs (element x is
        // q = qrow, key = ks + 16*cb + 4*lg + x), then that block's dS
        // packed into half of its 32-key chunk's fragment — one C-pair live.
        // dsf[c] element e is key 32c + 16*(e>>2) + 4*lg + (e&3), the order
        // the K^T ladder below contracts in.
        // Wave-uniform mask split (see dkv note).
        const bool full_tile = (ks + 64 <= qs + wave * 16 + 1) && (ks + 64 <= kend_total) && (qs + wave * 16 + 16 <= L);
        bf16x8 dsf[2];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            f32x4 sc = {0.f, 0.f, 0.f, 0.f};
            f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KCH; ++kc) {
                int d0 = kc * 32 + lg * 8;
                bf16x8 kb = *(const bf16x8*)&Klds[(cb * 16 + lr) * SQ + d0];
                sc = MFMA16(kb, qfr[kc], sc);
                bf16x8 vb = *(const bf16x8*)&Vlds[(cb * 16 + lr) * SQ + d0];
                dp = MFMA16(vb, dfr[kc], dp);
            }
            u32x4 cw = {};
            if constexpr (DROPOUT) cw = *(const u32x4*)&Cw[cb * 16 + lg * 4];
            if (__builtin_amdgcn_readfirstlane(full_tile ? 1 : 0)) {
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    float pv = exp2f(fmaf(sc[x], scale2, -lsev));
                    float dpm = dp[x];
                    if constexpr (DROPOUT)
                        dpm = drop_keep_words(drop_rw, cw[x], drop_thr) ? dp[x] * drop_rp : 0.f;
                    dsf[cb >> 1][(cb & 1) * 4 + x] = (__bf16)(pv * (dpm - delv) * scale);
                }
            } else {
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const int kpos = ks + cb * 16 + lg * 4 + x;
                    bool ok = qvalid && kpos < kend_total && kpos <= qrow;
                    float pv = ok ? exp2f(fmaf(sc[x], scale2, -lsev)) : 0.f;
                    float dpm = dp[x];
                    if constexpr (DROPOUT)
                        dpm = drop_keep_words(drop_rw, cw[x], drop_thr) ? dp[x] * drop_rp : 0.f;
                    float ds = ok ? pv * (dpm - delv) * scale : 0.f;
                    dsf[cb >> 1][(cb & 1) * 4 + x] = (__bf16)ds;
                }
            }
        }

        // dQ^T += K^T*dS^T (contraction over this tile's keys) — pipelined
        // tr16 ladder over the K image; the image reads above were consumed
        // by the score MFMAs, so no LDS op is outstanding when it opens.
        // Hand-expanded on the shared primitives, not tr16_ladder<4, N>: on
        // the template the six DPAD >= 64 instantiations compiled to other
        // prologues (dq<96, false> +2 VGPRs) and one missed the A/B
        // (profiles/attn_shared_ab_bench.txt).
        {
            __builtin_amdgcn_sched_barrier(0);
            // depth-4 rotation: 3 fragments in flight per wait (the dq cap
            // has ~16 VGPR of headroom the dkv cap does not)
            bf16x4 klo[4], khi[4];
            tr16_issue<0>(aK0, aK1, klo[0], khi[0]);
            tr16_issue<((1 / DCH) * 32 * SQ + (1 % DCH) * 16) * 2>(aK0, aK1, klo[1], khi[1]);
            tr16_issue<((2 / DCH) * 32 * SQ + (2 % DCH) * 16) * 2>(aK0, aK1, klo[2], khi[2]);
#define DQ_STEP(i)                                                                                      \
    if constexpr ((i) < 2 * DCH) {                                                                      \
        constexpr int kc2_ = (i) / DCH, dc_ = (i) % DCH;                                                \
        if constexpr ((i) + 3 < 2 * DCH) {                                                              \
            constexpr int kn_ = ((i) + 3) / DCH, dn_ = ((i) + 3) % DCH;                                 \
            tr16_issue<(kn_ * 32 * SQ + dn_ * 16) * 2>(aK0, aK1, klo[((i) + 3) % 4], khi[((i) + 3) % 4]); \
            lgkm_wait2<6>(klo[(i) % 4], khi[(i) % 4]);                                                  \
        } else if constexpr ((i) + 2 < 2 * DCH) {                                                       \
            lgkm_wait2<4>(klo[(i) % 4], khi[(i) % 4]);                                                  \
        } else if constexpr ((i) + 1 < 2 * DCH) {                                                       \
            lgkm_wait2<2>(klo[(i) % 4], khi[(i) % 4]);                                                  \
        } else {                                                                                        \
            lgkm_wait2<0>(klo[(i) % 4], khi[(i) % 4]);                                                  \
        }                                                                                               \
        dq[dc_] = MFMA16(tr16_join8(klo[(i) % 4], khi[(i) % 4]), dsf[kc2_], dq[dc_]);                   \
    }
            DQ_STEP(0) DQ_STEP(1) DQ_STEP(2) DQ_STEP(3)
            DQ_STEP(4) DQ_STEP(5) DQ_STEP(6) DQ_STEP(7)
            DQ_STEP(8) DQ_STEP(9) DQ_STEP(10) DQ_STEP(11)
            DQ_STEP(12) DQ_STEP(13) DQ_STEP(14) DQ_STEP(15)
#undef DQ_STEP
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // single bf16 store of the accumulated dQ^T straight into the packed
    // dqkv (each (t, h, d) is owned by exactly one q-tile workgroup)
    __bf16* dqrow = dqkv_q + (int64_t)(s0 + (qvalid ? qrow : 0)) * q_ts + q_hoff;
    fa_store_rowT_bf16<DCH>(dqrow, dq, 1.f, qvalid, D, lg);
}

template <int DPAD, bool DROPOUT>
static int launch_fa_bwd(const FaProblem& p) {
    const dim3 grid = fa_grid(p), block(512);
    const hipStream_t stream = (hipStream_t)p.stream;
    const __bf16 *q = (const __bf16*)p.q, *k = (const __bf16*)p.k, *v = (const __bf16*)p.v;
    const __bf16* dout = (const __bf16*)p.dout;
    const uint32_t seed_lo = (uint32_t)p.seed, seed_hi = (uint32_t)(p.seed >> 32);
    const uint32_t thr = drop_threshold(p.p_drop);
    const float rp = 1.f / (1.f - p.p_drop);
    hipLaunchKernelGGL((fa_bwd_dkv_kernel<DPAD, DROPOUT>), grid, block, FaDkvLds<DPAD>::bytes(DROPOUT), stream,
                       q, k, v, dout, p.lse, p.delta, p.dk_acc, p.dv_acc, p.seq_begin, p.seq_end,
                       p.H, p.Hkv, p.D, p.G, p.q_ts, p.q_gs, p.k_ts, p.k_hs, p.v_ts, p.v_hs, p.do_ts,
                       p.T, p.scale, seed_lo, seed_hi, thr, rp);
    int err = dol_last_error();
    if (err) return err;
    hipLaunchKernelGGL((fa_bwd_dq_kernel<DPAD, DROPOUT>), grid, block, FaKvLds<DPAD>::bytes(DROPOUT), stream,
                       q, k, v, dout, p.lse, p.delta, (__bf16*)p.dqkv_q, p.seq_begin, p.seq_end,
                       p.H, p.Hkv, p.D, p.G, p.q_ts, p.q_gs, p.k_ts, p.k_hs, p.v_ts, p.v_hs, p.do_ts,
                       p.T, p.scale, seed_lo, seed_hi, thr, rp);
    return dol_last_error();
}

// shared by every backward entry point
static int fa_spans_bwd_dispatch(const FaProblem& p) {
    int err = fa_check_args(p, false);
    if (err) return err;
    if (p.gaps && (p.batch == 0 || p.max_seqlen <= 0)) return 0;  // every row is a gap row
    return fa_select_kernel(p, [&](auto dpad, auto drop) {
        return launch_fa_bwd<decltype(dpad)::value, decltype(drop)::value>(p);
    });
}

extern "C" int dolomite_fa_varlen_bwd(dolomite_stream_t stream,
                                      const void* q, const void* k, const void* v,
                                      const void* dout, const float* lse,
                                      const float* delta, void* dqkv_q, float* dk_acc, float* dv_acc,
                                      const int32_t* cu_seqlens, int batch, int max_seqlen, int64_t T,
                                      int H, int Hkv, int D, int G,
                                      int64_t q_tstride, int64_t q_gstride,
                                      int64_t k_tstride, int64_t k_hstride,
                                      int64_t v_tstride, int64_t v_hstride,
                                      int64_t do_tstride,
                                      float scale, int dtype) {
    return fa_spans_bwd_dispatch({stream, q, k, v, nullptr, dout, const_cast<float*>(lse), delta, dqkv_q,
                                  dk_acc, dv_acc, cu_seqlens, cu_seqlens + 1, batch, max_seqlen, T,
                                  H, Hkv, D, G, q_tstride, q_gstride, k_tstride, k_hstride,
                                  v_tstride, v_hstride, do_tstride, scale, dtype, 0.f, 0, false});
}

extern "C" int dolomite_fa_varlen_bwd_dropout(dolomite_stream_t stream,
                                              const void* q, const void* k, const void* v,
                                              const void* dout, const float* lse,
                                              const float* delta, void* dqkv_q, float* dk_acc, float* dv_acc,
                                              const int32_t* cu_seqlens, int batch, int max_seqlen, int64_t T,
                                              int H, int Hkv, int D, int G,
                                              int64_t q_tstride, int64_t q_gstride,
                                              int64_t k_tstride, int64_t k_hstride,
                                              int64_t v_tstride, int64_t v_hstride,
                                              int64_t do_tstride,
                                              float scale, int dtype, float p_drop, uint64_t seed) {
    return fa_spans_bwd_dispatch({stream, q, k, v, nullptr, dout, const_cast<float*>(lse), delta, dqkv_q,
                                  dk_acc, dv_acc, cu_seqlens, cu_seqlens + 1, batch, max_seqlen, T,
                                  H, Hkv, D, G, q_tstride, q_gstride, k_tstride, k_hstride,
                                  v_tstride, v_hstride, do_tstride, scale, dtype, p_drop, seed, false});
}

// ===========================================================================
// Span entry points: sequences that are not back to back (a padded (B, S)
// batch viewed as B*S rows). The attention kernels only ever touch rows
// inside a span, so the rows between spans ("gap rows") are zeroed by a
// kernel of their own — whole-buffer memsets would cost more than the
// attention at the bench shape (1.3 GB of fp32 partials per launch).
// ===========================================================================

// Gap g of batch+1: rows [seq_end[g-1], seq_begin[g]) with seq_end[-1] = 0
// and seq_begin[batch] = T. grid (chunks, batch+1); each gap is a contiguous
// byte range (rows are contiguous), cleared with 16-byte stores in a
// grid-stride loop. Both bounds are clamped into [0, T] and an inverted pair
// is an empty range, so spans that break the precondition cannot push a
// store outside the buffer.
__global__ void __launch_bounds__(256) fa_zero_gap_rows_kernel(
    uint4* __restrict__ buf, int64_t row_vec,
    const int32_t* __restrict__ seq_begin, const int32_t* __restrict__ seq_end,
    int batch, int64_t T) {
    const int g = blockIdx.y;
    int64_t lo = g == 0 ? 0 : (int64_t)seq_end[g - 1];
    int64_t hi = g == batch ? T : (int64_t)seq_begin[g];
    lo = lo < 0 ? 0 : lo;
    hi = hi > T ? T : hi;
    if (hi <= lo) return;
    const int64_t first = lo * row_vec, last = hi * row_vec;   // 16-byte units
    const uint4 z = {0u, 0u, 0u, 0u};
    for (int64_t i = first + (int64_t)blockIdx.x * 256 + threadIdx.x; i < last;
         i += (int64_t)gridDim.x * 256)
        buf[i] = z;
}

extern "C" int dolomite_fa_zero_gap_rows(dolomite_stream_t stream, void* buf, int64_t row_bytes,
                                         const int32_t* seq_begin, const int32_t* seq_end,
                                         int batch, int64_t T) {
    if (row_bytes <= 0 || row_bytes % 16 != 0) return 9016;
    if (batch < 0 || T < 0 || batch >= 65535) return 9014;
    if (T == 0) return 0;
    // sized for the average gap if every row were a gap row (4 stores per
    // thread); longer gaps take more trips of the grid-stride loop
    const int64_t vec_per_gap = (T * (row_bytes / 16) + batch) / (batch + 1);
    int64_t chunks = (vec_per_gap + 1023) / 1024;
    chunks = chunks < 1 ? 1 : (chunks > 1024 ? 1024 : chunks);
    hipLaunchKernelGGL(fa_zero_gap_rows_kernel, dim3((uint32_t)chunks, (uint32_t)(batch + 1)),
                       dim3(256), 0, (hipStream_t)stream, (uint4*)buf, row_bytes / 16,
                       seq_begin, seq_end, batch, T);
    return dol_last_error();
}

extern "C" int dolomite_fa_spans_fwd(dolomite_stream_t stream,
                                     const void* q, const void* k, const void* v,
                                     void* o, float* lse,
                                     const int32_t* seq_begin, const int32_t* seq_end,
                                     int batch, int max_seqlen, int64_t T,
                                     int H, int Hkv, int D, int G,
                                     int64_t q_tstride, int64_t q_gstride,
                                     int64_t k_tstride, int64_t k_hstride,
                                     int64_t v_tstride, int64_t v_hstride,
                                     float scale, int dtype, float p_drop, uint64_t seed) {
    return fa_spans_fwd_dispatch({stream, q, k, v, o, nullptr, lse, nullptr, nullptr, nullptr, nullptr,
                                  seq_begin, seq_end, batch, max_seqlen, T, H, Hkv, D, G,
                                  q_tstride, q_gstride, k_tstride, k_hstride, v_tstride, v_hstride, 0,
                                  scale, dtype, p_drop, seed, true});
}

extern "C" int dolomite_fa_spans_bwd(dolomite_stream_t stream,
                                     const void* q, const void* k, const void* v,
                                     const void* dout, const float* lse,
                                     const float* delta, void* dqkv_q, float* dk_acc, float* dv_acc,
                                     const int32_t* seq_begin, const int32_t* seq_end,
                                     int batch, int max_seqlen, int64_t T,
                                     int H, int Hkv, int D, int G,
                                     int64_t q_tstride, int64_t q_gstride,
                                     int64_t k_tstride, int64_t k_hstride,
                                     int64_t v_tstride, int64_t v_hstride,
                                     int64_t do_tstride,
                                     float scale, int dtype, float p_drop, uint64_t seed) {
    return fa_spans_bwd_dispatch({stream, q, k, v, nullptr, dout, const_cast<float*>(lse), delta, dqkv_q,
                                  dk_acc, dv_acc, seq_begin, seq_end, batch, max_seqlen, T,
                                  H, Hkv, D, G, q_tstride, q_gstride, k_tstride, k_hstride,
                                  v_tstride, v_hstride, do_tstride, scale, dtype, p_drop, seed, true});
}

// Keep-mask probe: out[(h*nq + i)*nk + j] = keep(seed, h, tq0+i, tk0+j) as
// 0/1 bytes, through the same device function the attention kernels use
// (the host compares against the Python restatement bit for bit).
__global__ void __launch_bounds__(256) fa_dropout_mask_probe_kernel(
    uint8_t* __restrict__ out, uint32_t seed_lo, uint32_t seed_hi, uint32_t thr,
    int64_t total, int64_t tq0, int nq, int64_t tk0, int nk) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int j = (int)(idx % nk);
    const int64_t hi = idx / nk;
    const int i = (int)(hi % nq);
    const uint32_t h = (uint32_t)(hi / nq);
    out[idx] = drop_keep(seed_lo, seed_hi, h, (uint32_t)(tq0 + i), (uint32_t)(tk0 + j), thr) ? 1 : 0;
}

extern "C" int dolomite_fa_dropout_mask_probe(dolomite_stream_t stream, uint8_t* out,
                                              uint64_t seed, float p_drop, int H,
                                              int64_t tq0, int nq, int64_t tk0, int nk) {
    if (!drop_p_valid(p_drop)) return 9013;
    if (H < 0 || nq < 0 || nk < 0) return 9014;
    const int64_t total = (int64_t)H * nq * nk;
    if (total == 0) return 0;
    const int64_t nblocks = (total + 255) / 256;
    if (nblocks > 0x7fffffff) return 9014;
    hipLaunchKernelGGL(fa_dropout_mask_probe_kernel, dim3((uint32_t)nblocks), dim3(256), 0,
                       (hipStream_t)stream, out, (uint32_t)seed, (uint32_t)(seed >> 32),
                       drop_threshold(p_drop), total, tq0, nq, tk0, nk);
    return dol_last_error();
}

// ===========================================================================
// Backward pass 3: cast dq/dk/dv fp32 accumulators into the packed dqkv.
// ===========================================================================

// Reduce the (T, H, D) per-q-head fp32 partials over each kv head's G
// contributors in fixed order and cast into the packed dqkv. One thread
// per FOUR d-columns (D % 4 == 0 on this path): float4 streaming loads —
// the scalar version sat at 95% wave-wait on load latency.
template <typename T>
__global__ void __launch_bounds__(256) fa_grad_finalize_kernel(
    const float* __restrict__ dk_acc, const float* __restrict__ dv_acc,
    T* __restrict__ dqkv, int64_t total_kv,
    int Hkv, int D, int G, int64_t row_ts, int64_t k_off, int64_t kv_hs, int64_t v_off) {
    int64_t quad = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // 4-elem groups
    int64_t total_q4 = total_kv / 4;
    bool is_v = quad >= total_q4;
    if (is_v) quad -= total_q4;
    if (quad >= total_q4) return;
    int64_t kidx = quad * 4;
    int64_t t = kidx / ((int64_t)Hkv * D);
    int rem = (int)(kidx % ((int64_t)Hkv * D));
    int j = rem / D;
    int d = rem % D;
    const float* src = is_v ? dv_acc : dk_acc;
    int64_t base = ((t * Hkv + j) * (int64_t)G) * D + d;
    f4_t acc = {0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < G; ++g) {
        f4_t v4 = __builtin_nontemporal_load((const f4_t*)&src[base + (int64_t)g * D]);
        acc += v4;
    }
    T* out = &dqkv[t * row_ts + (is_v ? v_off : k_off) + (int64_t)j * kv_hs + d];
#pragma unroll
    for (int e = 0; e < 4; ++e) store_from_f32(out + e, acc[e]);
}

extern "C" int dolomite_fa_grad_finalize(dolomite_stream_t stream,
                                         const float* dk_acc, const float* dv_acc,
                                         void* dqkv, int64_t T, int Hkv, int D, int G,
                                         int64_t row_tstride,
                                         int64_t k_off, int64_t kv_hstride, int64_t v_off, int dtype) {
    int64_t total_kv = T * (int64_t)Hkv * D;
    if (D % 4 != 0) return 9012;  // D % 8 == 0 on every supported path
    int64_t total = 2 * (total_kv / 4);
    if (total == 0) return 0;
    dim3 grid((uint32_t)((total + 255) / 256)), block(256);
    if (dtype == DOLOMITE_BF16)
        hipLaunchKernelGGL((fa_grad_finalize_kernel<uint16_t>), grid, block, 0, (hipStream_t)stream,
                           dk_acc, dv_acc, (uint16_t*)dqkv, total_kv,
                           Hkv, D, G, row_tstride, k_off, kv_hstride, v_off);
    else
        hipLaunchKernelGGL((fa_grad_finalize_kernel<float>), grid, block, 0, (hipStream_t)stream,
                           dk_acc, dv_acc, (float*)dqkv, total_kv,
                           Hkv, D, G, row_tstride, k_off, kv_hstride, v_off);
    return dol_last_error();
}

// ===========================================================================
// MFMA fragment-layout self-test (see header comment).
// ===========================================================================

// ds_read_b64_tr_b16 semantics probe: LDS holds bf16 values = element index
// (0..255, exact in bf16). Each variant issues the transpose-read with a
// different per-lane address convention; the host inspects which elements
// landed in which lane/slot to pin the gather pattern (guide T10 says
// lane l elem j <- lds[(l&15) + j*16 + (l>>4)*64] but is not a spec).
typedef __bf16 bf16x4p __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(64) tr16_probe_kernel(float* out) {
    __shared__ __bf16 s[256];
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 256; i += 64) s[i] = (__bf16)(float)i;
    __syncthreads();
    const unsigned base = (unsigned)(size_t)(__bf16*)s;  // LDS byte address of s[0]
    unsigned addrs[3] = {
        base + (unsigned)((lane >> 4) * 128),                        // group base only
        base + (unsigned)(lane * 8),                                 // lane-linear b64
        base + (unsigned)(((lane & 15) * 2) + ((lane >> 4) * 128)),  // +column offset
    };
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        bf16x4p r;
        asm volatile("ds_read_b64_tr_b16 %0, %1\n\ts_waitcnt lgkmcnt(0)"
                     : "=v"(r)
                     : "v"(addrs[v])
                     : "memory");
#pragma unroll
        for (int j = 0; j < 4; ++j) out[(v * 64 + lane) * 4 + j] = (float)r[j];
    }
}

extern "C" int dolomite_tr16_probe(dolomite_stream_t stream, float* out) {
    hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out);
    return dol_last_error();
}

// End-to-end check of lds_tr16_bfrag under kernel conditions (dynamic LDS,
// PI23-staged row-major image): src is a row-major [64][cols] bf16 matrix;
// out[l][e] (float) = the B-fragment element e lane l received for the
// chunk (rowbase, d0). Host asserts out[l][e] == src[rowbase+(l>>4)*8+e][d0+(l&15)].
__global__ void __launch_bounds__(64) tr16_bfrag_probe_kernel(
    const __bf16* src, float* out, int cols, int S, int rowbase, int d0) {
    extern __shared__ char smem_raw[];
    __bf16* img = (__bf16*)smem_raw;
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 64 * (cols / 8); i += 64) {
        int row = i / (cols / 8), c8 = (i % (cols / 8)) * 8;
        *(bf16x8*)&img[PI23(row) * S + c8] = *(const bf16x8*)&src[row * cols + c8];
    }
    __syncthreads();
    bf16x8 f = lds_tr16_bfrag(img, rowbase, S, d0, lane);
#pragma unroll
    for (int e = 0; e < 8; ++e) out[lane * 8 + e] = (float)f[e];
}

extern "C" int dolomite_tr16_bfrag_probe(dolomite_stream_t stream, const void* src, float* out,
                                         int cols, int S, int rowbase, int d0) {
    size_t shmem = (size_t)64 * S * sizeof(__bf16);
    hipLaunchKernelGGL(tr16_bfrag_probe_kernel, dim3(1), dim3(64), shmem, (hipStream_t)stream,
                       (const __bf16*)src, out, cols, S, rowbase, d0);
    return dol_last_error();
}

__global__ void __launch_bounds__(64) mfma_probe_kernel(const __bf16* A, const __bf16* B, float* C) {
    int lane = threadIdx.x & 63;
    int lr = lane & 15, lg = lane >> 4;
    bf16x8 a, b;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        a[e] = A[lr * 32 + lg * 8 + e];      // A[i][k], i=lr, k=lg*8+e
        b[e] = B[(lg * 8 + e) * 16 + lr];    // B[k][j], k=lg*8+e, j=lr
    }
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    c = MFMA16(a, b, c);
#pragma unroll
    for (int r = 0; r < 4; ++r) C[(lg * 4 + r) * 16 + lr] = c[r];
}

extern "C" int dolomite_mfma_probe(dolomite_stream_t stream, const void* A, const void* B, float* C) {
    hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream,
                       (const __bf16*)A, (const __bf16*)B, C);
    return dol_last_error();
}
