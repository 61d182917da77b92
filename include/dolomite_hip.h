/* dolomite_hip — C-ABI boundary of the MI355X HIP kernel library.
 *
 * These entry points are the gfx950-native replacements for the GPU work the
 * reference delegates to third-party kernels (SURVEY.md §2 "Delegated
 * kernel" table). Each declaration cites the reference call site
 * (paths under /root/reference/dolomite_engine/) it replaces.
 *
 * Conventions:
 *   - caller (the Python host on PyTorch-ROCm) owns all memory; pointers are
 *     device pointers; strides/sizes are in ELEMENTS (not bytes) as int64;
 *   - `stream` is the hipStream_t the call is ordered on (passed as void*);
 *   - dtype codes: 0 = fp32, 1 = bf16;
 *   - return 0 on success, nonzero hipError_t-style code on failure;
 *   - thread-safe per stream; no internal allocation on the hot path.
 */

#ifndef DOLOMITE_HIP_H
#define DOLOMITE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dolomite_stream_t; /* hipStream_t */

enum dolomite_dtype { DOLOMITE_F32 = 0, DOLOMITE_BF16 = 1 };

/* Library/version probe (used by the loader to verify ABI). */
int dolomite_hip_abi_version(void);

/* ------------------------------------------------------------------------
 * Fused RMSNorm (+ optional residual add), forward / backward.
 * Replaces: Triton RMSNorm (modeling_utils/normalization/rmsnorm/torchtitan.py)
 * with the canonical semantics of rmsnorm/base.py:18-25:
 *   s     = x + res_in            (when res_in != NULL; else s = x)
 *   rstd  = rsqrt(mean(s_fp32^2) + eps)
 *   y     = w * cast_to_input_dtype(s_fp32 * rstd)
 * res_out (when non-NULL) receives s (the pre-norm sum, used as the next
 * residual). rstd is cached fp32 per row for backward.
 * x,y,res_*: (T, H) row-major contiguous, dtype `dtype`. w: (H,), dtype.
 * ---------------------------------------------------------------------- */
int dolomite_rmsnorm_fwd(dolomite_stream_t stream,
                         const void* x, const void* res_in, const void* w,
                         void* y, void* res_out, float* rstd,
                         int64_t T, int64_t H, float eps, int dtype);

/* Backward: given dy and the saved pre-norm input s (= res_out of fwd, or x
 * when no residual) and rstd, computes
 *   dx  = r*(w*dy - s_hat * mean(w*dy*s_hat)) [+ dres_in]  (s_hat = s_fp32*rstd;
 *         dres_in, when non-NULL, is the residual-stream gradient folded into
 *         dx in the same pass instead of a separate elementwise add)
 *   dw  = sum_rows(dy * cast_to_dtype(s_hat))        (fp32 accumulation)
 * dw_partial: (nblocks, H) fp32 scratch written by the kernel;
 * dolomite_reduce_partials sums it into dw (H,) fp32 in a fixed order, so
 * dw (and LayerNorm's db) are bitwise reproducible.
 * Error 9002 (returned before anything is launched): H too wide for one
 * wave to hold a row in registers — H > 8192 for bf16 with H % 8 == 0,
 * H > 4096 for fp32 with H % 4 == 0, H > 1024 for any other H. Holds for
 * all four norm entry points (rmsnorm/layernorm, fwd/bwd).
 * nblocks is returned by dolomite_rmsnorm_bwd_nblocks(T). */
int dolomite_rmsnorm_bwd_nblocks(int64_t T);
int dolomite_rmsnorm_bwd(dolomite_stream_t stream,
                         const void* dy, const void* s, const void* w,
                         const float* rstd, void* dx, float* dw_partial,
                         const void* dres_in, int64_t T, int64_t H, int dtype);

/* LayerNorm, same calling pattern (replaces the reference 'layernorm'/'torch'
 * nn.LayerNorm path; mean/rstd cached fp32). db shares dw_partial layout:
 * dw_partial holds (2*nblocks, H): [dw partials ; db partials]. */
int dolomite_layernorm_fwd(dolomite_stream_t stream,
                           const void* x, const void* res_in, const void* w, const void* b,
                           void* y, void* res_out, float* mean, float* rstd,
                           int64_t T, int64_t H, float eps, int dtype);
int dolomite_layernorm_bwd(dolomite_stream_t stream,
                           const void* dy, const void* s, const void* w,
                           const float* mean, const float* rstd,
                           void* dx, float* dwdb_partial,
                           const void* dres_in, int64_t T, int64_t H, int dtype);

/* Sum partials: out[h] = sum_i partial[i*H + h]; out fp32 (H,), need not be
 * zeroed. The summation order is FIXED (no atomics), so the result is
 * bitwise reproducible run to run:
 *   nsplit = min(32, ceil(nblocks / 128)),  chunk = ceil(nblocks / nsplit)
 *   s_c[h] = ((0 + partial[i0,h]) + partial[i0+1,h]) + ...   for rows
 *            i0 = c*chunk .. min(i0 + chunk, nblocks) - 1, ascending
 *   out[h] = ((0 + s_0[h]) + s_1[h]) + ... + s_{nsplit-1}[h], ascending c
 * all in fp32; for nsplit == 1, out = s_0. The Python restatement is
 * ops/functional.py reduce_partials_ref.
 * `partial` is SCRATCH despite the const the signature keeps (the C ABI is
 * unchanged): it must be mutable memory, and for nsplit > 1 the call
 * overwrites row c*chunk with s_c (the other rows are left as they were).
 * No other memory is used. */
int dolomite_reduce_partials(dolomite_stream_t stream,
                             const float* partial, float* out,
                             int64_t nblocks, int64_t H);

/* ------------------------------------------------------------------------
 * RoPE on the packed QKV projection output, forward / backward.
 * Replaces apply_rotary_pos_emb (position_embedding/rope.py:104-121) at the
 * call site attention/padding_free.py:38-40, operating IN PLACE of the
 * fused c_attn layout (attention/base.py:72-81) without unpacking:
 *   qkv: (T, row_len) where row q-head h lives at
 *        (h/G)*q_gstride + (h%G)*D  and kv-head j at k_off + j*kv_hstride
 *        (v is untouched). G = n_head/num_kv_heads heads per kv group.
 *   cos/sin: (T, D) fp32, already gathered per token position
 *        (gpt_dolomite/base.py:289-296).
 *   dir: +1 forward rotation, -1 inverse (exact backward, since the table
 *        halves are duplicated: R^T = -R and S commutes with R).
 * in == out: in place. out != in: only the q and k slots of qkv_out are
 * written; its v slots are NOT copied from qkv_in and keep what they held
 * (rotate_v_copy is reserved and ignored) — the caller copies v if it needs
 * a complete row. Error 9003: odd D.
 * ---------------------------------------------------------------------- */
int dolomite_rope_qkv(dolomite_stream_t stream,
                      const void* qkv_in, void* qkv_out,
                      const float* cos_t, const float* sin_t,
                      int64_t T, int64_t row_len,
                      int H, int Hkv, int D, int G,
                      int64_t q_gstride, int64_t k_off, int64_t kv_hstride,
                      int dir, int rotate_v_copy, int dtype);

/* ------------------------------------------------------------------------
 * Varlen causal flash attention, forward.
 * Replaces flash_attn_varlen_func (attention/padding_free.py:51-62).
 * q/k/v address layout (strides in elements):
 *   q[t, h, d]  = q_ptr + t*q_tstride + (h/G)*q_gstride + (h%G)*D + d
 *   k[t, j, d]  = k_ptr + t*k_tstride + j*k_hstride + d
 *   v[t, j, d]  = v_ptr + t*v_tstride + j*v_hstride + d
 * (this addresses the packed c_attn output without copies for MHA/GQA/MQA)
 * o: (T, H*D) row-major contiguous bf16/fp32; lse: (H, T) fp32 log-sum-exp
 * (natural log, includes softmax scale), for backward.
 * cu_seqlens: (batch+1,) int32 device pointer; causal only. Attention
 * dropout: the *_dropout entry points below.
 * Error codes: 9010 dtype != bf16, 9011 D > 128, 9015 scale not > 0 (the
 * forward takes each row's max on the unscaled scores).
 * ---------------------------------------------------------------------- */
int dolomite_fa_varlen_fwd(dolomite_stream_t stream,
                           const void* q, const void* k, const void* v,
                           void* o, float* lse,
                           const int32_t* cu_seqlens, int batch, int max_seqlen, int64_t T,
                           int H, int Hkv, int D, int G,
                           int64_t q_tstride, int64_t q_gstride,
                           int64_t k_tstride, int64_t k_hstride,
                           int64_t v_tstride, int64_t v_hstride,
                           float scale, int dtype);

/* Backward, three passes (all launched by the host in order on `stream`):
 *  1. preprocess: delta[h,t] = rowsum(dO[t,h,:]*O[t,h,:]) fp32.
 *  2. main: dkv — one workgroup per (kv-tile, seq, q-head); recomputes P
 *     from q,k,lse; dk/dv accumulate in registers over the q-tile loop and
 *     store EXCLUSIVELY (no atomics) into (T, H, D) fp32 per-q-head
 *     partials. dq — one workgroup per (q-tile, seq, q-head),
 *     register-accumulated and stored bf16 directly into the packed dqkv
 *     q-slots.
 *  3. grad_finalize: reduces each kv head's G partial contributions in
 *     FIXED order (deterministic gradients — bit-exact resume depends on
 *     it) and casts into the packed dqkv.
 */
int dolomite_fa_bwd_preprocess(dolomite_stream_t stream,
                               const void* o, const void* dout, float* delta,
                               int64_t T, int H, int D,
                               int64_t o_tstride, int64_t do_tstride, int dtype);
int dolomite_fa_varlen_bwd(dolomite_stream_t stream,
                           const void* q, const void* k, const void* v,
                           const void* dout, const float* lse,
                           const float* delta, void* dqkv_q, float* dk_acc, float* dv_acc,
                           const int32_t* cu_seqlens, int batch, int max_seqlen, int64_t T,
                           int H, int Hkv, int D, int G,
                           int64_t q_tstride, int64_t q_gstride,
                           int64_t k_tstride, int64_t k_hstride,
                           int64_t v_tstride, int64_t v_hstride,
                           int64_t do_tstride,
                           float scale, int dtype);
/* dk_acc/dv_acc are (T, H, D) fp32 PER-Q-HEAD partials written exclusively
 * (no atomics) by dolomite_fa_varlen_bwd; the finalize reduces each kv
 * head's G contributors in fixed order — deterministic gradients. */
int dolomite_fa_grad_finalize(dolomite_stream_t stream,
                              const float* dk_acc, const float* dv_acc,
                              void* dqkv, int64_t T, int Hkv, int D, int G,
                              int64_t row_tstride,
                              int64_t k_off, int64_t kv_hstride, int64_t v_off, int dtype);

/* ------------------------------------------------------------------------
 * Attention dropout (flash_attn_varlen_func's dropout_p, forwarded by the
 * reference at attention/padding_free.py:49-59), fused into the kernels.
 *
 * Keep-mask: a pure counter-based function, never written to memory — the
 * forward and both backward kernels regenerate it. All arithmetic is
 * unsigned 32-bit (wrapping):
 *   mix(x):  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;
 *            x *= 0x846CA68B;  x ^= x >> 16
 *   seed_lo = seed & 0xFFFFFFFF,  seed_hi = seed >> 32
 *   rw = mix(seed_lo ^ (t_q * 0x9E3779B1))                  per-row word
 *   hw = mix(seed_hi ^ (h   * 0xC2B2AE3D))                  per-head word
 *   cw = mix(hw      ^ (t_k * 0x85EBCA77))                  per-column word
 *   x  = rw ^ cw;  x ^= x >> 16;  x *= 0x7FEB352D;  x ^= x >> 15;
 *   x *= 0x846CA68B                      (mix without its last xorshift)
 *   keep(seed, h, t_q, t_k, p) = x >= floor(p * 2^32)
 * h is the q-head; t_q / t_k are GLOBAL packed token indices
 * (cu_seqlens[b] + position, low 32 bits), so the mask depends neither on
 * tile geometry nor on which kernel asks. p is the IEEE float32 p_drop
 * (floor(p * 2^32) is exact in double). Kept probabilities are scaled by
 * 1/(1-p) (float32); lse is the UNDROPPED log-sum-exp. The Python
 * restatement is ops/functional.py attention_dropout_keep_mask.
 *
 * Same argument lists and error codes as dolomite_fa_varlen_fwd / _bwd,
 * plus (p_drop, seed); error 9013 for p_drop outside [0, 1) (NaN included).
 * p_drop == 0 runs exactly the dropout-free kernels. The backward must get
 * the p_drop and seed of its forward; preprocess and grad_finalize are
 * unchanged (delta = rowsum(dO*O) holds under dropout).
 * ---------------------------------------------------------------------- */
int dolomite_fa_varlen_fwd_dropout(dolomite_stream_t stream,
                                   const void* q, const void* k, const void* v,
                                   void* o, float* lse,
                                   const int32_t* cu_seqlens, int batch, int max_seqlen, int64_t T,
                                   int H, int Hkv, int D, int G,
                                   int64_t q_tstride, int64_t q_gstride,
                                   int64_t k_tstride, int64_t k_hstride,
                                   int64_t v_tstride, int64_t v_hstride,
                                   float scale, int dtype, float p_drop, uint64_t seed);
int dolomite_fa_varlen_bwd_dropout(dolomite_stream_t stream,
                                   const void* q, const void* k, const void* v,
                                   const void* dout, const float* lse,
                                   const float* delta, void* dqkv_q, float* dk_acc, float* dv_acc,
                                   const int32_t* cu_seqlens, int batch, int max_seqlen, int64_t T,
                                   int H, int Hkv, int D, int G,
                                   int64_t q_tstride, int64_t q_gstride,
                                   int64_t k_tstride, int64_t k_hstride,
                                   int64_t v_tstride, int64_t v_hstride,
                                   int64_t do_tstride,
                                   float scale, int dtype, float p_drop, uint64_t seed);

/* ------------------------------------------------------------------------
 * Span attention: the same kernels over sequences that are NOT back to back.
 * Replaces the reference's dense flash path (attention/flash.py: unpad by the
 * mask, flash_attn_varlen_func, pad_input) without the unpad / pad copies: a
 * padded (B, S, row_len) batch viewed as (B*S, row_len) is the packed layout
 * with sequence b on rows [seq_begin[b], seq_end[b]).
 *
 * seq_begin, seq_end: (batch,) int32 device pointers. Precondition:
 *   0 <= seq_begin[b] <= seq_end[b] <= T, spans ascending and disjoint
 *   (seq_end[b] <= seq_begin[b+1]); empty spans are allowed.
 * max_seqlen: the longest span. (cu_seqlens, cu_seqlens + 1) is the
 * back-to-back special case the varlen entry points pass.
 * Rows outside every span ("gap rows": [seq_end[b-1], seq_begin[b]) with
 * seq_end[-1] = 0 and seq_begin[batch] = T):
 *   - dolomite_fa_spans_fwd leaves o exactly zero there (pad_input's
 *     semantics); lse is unspecified there.
 *   - dolomite_fa_spans_bwd writes nothing there (dqkv_q, dk_acc, dv_acc);
 *     dolomite_fa_grad_finalize then reduces whatever the partials hold on
 *     those rows, so the host runs dolomite_fa_zero_gap_rows on dqkv AFTER
 *     the finalize: q, k and v slots of every gap row end exactly zero.
 *   - delta from dolomite_fa_bwd_preprocess is unspecified there and never
 *     read.
 * Dropout: t_q / t_k of the keep-mask stay the GLOBAL row indices of the
 * buffer (b*S + position for a padded batch). p_drop == 0 runs the
 * dropout-free kernels. The other arguments and the error codes are those of
 * dolomite_fa_varlen_fwd_dropout / _bwd_dropout.
 * ---------------------------------------------------------------------- */
int dolomite_fa_spans_fwd(dolomite_stream_t stream,
                          const void* q, const void* k, const void* v,
                          void* o, float* lse,
                          const int32_t* seq_begin, const int32_t* seq_end,
                          int batch, int max_seqlen, int64_t T,
                          int H, int Hkv, int D, int G,
                          int64_t q_tstride, int64_t q_gstride,
                          int64_t k_tstride, int64_t k_hstride,
                          int64_t v_tstride, int64_t v_hstride,
                          float scale, int dtype, float p_drop, uint64_t seed);
int dolomite_fa_spans_bwd(dolomite_stream_t stream,
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
                          float scale, int dtype, float p_drop, uint64_t seed);
/* Zero the gap rows of a (T, row_bytes) row-major buffer, touching no span
 * row. buf must be 16-byte aligned; error 9016 if row_bytes is not a
 * positive multiple of 16, 9014 for batch < 0 or T < 0. */
int dolomite_fa_zero_gap_rows(dolomite_stream_t stream, void* buf, int64_t row_bytes,
                              const int32_t* seq_begin, const int32_t* seq_end,
                              int batch, int64_t T);

/* Keep-mask probe: out[(h*nq + i)*nk + j] = keep(seed, h, tq0+i, tk0+j, p_drop)
 * as 0/1 bytes for h in [0, H), through the device function the attention
 * kernels use. out: (H, nq, nk) uint8 device pointer. Errors: 9013 as above,
 * 9014 for a negative or oversized box. */
int dolomite_fa_dropout_mask_probe(dolomite_stream_t stream, uint8_t* out,
                                   uint64_t seed, float p_drop, int H,
                                   int64_t tq0, int nq, int64_t tk0, int nk);

/* ------------------------------------------------------------------------
 * KV cache and single-token decode attention (inference; the reference's
 * dense flash path with a cache, attention/flash.py:42-43 and the
 * query_length == 1 branch at :94-100). bf16 here; the e4m3 cache has entry
 * points of its own below (dolomite_kv_cache_append_fp8 / dolomite_fa_decode_fp8).
 *
 * Cache layout, shared by both entry points (elements):
 *   k_cache[b, s, j, d] = k_cache + b*bstride + s*tstride + j*hstride + d
 * and the same strides for v_cache; the natural allocation is a contiguous
 * (B, S_cap, Hkv, D) bf16 tensor each. The cache is never cleared: positions
 * at and beyond a sequence's length hold whatever the allocation held.
 *
 * dolomite_kv_cache_append copies the K and V slots of packed (RoPE'd) qkv
 * rows into the cache: row src_begin[b] + i, for i in
 * [0, src_end[b] - src_begin[b]), goes to cache position dst_pos[b] + i of
 * sequence b. A position >= S_cap (or < 0) is skipped, never written;
 * nothing outside the named positions is touched. One kernel serves the
 * prefill (the span arrays of dolomite_fa_spans_fwd, dst_pos = 0) and the
 * decode step (one row per sequence).
 *   qkv: (T, row_tstride) rows; K head j of a row at k_off + j*kv_hstride,
 *     V head j at v_off + j*kv_hstride (the QKVLayout strides).
 *   src_begin, src_end, dst_pos: (batch,) int32 device pointers,
 *     0 <= src_begin[b] <= src_end[b] <= T.
 *   max_rows: an upper bound on src_end[b] - src_begin[b] (grid sizing;
 *     rows beyond it are not copied).
 * 16-byte loads and stores: D and every stride / offset must be multiples
 * of 8 elements and the pointers 16-byte aligned.
 * Error codes: 9010 dtype != bf16, 9030 negative size (batch, max_rows,
 * S_cap), Hkv <= 0 or batch > 65535, 9031 D or a stride not a positive
 * multiple of 8.
 * ---------------------------------------------------------------------- */
int dolomite_kv_cache_append(dolomite_stream_t stream, const void* qkv,
                             const int32_t* src_begin, const int32_t* src_end,
                             const int32_t* dst_pos, void* k_cache, void* v_cache,
                             int batch, int max_rows, int Hkv, int D, int S_cap,
                             int64_t row_tstride, int64_t k_off, int64_t v_off, int64_t kv_hstride,
                             int64_t cache_bstride, int64_t cache_tstride, int64_t cache_hstride,
                             int dtype);

/* dolomite_fa_decode: one query token per sequence against the cache.
 *   q[b, h, d] = q + b*q_tstride + (h/G)*q_gstride + (h%G)*D + d  (the new
 *     token's packed row, one row per sequence)
 *   cache_len: (batch,) int32 device pointer, the number of valid keys of
 *     each sequence INCLUDING the new token (the append has already run).
 *     Values are clamped into [0, max_len].
 *   max_len: an upper bound on cache_len, <= the cache capacity.
 *   o: (batch, H*D) bf16 row-major contiguous.
 * There is no causal mask: the key range [0, cache_len[b]) is the mask.
 * Keys at and beyond cache_len[b] never influence the result, whatever
 * that memory holds (NaN and Inf included). cache_len[b] == 0 gives an
 * all-(+0) output row.
 *
 * Split-KV: the grid is (nsplit, batch, Hkv) — Hkv * ceil(G / 32) for
 * G > 32. Split c owns keys [c*chunk, min((c+1)*chunk, cache_len[b])) with
 * chunk = ceil(max_len / nsplit) rounded up to the 64-key tile; a split
 * with no keys is legal and contributes nothing. The G query heads of a kv
 * head share one pass over its K/V. With nsplit > 1 each workgroup stores
 * fp32 partials (unnormalised O, row max, row sum) exclusively into
 * `scratch` and a second kernel combines them in ascending split order: no
 * atomics, bitwise reproducible for fixed arguments. The result for
 * different nsplit differs by fp32 rounding of the join.
 *   scratch: dolomite_fa_decode_scratch_floats(batch, H, D, nsplit) floats,
 *     16-byte aligned, caller-owned (0 and may be NULL for nsplit == 1;
 *     the query returns -1 for invalid arguments). nsplit == 1 stores o
 *     directly.
 * Error codes: 9010 dtype != bf16, 9011 D > 128, 9015 scale not > 0, 9031
 * D not a positive multiple of 8, 9032 negative / inconsistent sizes
 * (H != Hkv*G included), 9033 nsplit < 1 or a grid dimension over 65535,
 * 9034 nsplit > 1 without scratch.
 * ---------------------------------------------------------------------- */
int64_t dolomite_fa_decode_scratch_floats(int batch, int H, int D, int nsplit);
int dolomite_fa_decode(dolomite_stream_t stream,
                       const void* q, const void* k_cache, const void* v_cache, void* o,
                       float* scratch, const int32_t* cache_len,
                       int batch, int H, int Hkv, int D, int G,
                       int max_len, int nsplit,
                       int64_t q_tstride, int64_t q_gstride,
                       int64_t k_bstride, int64_t k_tstride, int64_t k_hstride,
                       int64_t v_bstride, int64_t v_tstride, int64_t v_hstride,
                       float scale, int dtype);

/* ------------------------------------------------------------------------
 * fp8 KV cache: the cache halves its bytes and a decode step its HBM read.
 *   k_cache / v_cache: OCP e4m3 bytes (torch.float8_e4m3fn), addressed like
 *     the bf16 cache with strides in elements (= bytes), unit stride on d.
 *   k_scale / v_scale: fp32, one per (sequence, kv head, position):
 *     scale[b, j, s] = scale + b*scale_bstride + j*scale_hstride + s, the
 *     natural allocation a contiguous (B, Hkv, S_cap) tensor each.
 * Quantisation rule of one (position, kv head) slice x of D bf16 values, all
 * arithmetic in fp32 (IEEE division, one rounding per operation):
 *   a = max(max_d |x[d]|, 2^-64), scale = a / 448, inv = 448 / a,
 *   q[d] = e4m3 round-to-nearest-even of x[d] * inv;   x[d] ~ q[d] * scale.
 * An all-zero slice quantises to zeros. NaN / Inf in x: unspecified.
 *
 * dolomite_kv_cache_append_fp8: dolomite_kv_cache_append's arguments and
 * semantics (spans, dst_pos, max_rows — rows at and beyond it are not
 * appended —, positions outside [0, S_cap) skipped, nothing else written in
 * the cache or the scales), quantising on the way. qkv is bf16 (`dtype`).
 * Deterministic. 16-byte loads and 8-byte stores: D and every stride /
 * offset but the scale strides in units of 8 elements.
 * Error codes: 9010 dtype != bf16, 9030 negative size, Hkv <= 0,
 * batch > 65535 or more than 2^31 lane slots per sequence, 9031 D or a
 * stride not a positive multiple of 8, or D > 128.
 *
 * dolomite_fa_decode_fp8: dolomite_fa_decode over such a cache — the same
 * grid, key split, partials, scratch (dolomite_fa_decode_scratch_floats) and
 * ascending-order combine; q and o are bf16 (`dtype`). The K scale multiplies
 * the fp32 score, the V scale the softmax weight before it is packed to bf16;
 * the row sum is of the unscaled weights. Keys at and beyond cache_len[b]
 * never influence the result whatever bytes and scales they hold, and
 * nothing at or beyond position max_len is read, for any capacity.
 * Error codes: dolomite_fa_decode's, and 9031 also for a cache stride that is
 * not a multiple of 8.
 * ---------------------------------------------------------------------- */
int dolomite_kv_cache_append_fp8(dolomite_stream_t stream, const void* qkv,
                                 const int32_t* src_begin, const int32_t* src_end,
                                 const int32_t* dst_pos, void* k_cache, void* v_cache,
                                 float* k_scale, float* v_scale,
                                 int batch, int max_rows, int Hkv, int D, int S_cap,
                                 int64_t row_tstride, int64_t k_off, int64_t v_off, int64_t kv_hstride,
                                 int64_t cache_bstride, int64_t cache_tstride, int64_t cache_hstride,
                                 int64_t scale_bstride, int64_t scale_hstride, int dtype);
int dolomite_fa_decode_fp8(dolomite_stream_t stream,
                           const void* q, const void* k_cache, const void* v_cache,
                           const float* k_scale, const float* v_scale, void* o,
                           float* scratch, const int32_t* cache_len,
                           int batch, int H, int Hkv, int D, int G,
                           int max_len, int nsplit,
                           int64_t q_tstride, int64_t q_gstride,
                           int64_t k_bstride, int64_t k_tstride, int64_t k_hstride,
                           int64_t v_bstride, int64_t v_tstride, int64_t v_hstride,
                           int64_t scale_bstride, int64_t scale_hstride,
                           float scale, int dtype);

/* dolomite_fa_extend: n_b >= 0 new query tokens per sequence against the
 * cache, causally (a continued conversation, a chunk of a chunked prefill,
 * the verify pass over draft tokens). The new tokens are rows
 * [seq_begin[b], seq_end[b]) of the packed qkv (T rows), n_b of them, and
 * the cache ALREADY holds their K/V (the append has run with
 * dst_pos = cache_len - n_b). With past_b = cache_len[b] - n_b, query i
 * attends keys [0, past_b + i + 1): the bottom-right-aligned causal mask.
 *   q[t, h, d] = qkv + t*q_tstride + (h/G)*q_gstride + (h%G)*D + d
 *   seq_begin, seq_end: (batch,) int32 device pointers, ascending and
 *     disjoint, 0 <= seq_begin[b] <= seq_end[b] <= T.
 *   max_new: an upper bound on n_b (grid sizing; queries beyond it are not
 *     computed).
 *   cache_len: (batch,) int32 device pointer, the valid keys of each
 *     sequence INCLUDING the new tokens; max_len bounds it, <= the cache
 *     capacity.
 *   o: (T, H*D) bf16 row-major contiguous; row t of a span gets query
 *     t - seq_begin[b]. Rows outside every span (an empty span has none) are
 *     all-(+0), written by dolomite_fa_zero_gap_rows from inside this call.
 * Keys at and beyond cache_len[b] never influence the result, whatever that
 * memory holds (NaN and Inf included); keys of later queries of the same
 * chunk are masked exactly. Every value read from the device arrays is
 * clamped (cache_len into [0, max_len], past_b >= 0, n_b <= max_new, the
 * span into [0, T]): with arguments that break the preconditions the result
 * is unspecified, but nothing outside qkv / o / the first max_len cache
 * positions is touched.
 *
 * Work split: for one (sequence, kv head) the n_b*G (query, q head) pairs
 * are flattened query-major, r = i*G + g, and a workgroup owns 128
 * consecutive r, which share one pass over the kv head's K/V. The grid is
 * (nsplit, ceil(max_new*G / 128) * batch, Hkv). Split c of a workgroup owns
 * keys [c*chunk, min((c+1)*chunk, kmax)), kmax the largest causal bound of
 * its columns and chunk = ceil(max_len / nsplit) rounded up to the 64-key
 * tile; a split without keys is legal. With nsplit > 1 the workgroups store
 * fp32 partials exclusively into `scratch` and a second kernel combines them
 * in ascending split order: no atomics, bitwise reproducible for fixed
 * arguments.
 *   scratch: dolomite_fa_extend_scratch_floats(batch, max_new, H, D, nsplit)
 *     floats, 16-byte aligned, caller-owned (0 and may be NULL for
 *     nsplit == 1; the query returns -1 for invalid arguments).
 * Error codes, all returned before any launch: 9010 dtype != bf16, 9011
 * D > 128, 9015 scale not > 0, 9041 D or a stride not a (positive) multiple
 * of 8, 9042 negative / inconsistent sizes (H != Hkv*G included), 9043
 * nsplit < 1 or a grid dimension over its limit, 9044 nsplit > 1 without
 * scratch.
 * ---------------------------------------------------------------------- */
int64_t dolomite_fa_extend_scratch_floats(int batch, int max_new, int H, int D, int nsplit);
int dolomite_fa_extend(dolomite_stream_t stream,
                       const void* qkv, const void* k_cache, const void* v_cache, void* o,
                       float* scratch, const int32_t* seq_begin, const int32_t* seq_end,
                       const int32_t* cache_len,
                       int batch, int max_new, int64_t T, int H, int Hkv, int D, int G,
                       int max_len, int nsplit,
                       int64_t q_tstride, int64_t q_gstride,
                       int64_t k_bstride, int64_t k_tstride, int64_t k_hstride,
                       int64_t v_bstride, int64_t v_tstride, int64_t v_hstride,
                       float scale, int dtype);

/* dolomite_fa_extend_fp8: dolomite_fa_extend over the fp8 KV cache above
 * (e4m3 k_cache / v_cache, fp32 k_scale / v_scale with the strides of
 * dolomite_fa_decode_fp8) — the same spans, causal mask, clamps, gap rows,
 * grid, key split, partials, scratch (dolomite_fa_extend_scratch_floats) and
 * ascending-order combine; qkv and o are bf16 (`dtype`). The keys and values
 * attended are q8 * scale, the new tokens' own included (the quantising append
 * has run). A 64-key tile is converted to bf16 once per workgroup on its way
 * into LDS (exact); the K scale multiplies the fp32 score, the V scale the
 * softmax weight before it is packed to bf16, the row sum is of the unscaled
 * weights. Keys at and beyond cache_len[b] never influence the result
 * whatever bytes and scales they hold, and neither a cache byte nor a scale
 * at or beyond position max_len is read, for any capacity.
 * 8-byte cache loads: D and every stride but the scale strides in units of 8
 * elements.
 * Error codes, all returned before any launch: dolomite_fa_extend's (9042
 * also for a negative scale stride), and 9045 k_scale or v_scale NULL.
 * ---------------------------------------------------------------------- */
int dolomite_fa_extend_fp8(dolomite_stream_t stream,
                           const void* qkv, const void* k_cache, const void* v_cache,
                           const float* k_scale, const float* v_scale, void* o,
                           float* scratch, const int32_t* seq_begin, const int32_t* seq_end,
                           const int32_t* cache_len,
                           int batch, int max_new, int64_t T, int H, int Hkv, int D, int G,
                           int max_len, int nsplit,
                           int64_t q_tstride, int64_t q_gstride,
                           int64_t k_bstride, int64_t k_tstride, int64_t k_hstride,
                           int64_t v_bstride, int64_t v_tstride, int64_t v_hstride,
                           int64_t scale_bstride, int64_t scale_hstride,
                           float scale, int dtype);

/* ------------------------------------------------------------------------
 * fp8 (e4m3) weight-only linear for 1 to 64 rows (W8A16): the skinny GEMM of
 * a decode or short extend step, which reads half the weight bytes of the
 * bf16 F.linear it replaces at modeling_utils/linear.py (ParameterizedLinear).
 *   y[m, n] = bf16( (sum_k x[m, k] * wq[n, k]) * wscale[n] + bias[n] )
 *   x:      (M, K) bf16, row m at x + m*x_row_stride, unit stride on k
 *   wq:     (N, K) OCP e4m3 bytes (torch.float8_e4m3fn), dense
 *   wscale: (N,) fp32, one per output channel. The quantisation rule is the
 *           fp8 KV cache's above, applied per weight row:
 *           scale[n] = max(amax|W[n, :]|, 2^-64) / 448
 *   bias:   (N,) bf16, or NULL
 *   y:      (M, N) bf16, dense; every element is written
 * e4m3 -> bf16 is exact, as are the bf16 products inside the MFMA; the sum is
 * accumulated in fp32 (in an order that depends on nsplit), multiplied by
 * wscale[n] once, the bias added, and rounded once to bf16. Rows of x at and
 * beyond M and channels at and beyond N are never read.
 *
 * Split-K: the grid is (ceil(N / 64), nsplit). Split c owns
 * k in [c*kper, min((c+1)*kper, K)), kper = 64 * ceil(ceil(K / 64) / nsplit);
 * a split without k is legal and contributes zeros. With nsplit > 1 every
 * workgroup stores its fp32 partials exclusively into scratch[c][m][n] and a
 * second kernel sums them in ascending split order before the scale and the
 * bias: no atomics, bitwise reproducible for fixed arguments.
 *   dolomite_fp8_linear_num_splits: the default split count,
 *     min(ceil(256 / ceil(N / 64)), ceil(ceil(K / 64) / 4), max(1, K / (8 M)))
 *     (at least 1), then lowered to drop empty splits: about one workgroup on
 *     each of the 256 CUs, at least one 256-wide k tile per split, and no more
 *     partial bytes (written and read back) than weight bytes. -1 for
 *     arguments dolomite_fp8_linear rejects.
 *   scratch: dolomite_fp8_linear_scratch_floats(M, N, K, nsplit) =
 *     nsplit * M * N floats, 16-byte aligned, caller-owned (0 and may be NULL
 *     for nsplit == 1; the query returns -1 for invalid arguments).
 * 16-byte loads: x and wq 16-byte aligned, x_row_stride a multiple of 8.
 * Error codes, all returned before any launch: 9010 dtype != bf16, 9070
 * M < 1, 9071 M > 64, 9072 K not a positive multiple of 16, 9073 N < 1 or a
 * size over its limit (N < 2^31, K <= 2^30), 9074 x_row_stride < K or not a
 * multiple of 8, or a misaligned pointer, 9075 nsplit < 1 or > 65535, 9076
 * nsplit > 1 without scratch, 9077 a NULL x, wq, wscale or y.
 * ---------------------------------------------------------------------- */
int dolomite_fp8_linear_num_splits(int64_t M, int64_t N, int64_t K);
int64_t dolomite_fp8_linear_scratch_floats(int64_t M, int64_t N, int64_t K, int nsplit);
int dolomite_fp8_linear(dolomite_stream_t stream, const void* x, const void* wq,
                        const float* wscale, const void* bias, void* y, float* scratch,
                        int64_t M, int64_t N, int64_t K, int64_t x_row_stride,
                        int nsplit, int dtype);

/* ------------------------------------------------------------------------
 * fp8 (e4m3) weight-only linear for any number of rows (W8A16): the tiled
 * GEMM that serves ops.fp8_linear above the 64 rows of dolomite_fp8_linear
 * (batched decode, chunked prefill, draft verification, short prompts). Same
 * operands, same arithmetic and same argument conventions as
 * dolomite_fp8_linear above: y[m, n] = bf16( (sum_k x[m, k] * wq[n, k]) *
 * wscale[n] + bias[n] ), exact e4m3 -> bf16 conversion and products, fp32
 * accumulation in an order that depends on nsplit, one rounding. The weight
 * is read as fp8 only; no bf16 copy of it is written anywhere.
 *
 * The grid is (ceil(N / 128), ceil(M / 128), nsplit): a workgroup owns a
 * 128-row x 128-channel tile of y. Split c owns
 * k in [c*kper, min((c+1)*kper, K)), kper = 128 * ceil(ceil(K / 128) / nsplit);
 * a split without k is legal and contributes zeros. With nsplit > 1 every
 * workgroup stores its fp32 partials exclusively into scratch[c][m][n] and a
 * second kernel sums them in ascending split order before the scale and the
 * bias: no atomics, bitwise reproducible for fixed arguments.
 *   dolomite_fp8_gemm_num_splits: the default split count,
 *     min(ceil(256 / tiles), max(1, floor(ceil(K / 128) / 2)), max(1, K / (4 M)))
 *     with tiles = ceil(N / 128) * ceil(M / 128), then lowered to drop empty
 *     splits: about one workgroup on each of the 256 CUs, two k tiles per
 *     split at least, and partial traffic of at most twice the weight bytes.
 *     -1 for arguments dolomite_fp8_gemm rejects.
 *   scratch: dolomite_fp8_gemm_scratch_floats(M, N, K, nsplit) =
 *     nsplit * M * N floats, 16-byte aligned, caller-owned (0 and may be NULL
 *     for nsplit == 1; the query returns -1 for invalid arguments).
 * 16-byte loads: x and wq 16-byte aligned, x_row_stride a multiple of 8.
 * Error codes, all returned before any launch: 9010 dtype != bf16, 9080
 * M < 1, 9081 M > 65535 * 128, 9082 K not a positive multiple of 16, 9083
 * N < 1 or a size over its limit (N < 2^31, K <= 2^30, M * N <= 2^38), 9084
 * x_row_stride < K or not a multiple of 8, or a misaligned pointer, 9085
 * nsplit < 1 or > 65535, 9086 nsplit > 1 without scratch, 9087 a NULL x, wq,
 * wscale or y.
 * ---------------------------------------------------------------------- */
int dolomite_fp8_gemm_num_splits(int64_t M, int64_t N, int64_t K);
int64_t dolomite_fp8_gemm_scratch_floats(int64_t M, int64_t N, int64_t K, int nsplit);
int dolomite_fp8_gemm(dolomite_stream_t stream, const void* x, const void* wq,
                      const float* wscale, const void* bias, void* y, float* scratch,
                      int64_t M, int64_t N, int64_t K, int64_t x_row_stride,
                      int nsplit, int dtype);

/* MFMA fragment-layout self-test: computes C = A(16x32) @ B(32x16) with the
 * compiled fragment mapping; host verifies against a CPU matmul.
 * A/B bf16 row-major contiguous, C fp32 row-major. */
int dolomite_mfma_probe(dolomite_stream_t stream,
                        const void* A, const void* B, float* C);

/* ------------------------------------------------------------------------
 * Fused softmax cross-entropy over the vocab, forward / backward.
 * Replaces F.cross_entropy at model_wrapper/pretraining.py:125 and
 * gpt_dolomite/main.py:200 (mean reduction, ignore_index -100, fp32
 * log-softmax as torch does for bf16 inputs).
 * fwd: per-row loss (T,) fp32 (0 for ignored rows), per-row lse (T,) fp32,
 *      n_valid is computed by the caller.
 * bwd: dlogits = (softmax - onehot) * grad_scale, 0 for ignored rows;
 *      dlogits may alias logits (in-place).
 * logits rows at logits_ptr + t*row_stride.
 * ---------------------------------------------------------------------- */
int dolomite_ce_fwd(dolomite_stream_t stream,
                    const void* logits, const int64_t* labels,
                    float* row_loss, float* lse,
                    int64_t T, int64_t V, int64_t row_stride,
                    int ignore_index, int dtype);
/* grad_scale_dev: DEVICE pointer to one fp32 (upstream grad / n_valid),
 * so the backward launch needs no host readback of device scalars. */
int dolomite_ce_bwd(dolomite_stream_t stream,
                    const void* logits, const int64_t* labels, const float* lse,
                    void* dlogits, const float* grad_scale_dev,
                    int64_t T, int64_t V, int64_t row_stride,
                    int ignore_index, int dtype);

/* ------------------------------------------------------------------------
 * Fused AdamW on a flat fp32 master shard, with bf16 param write-out.
 * Replaces the TorchAdamW step (optimization/optimizer.py:74, defaults
 * arguments.py:235-249) on the ZeRO-2 local shard. torch.optim.AdamW
 * semantics: decoupled wd, bias-corrected moments.
 *   master/m/v: (n,) fp32.  grad: (n,) fp32 or bf16 (grad_dtype).
 *   param_out: (n,) bf16 copy of updated master (NULL to skip).
 *   gscale: optional DEVICE scalar multiplied into every grad element
 *           (the grad-clip coefficient, fused here so the clip costs one
 *           scalar read instead of a read+write pass; NULL = 1.0).
 * ---------------------------------------------------------------------- */
int dolomite_adamw_step(dolomite_stream_t stream,
                        float* master, void* param_out_bf16,
                        const void* grad, int grad_dtype,
                        float* m, float* v,
                        int64_t n, float lr, float beta1, float beta2,
                        float eps, float weight_decay, int step,
                        const float* gscale);

/* Multiply a flat fp32 (or bf16) buffer by a scalar (grad clip apply). */
int dolomite_scale_inplace(dolomite_stream_t stream, void* buf, int64_t n,
                           float scale, int dtype);

/* Deterministic MoE top-k row combine: out[t,:] = sum_j h[inv[t*k_top+j],:]
 * (fixed j order). Replaces torch zeros+index_add for the expert scatter-back
 * (moe/base.py:127) and the backward of the expert-row gather — both ~9x off
 * the HBM roofline in eager torch. inv: (T*k_top,) int32 inverse of the
 * expert sort (inv[pair] = slot). bf16, K % 8 == 0. */
int dolomite_moe_rows_combine(dolomite_stream_t stream, const void* h,
                              const int32_t* inv, void* out,
                              int64_t T, int K, int k_top, int dtype);

/* Deterministic sum of squares (grad-norm input): out[0] = sum(x[i]^2) in
 * fp32, fixed reduction order run-to-run (per-thread strided order + fixed
 * LDS trees), so the clipped optimizer step stays bit-reproducible.
 * partials: (1024,) fp32 scratch. x: (n,) fp32 or bf16. */
int dolomite_sqsum(dolomite_stream_t stream, const void* x, int64_t n,
                   float* partials, float* out, int dtype);

/* ------------------------------------------------------------------------
 * Grouped expert GEMMs for the MoE family — replaces the reference's
 * scattermoe/triton grouped path (moe_dolomite/moe/scatter.py:109-138) for
 * the SparseMoE expert matmuls (moe/base.py:137-156). Rows are
 * expert-sorted; offsets is the (E+1) int32 cumulative row count per
 * expert (device pointer). bf16 in / fp32 accumulate / bf16 out.
 * Requires K % 8 == 0 and N % 8 == 0 (error 9020 otherwise; the Python
 * layer falls back to the eager per-expert loop).
 *   fwd   : y[t,n]    = sum_k x[t,k] * w[e(t),n,k] (+ bias[e,n], opt NULL)
 *   dgrad : dx[t,k]   = sum_n dy[t,n] * w[e(t),n,k]
 *   wgrad : dw[e,n,k] = sum_{t in group e} dy[t,n] * x[t,k]
 * max_rows = largest group size (host int, for grid sizing).
 * ---------------------------------------------------------------------- */
int dolomite_moe_gemm_fwd(dolomite_stream_t stream, const void* x, const void* w,
                          const void* bias, void* y, const int32_t* offsets,
                          int E, int max_rows, int N, int K, int dtype);
int dolomite_moe_gemm_dgrad(dolomite_stream_t stream, const void* dy, const void* w,
                            void* dx, const int32_t* offsets,
                            int E, int max_rows, int N, int K, int dtype);
int dolomite_moe_gemm_wgrad(dolomite_stream_t stream, const void* dy, const void* x,
                            void* dw, const int32_t* offsets,
                            int E, int N, int K, int dtype);

/* ------------------------------------------------------------------------
 * MoE token routing — replaces the torch chain of the SparseMoE router
 * (moe/base.py:96-127): topk, fp32 softmax over the k selected logits,
 * bincount, the expert sort, and the gather / index-put built on it.
 *
 * logits: (T, E) row-major, fp32 or bf16. 1 <= E <= 64,
 * 1 <= top_k <= min(E, 8). With pair p = t*top_k + j:
 *   selected[p]  int32: token t's j-th largest logit's expert (descending
 *                logits; equal logits go to the LOWEST expert index)
 *   gates[p]     softmax over the top_k selected logits of token t, evaluated
 *                in fp32 and rounded once to the logits' dtype
 *   inv[p]       int32: the pair's position ("slot") in the STABLE sort of
 *                the pairs by expert (ascending p inside an expert)
 *   batch_index[slot] = p / top_k (int64),  batch_gates[slot] = gates[p]
 *   num_tokens_per_expert (E,) int64, offsets (E+1,) int32 its exclusive
 *                cumulative sum (offsets[E] = T*top_k)
 * i.e. what selected.flatten().sort(stable=True) gives. Three launches (top-k
 * with a per-tile expert histogram, a scan, a rank-based scatter); no slot
 * comes from an atomic counter: bitwise reproducible.
 *   scratch: dolomite_moe_route_scratch_ints(T, E, top_k) int32, caller-owned
 *     (ceil(T / 128) * E; the query returns -1 for invalid arguments). Need
 *     not be cleared.
 * T == 0 is legal and launches nothing. NaN logits: unspecified result,
 * nothing outside the buffers is touched.
 *
 * dolomite_moe_route_bwd: given d_batch_gates (T*top_k,) in slot order (the
 * logits' dtype), writes every element of d_logits (T, E), which need not be
 * cleared: with w the fp32 softmax of token t's selected logits (recomputed
 * from `logits` as the forward evaluated it, before rounding) and
 * g_j = d_batch_gates[inv[t*top_k + j]],
 *   d_logits[t, selected_j] = w_j * (g_j - sum_i w_i g_i),  +0 elsewhere.
 * top_k == 1 gives exactly +0 everywhere. selected / inv values are clamped
 * into range before use.
 * Error codes, all returned before any launch: 9050 dtype not fp32 / bf16,
 * 9051 E or top_k out of range, 9052 T < 0 or T*top_k >= 2^31, 9053 no
 * scratch.
 * ---------------------------------------------------------------------- */
int64_t dolomite_moe_route_scratch_ints(int64_t T, int E, int top_k);
int dolomite_moe_route_fwd(dolomite_stream_t stream, const void* logits,
                           int32_t* selected, void* gates, int32_t* inv,
                           int64_t* batch_index, void* batch_gates,
                           int64_t* num_tokens_per_expert, int32_t* offsets,
                           int32_t* scratch, int64_t T, int E, int top_k, int dtype);
int dolomite_moe_route_bwd(dolomite_stream_t stream, const void* d_batch_gates,
                           const int32_t* inv, const int32_t* selected,
                           const void* logits, void* d_logits,
                           int64_t T, int E, int top_k, int dtype);
/* The first launch of dolomite_moe_route_fwd alone: `selected` and `gates`
 * (T, top_k) in pair order as stated above, no scan and no scatter. scratch
 * as for the forward (it receives the per-tile expert histogram). Same error
 * codes. */
int dolomite_moe_route_topk(dolomite_stream_t stream, const void* logits,
                            int32_t* selected, void* gates, int32_t* scratch,
                            int64_t T, int E, int top_k, int dtype);

/* ------------------------------------------------------------------------
 * Fused expert MLP of a MoE decode / short extend step: 1 <= T <= 64 tokens,
 * top_k of E experts each — replaces, for those sizes, the gather, the two
 * grouped GEMMs, the activation, the gate multiply and the combine of
 * SparseMoE.forward (moe/base.py:129-160), and needs no expert sort.
 *   out[t] = sum_j gates[t,j] * (W_proj[e] act(W_fc[e] x[t] + b_fc[e]) + b_proj[e]),
 *   e = selected[t,j], summed in ascending j
 *   x        (T, H) bf16, dense        selected (T, top_k) int32, ids of a row distinct
 *   gates    (T, top_k) bf16
 *   w_fc     (E, F, H) bf16, dense; F = 2I with glu != 0 (rows [0, I) the `a`
 *            half, [I, 2I) the `b` half: h = a * act(b)), else F = I (h = act(.))
 *   w_proj   (E, H, I) bf16, dense     b_fc (E, F), b_proj (E, H) bf16, or NULL
 *   h        (T*top_k, I) bf16 and part (T*top_k, H) fp32: caller-owned
 *            scratch, need not be cleared
 *   out      (T, H) bf16; every element is written
 * act is a DOLOMITE_ACT_* code (expressions: the GLU section below). Sums are
 * fp32; h is rounded to bf16 once, out once. Three launches (fc + activation,
 * proj * gate into part, combine), no host readback, no atomics: bitwise
 * reproducible for fixed arguments. The weight of an expert no row selects is
 * not read. Ids outside [0, E) select nothing (their rows of part stay
 * unwritten); nothing outside the buffers is touched.
 * waves: 0 takes the occupancy rule (workgroups of 4, 2 or 1 waves of 16
 * channels each: the largest for which ceil(ceil(N / 16) / waves) *
 * min(E, T*top_k) >= 256, else 1, N the launch's output width); 1, 2 or 4
 * forces one.
 * Error codes, all returned before any launch: 9010 dtype != bf16, 9080 T
 * outside [1, 64], 9081 E outside [1, 64] or top_k outside [1, min(E, 8)],
 * 9082 H or I not a positive multiple of 8 (or over 2^24), 9083 unknown act,
 * 9084 waves not 0 / 1 / 2 / 4, 9085 a NULL buffer, 9086 a misaligned one
 * (16 bytes: x, w_fc, w_proj, h, part; 8: out).
 * ---------------------------------------------------------------------- */
int dolomite_moe_decode_mlp(dolomite_stream_t stream, const void* x, const int32_t* selected,
                            const void* gates, const void* w_fc, const void* b_fc,
                            const void* w_proj, const void* b_proj, void* h, float* part,
                            void* out, int T, int E, int top_k, int H, int I, int act, int glu,
                            int waves, int dtype);

/* ------------------------------------------------------------------------
 * GLU activation, forward / backward — replaces the torch chain
 * `a, b = h.chunk(2, -1); a * act(b)` of the gated MLP (glu.py:26-28) and its
 * autograd backward (two multiplies, the activation's backward, a cat) on the
 * fused c_fc layout [up ; gate] that hf_models/conversion.py writes.
 *   h : (R, 2I) row-major, row stride ld_h >= 2I elements (a view into a wider
 *       buffer is fine); up = h[:, :I], gate = h[:, I:2I]
 *   fwd: y (R, I) dense,   y[r, c]       = up * act(gate)
 *   bwd: g = dL/dy (R, I) dense, dh (R, 2I) dense (row stride 2I),
 *                          dh[r, c]      = g * act(gate)
 *                          dh[r, I + c]  = g * up * act'(gate)
 * The backward recomputes act and act' from h: nothing but h is saved. Every
 * element of y / dh is written (no memset needed), evaluated in fp32 from the
 * loaded values and rounded once to `dtype`. With s(x) = 1 / (1 + exp(-x)),
 * k0 = sqrt(2/pi), k1 = 0.044715:
 *   DOLOMITE_ACT_SILU       act = x s(x)          act' = s (1 + x (1 - s))
 *   DOLOMITE_ACT_GELU_TANH  u = k0 x (1 + k1 x^2), e = exp(-2|u|), r = 1 / (1 + e)
 *                           c = (1 + tanh u) / 2 = r for u >= 0, e r for u < 0
 *                           d = 1 - tanh^2 u     = 4 e r^2
 *                           act = x c             act' = c + x d k0 (1 + 3 k1 x^2) / 2
 *                           (the second term is +0 where d == 0). tanh as
 *                           1 - 2 / (exp(2u) + 1) loses 1 + t and 1 - t^2 to
 *                           cancellation near saturation; this form does not.
 *   DOLOMITE_ACT_GELU       c = (1 + erf(x / sqrt 2)) / 2
 *                           act = x c             act' = c + x exp(-x^2 / 2) / sqrt(2 pi)
 *   DOLOMITE_ACT_RELU       act = max(x, 0)       act' = 1 for x > 0, else 0
 * s, c and d saturate (to 0 or 1) for finite x of any size: no inf * 0 and
 * no inf / inf. NaN and Inf inputs are unspecified.
 * Lanes move 16-byte vectors (8 bf16 / 4 fp32) when I and ld_h are multiples
 * of that width and h, y, g, dh are 16-byte aligned; any other I >= 1 runs an
 * element-per-lane instantiation. R == 0 or I == 0 launches nothing.
 * Error codes, all returned before any launch: 9060 unknown act, 9061 dtype
 * not fp32 / bf16, 9062 R < 0 or I < 0, 9063 ld_h < 2I.
 * ---------------------------------------------------------------------- */
enum dolomite_act {
    DOLOMITE_ACT_SILU = 0,
    DOLOMITE_ACT_GELU_TANH = 1,
    DOLOMITE_ACT_GELU = 2,
    DOLOMITE_ACT_RELU = 3
};
int dolomite_glu_fwd(dolomite_stream_t stream, const void* h, int64_t ld_h,
                     void* y, int64_t R, int64_t I, int act, int dtype);
int dolomite_glu_bwd(dolomite_stream_t stream, const void* g, const void* h,
                     int64_t ld_h, void* dh, int64_t R, int64_t I, int act, int dtype);

/* ------------------------------------------------------------------------
 * Host-side dataset index builders (CPU; the reference's only native
 * component, data/megatron/utils/helpers.cpp).
 * build_sample_idx: pack epoch-replicated documents into seq_length+1 token
 *   windows; sample_idx is [(num_samples+1) x 2] rows of (doc_idx position,
 *   token offset); caller computes num_samples =
 *   (num_epochs*tokens_per_epoch - 1) / seq_length and allocates.
 * build_blending_indices: greedy max-error dataset interleave. Buffers are
 * HOST pointers.
 * ---------------------------------------------------------------------- */
int dolomite_build_sample_idx_i32(const int32_t* sizes, const int32_t* doc_idx,
                                  int32_t seq_length, int32_t num_epochs,
                                  int64_t tokens_per_epoch, int32_t* sample_idx,
                                  int64_t num_samples);
int dolomite_build_sample_idx_i64(const int32_t* sizes, const int32_t* doc_idx,
                                  int32_t seq_length, int32_t num_epochs,
                                  int64_t tokens_per_epoch, int64_t* sample_idx,
                                  int64_t num_samples);
int dolomite_build_blending_indices(int16_t* dataset_index, int64_t* dataset_sample_index,
                                    const double* weights, int32_t num_datasets,
                                    int64_t size);

#ifdef __cplusplus
}
#endif

#endif /* DOLOMITE_HIP_H */
