// dolomite_hip — what the extend attention kernels share (extend.hip over the
// bf16 cache, extend_fp8.hip over the e4m3 cache): the tile constants, the
// clamped span of one sequence and the host side of the split combine.
#pragma once

#include "mfma_tiles.h"

#define EXT_LOG2E 1.44269504088896340736f

#define EXT_COLS 128     // (query, head) columns per workgroup: 8 waves x 16
#define EXT_KTILE 64     // keys per staged tile

// The new-token span and key count of sequence b, every value clamped so
// that bad arguments cannot address outside qkv / o / the cache: rows
// [s0, s0 + n) with 0 <= s0, s0 + n <= T and n <= max_new; len in
// [0, max_len]; past = len - n, at least 0.
struct ExtSeq {
    int s0, n, len, past;
};

__device__ __forceinline__ ExtSeq ext_seq(const int32_t* seq_begin, const int32_t* seq_end,
                                          const int32_t* cache_len, int b, int max_new, int max_len, int T) {
    ExtSeq s;
    s.s0 = min(max(__builtin_amdgcn_readfirstlane(seq_begin[b]), 0), T);
    const int e = __builtin_amdgcn_readfirstlane(seq_end[b]);
    s.n = min(min(max(e - s.s0, 0), max_new), T - s.s0);
    s.len = min(max(__builtin_amdgcn_readfirstlane(cache_len[b]), 0), max_len);
    s.past = max(s.len - s.n, 0);
    return s;
}

// Split combine of the extend kernels (defined in extend.hip): o's span rows
// from the fp32 partials of `rows` = batch*max_new*H slots, in ascending
// split order.
int dol_fa_extend_combine(hipStream_t s, const float* part_o, const float* part_m, const float* part_l,
                          __bf16* o, const int32_t* seq_begin, const int32_t* seq_end,
                          const int32_t* cache_len, int64_t rows, int max_new, int max_len, int T, int H,
                          int D, int nsplit);
