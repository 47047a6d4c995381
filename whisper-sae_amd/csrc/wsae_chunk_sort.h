// The sorted compact code the weight-gradient contractions read (wsae_wgrad.hip): its layout, the entry word and the range
// read.  It is written by a per-chunk counting sort, in a launch of its own (bucket_kernel, bucket_sort_kernel) or as the tail
// of the chunked MFMA decode (wsae_decode_mfma.hip).  Per chunk of KT batch rows the entries are ordered by feature tile of
// width tw:
//   ent_off[chunk][t] .. ent_off[chunk][t + 1] : positions, in the flat arrays, of the entries of tile t (ntiles + 1 per chunk);
//   ent_pos : the entry word below;  ent_hid = relu(value), ent_dpre = dpre, in the contraction dtype.
// The three sorts keep their own text (count, one-wave exclusive scan, scatter): behind a shared function each of them
// compiles to other instructions ("What the contraction kernels share").
#pragma once

#include "wsae_common.h"

#define BUCKET_MAX_TILES 512

// Entry word: feature in tile << 16 | row in chunk (a chunk has at most 64 rows: 6 bits).  wgrad2s_kernel keeps the entry's
// rank among the entries of its 2:4 group in bits 9:8 of the copy it holds in registers; the sorts write them as zero.
// wgrad2_kernel and wgrad2s_kernel take the word apart by hand for the same reason the sorts keep their text.
__device__ __forceinline__ uint32_t ent_pack(int feature, int row) { return ((uint32_t)feature << 16) | (uint32_t)row; }
__device__ __forceinline__ int ent_feature(uint32_t p) { return (int)(p >> 16); }
__device__ __forceinline__ int ent_row(uint32_t p) { return (int)(p & 0xFFFFu); }

// (lo, n): the entries of tile tm in chunk ck.  Chunks past the last read the last one's row: the contraction kernels run their
// offsets a chunk or more ahead with unconditional loads.
__device__ __forceinline__ void ent_range(const int32_t* ent_off, int ck, int nchunks, int ntm, int tm, int& lo, int& n) {
    const int32_t* o = ent_off + (int64_t)min(ck, nchunks - 1) * (ntm + 1) + tm;
    lo = o[0];
    n = o[1] - lo;
}
