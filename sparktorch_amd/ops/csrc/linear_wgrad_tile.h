// The batch-tile image that linear_wgrad.hip and hidden_bwd.hip share: 32
// batch rows of dz / x staged as they lie in memory, 16 B slots XOR-swizzled
// by row, read back through the transposing LDS read as k-packed MFMA
// fragments that reduce over the batch rows.
#pragma once

#include "mfma_tile.h"

#define LWG_ROWS 32    // batch rows per tile = one 16x16x32 k-step
#define LWG_SPLIT_TILES 64  // register chains this long (2048 rows) are flushed half-way
#define LWG_XCOLS 128  // x image row: 16 slots of 16 B (NF = 7 leaves two unused)
#define LWG_MIN_TILES 16  // tiles per block below which the grid shrinks instead

// Slot swizzle.  A transposing read's 32-lane half covers an aligned group of
// 8 rows x 32 B (one 16-column fragment = an aligned slot pair per row); the
// key moves the 8 rows' pairs onto 8 distinct 32 B bank groups.
template <int SLOTS>
struct lwg_key {
  static __device__ __forceinline__ int key(int row) {
    return SLOTS >= 16 ? ((row & 7) << 1) : (((row >> 1) & 3) << 1);
  }
};

// fragment value i <-> tile row (i/4)*16 + q*4 + (i%4), column col0 + l15
// (the same row order for both operands, so the k pairing is consistent)
template <int SLOTS>
__device__ __forceinline__ mt_frag_t lwg_tr_frag(const bf16raw* __restrict__ img, int q, int l15,
                                                 int col0) {
  return mt_tr_frag<SLOTS * 8, 4, 16, lwg_key<SLOTS>>(img, 0, q, l15, col0);
}

// x tile width in 16-column fragments: the one of {7, 8} that covers Ki with
// fewer dead columns (784 = 7 x 112; 256 = 2 x 128)
static inline int lwg_nf(int Ki) {
  const int c7 = (Ki + 111) / 112 * 112, c8 = (Ki + 127) / 128 * 128;
  return c7 < c8 ? 7 : 8;
}
