// What the persistent batch-streaming wgrad kernels share: linear_wgrad.hip
// (all No <= 256 rows of dW per block, x cut into column tiles),
// linear_wgrad_wide.hip (its mirror image: dz cut into column tiles) and
// hidden_bwd.hip (linear_wgrad.hip's decomposition with the masked dgrad
// added).  Each rule of the family is written here once:
//
//   * the batch-tile image: 32 batch rows of dz / x staged as they lie in
//     memory, 16 B slots XOR-swizzled by row, read back through the
//     transposing LDS read as k-packed MFMA fragments that reduce over the
//     batch rows.  An operand is staged either as whole rows (lwg_row_image)
//     or as one LWG_XCOLS-wide column slice of its rows, clamped into the row
//     (lwg_slice_image); full tiles go global->LDS by DMA, the partial last
//     tile through registers with zero fill;
//   * the block deal: block id -> (row group, column tile), the column tiles of
//     a row group on one XCD;
//   * the walk's plan: which tiles a row group owns and where a long walk
//     flushes half-way;
//   * dW / db of the decomposition that keeps all dW rows in a block: the
//     accumulate step and the atomic flush;
//   * on the host: the bounds every launcher checks, the grid plan and the
//     dispatch on the fragment counts.
//
// Device helpers are __device__ __forceinline__ templates on compile-time
// sizes.  Those called from a kernel's lambdas take their arguments by const
// reference, as the lambdas take their captures: by value the compiler
// simplifies the helper on its own first and the kernels' instruction stream
// and register count move (profiles/wgrad_family_refactor.md).  Names carry
// the lwg_ / LWG_ prefix: the tools include several .hip files into one
// translation unit.
#pragma once

#include <type_traits>

#include "mfma_tile.h"

#define LWG_ROWS 32    // batch rows per tile = one 16x16x32 k-step
#define LWG_SPLIT_TILES 64  // register chains this long (2048 rows) are flushed half-way
#define LWG_XCOLS 128  // slice image row: 16 slots of 16 B (NF = 7 leaves two unused)
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

// ---- block deal ----

// block id -> (row group, column tile).  Hardware deals consecutive ids
// round-robin over the 8 XCDs; with xcd_deal the ncol blocks of a group are
// consecutive slots of ONE XCD, so they start together and their re-reads of
// the operand they share hit that XCD's L2.
__device__ __forceinline__ void lwg_block_deal(const int& ncol, const int& xcd_deal, int& grp,
                                               int& ct) {
  if (xcd_deal) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    grp = (j / ncol) * 8 + xcd;
    ct = j % ncol;
  } else {
    grp = blockIdx.x / ncol;
    ct = blockIdx.x % ncol;
  }
}

// ---- the two tile images ----
//
// SLOTS: 16 B slots per image row; WAVES: waves of the block (4 or 8).  A tile
// is LWG_ROWS * SLOTS * 16 B = DMA * WAVES 1 KB chunks; wave w issues chunks
// w, w + WAVES, ...: chunk c fills image rows c * RPC ... + RPC - 1, so a
// lane's row advances by a multiple of 8 from one of its chunks to the next,
// its swizzle key stays, and one 32-bit lane offset (plus a wave-uniform base)
// serves all of them.
template <int SLOTS, int WAVES>
struct lwg_image_base {
  static constexpr int COLS = SLOTS * 8;
  static constexpr int ELEMS = LWG_ROWS * COLS;
  static constexpr int RPC = 64 / SLOTS;                // image rows per chunk
  static constexpr int DMA = ELEMS * 2 / 1024 / WAVES;  // DMA instructions per wave and tile
  static_assert(DMA >= 1 && DMA * WAVES * 1024 == ELEMS * 2,
                "chunks are dealt evenly to the waves");
  static_assert(DMA == 1 || (WAVES * RPC) % 8 == 0, "key must not depend on the chunk");
  static_assert(LWG_ROWS * SLOTS % (64 * WAVES) == 0, "the tail's slots are dealt evenly");
};

// Whole rows of an operand whose row length SLOTS * 8 is fixed at compile time.
template <int SLOTS, int WAVES>
struct lwg_row_image : lwg_image_base<SLOTS, WAVES> {
  using base = lwg_image_base<SLOTS, WAVES>;
  // the lane's source offset in its first chunk
  static __device__ __forceinline__ unsigned lane_off(int wid, int lane) {
    const int r0 = wid * base::RPC + lane / SLOTS;
    return r0 * base::COLS + (((lane % SLOTS) ^ lwg_key<SLOTS>::key(r0)) << 3);
  }
  // one full tile, rows row0 .. row0 + LWG_ROWS - 1 of g, to img
  static __device__ __forceinline__ void dma(const bf16raw* __restrict__ const& g,
                                             bf16raw* const& img, const int64_t& row0,
                                             const unsigned& off, const int& wid) {
#pragma unroll
    for (int i = 0; i < base::DMA; ++i) {
      const bf16raw* p = g + (row0 + i * WAVES * base::RPC) * base::COLS;
      mt_glds16(p + off, img + (wid + WAVES * i) * 512);
    }
  }
  // the partial last tile through registers: rows at or past B are zero
  static __device__ __forceinline__ void fill_tail(const bf16raw* __restrict__ const& g,
                                                   bf16raw* const& img, const int64_t& row0,
                                                   const int& B, const int& t) {
#pragma unroll
    for (int u = t; u < LWG_ROWS * SLOTS; u += 64 * WAVES) {
      const int row = u / SLOTS;
      const int slot = (u % SLOTS) ^ lwg_key<SLOTS>::key(row);
      shortx8 v = {};
      if (row0 + row < B) v = *(const shortx8*)(g + (row0 + row) * base::COLS + slot * 8);
      *(shortx8*)(img + u * 8) = v;
    }
  }
};

// A column slice, SLOTS wide from slot slot0, of an operand with ld columns
// (nslots = ld / 8 slots a row), both known at run time.  Slots past the row's
// end are clamped to its last slot: they fill image columns whose products are
// never flushed (MFMA output rows and columns are independent).
template <int SLOTS, int WAVES>
struct lwg_slice_image : lwg_image_base<SLOTS, WAVES> {
  using base = lwg_image_base<SLOTS, WAVES>;
  static __device__ __forceinline__ unsigned lane_off(int wid, int lane, int ld, int slot0,
                                                      int nslots) {
    const int r0 = wid * base::RPC + lane / SLOTS;
    int gs = slot0 + ((lane % SLOTS) ^ lwg_key<SLOTS>::key(r0));
    if (gs > nslots - 1) gs = nslots - 1;
    return r0 * ld + gs * 8;
  }
  static __device__ __forceinline__ void dma(const bf16raw* __restrict__ const& g,
                                             bf16raw* const& img, const int64_t& row0,
                                             const unsigned& off, const int& wid, const int& ld) {
#pragma unroll
    for (int i = 0; i < base::DMA; ++i) {
      const bf16raw* p = g + (row0 + i * WAVES * base::RPC) * ld;
      mt_glds16(p + off, img + (wid + WAVES * i) * 512);
    }
  }
  static __device__ __forceinline__ void fill_tail(const bf16raw* __restrict__ const& g,
                                                   bf16raw* const& img, const int64_t& row0,
                                                   const int& B, const int& t, const int& ld,
                                                   const int& slot0, const int& nslots) {
#pragma unroll
    for (int u = t; u < LWG_ROWS * SLOTS; u += 64 * WAVES) {
      const int row = u / SLOTS;
      int gs = slot0 + ((u % SLOTS) ^ lwg_key<SLOTS>::key(row));
      if (gs > nslots - 1) gs = nslots - 1;
      shortx8 v = {};
      if (row0 + row < B) v = *(const shortx8*)(g + (row0 + row) * ld + gs * 8);
      *(shortx8*)(img + u * 8) = v;
    }
  }
};

// ---- the walk ----

// Row group grp walks full tiles grp, grp + groups, ... < nfull: my_tiles of
// them.  A block with LWG_SPLIT_TILES or more flushes once half-way: fp32
// rounding grows with the length and magnitude of one accumulator chain, and
// the extra flush halves both for the price of one more pass of atomics.  The
// first segment is a multiple of PERIOD tiles (the number of image sets the
// kernel's unrolled tile loop turns through), so the sets keep their turn:
// lwg_half_walk gives its length in tiles, 0 for a walk that is not split.
__device__ __forceinline__ int lwg_my_tiles(const int& grp, const int& groups, const int& nfull) {
  return grp < nfull ? (nfull - grp + groups - 1) / groups : 0;
}
template <int PERIOD>
__device__ __forceinline__ int lwg_half_walk(const int& my_tiles) {
  static_assert(PERIOD == 2 || PERIOD == 3, "two or three image sets");
  if (my_tiles < LWG_SPLIT_TILES) return 0;
  return PERIOD == 2 ? (((my_tiles + 1) / 2 + 1) & ~1) : ((my_tiles + 1) / 2 + 2) / 3 * 3;
}

// ---- dW / db with all dW rows in the block ----
//
// Wave wid owns dW rows 16 MF wid .. + 16 MF - 1 (fragments of the whole-row
// dz image, ZSLOTS slots a row) times the NF fragments of the x slice image.
// db is a ones-fragment MFMA on the dz fragments, in the blocks that have
// do_db set (column tile 0): no virtual column, no extra tile.

template <int MF, int NF, int ZSLOTS>
__device__ __forceinline__ void lwg_accumulate(floatx4 (&acc)[MF][NF], floatx4 (&accb)[MF],
                                               const bf16raw* const& zb, const bf16raw* const& xb,
                                               const mt_frag_t& ones, const bool& do_db,
                                               const int& wid, const int& q, const int& l15) {
  mt_frag_t az[MF];
#pragma unroll
  for (int a = 0; a < MF; ++a) az[a] = lwg_tr_frag<ZSLOTS>(zb, q, l15, (wid * MF + a) * 16);
  if (do_db) {
#pragma unroll
    for (int a = 0; a < MF; ++a)
      accb[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az[a], ones, accb[a], 0, 0, 0);
  }
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const mt_frag_t bx = lwg_tr_frag<LWG_XCOLS / 8>(xb, q, l15, f * 16);
#pragma unroll
    for (int a = 0; a < MF; ++a)
      acc[a][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az[a], bx, acc[a][f], 0, 0, 0);
  }
}

// Adds the accumulators to dw / db and clears them.  Accumulator lane
// (l15, q), element r <-> dW row base + 4q + r, column l15 of the fragment (16
// lanes = one 64 B segment).  seg_end: the end of the segment just walked.
template <int MF, int NF>
__device__ __forceinline__ void lwg_flush(floatx4 (&acc)[MF][NF], floatx4 (&accb)[MF],
                                          float* __restrict__ const& dw,
                                          float* __restrict__ const& db, const int& Ki,
                                          const int& ct, const bool& do_db, const int& seg_end,
                                          const int& wid, const int& q, const int& l15) {
  // Derived from the segment end so that the flush addresses are formed
  // here, not hoisted above the tile loop where they would cost registers.
  float* const dwp = dw + (__builtin_amdgcn_readfirstlane(seg_end) - seg_end);
#pragma unroll
  for (int a = 0; a < MF; ++a) {
    const int no = (wid * MF + a) * 16 + q * 4;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int col = ct * (NF * 16) + f * 16 + l15;
      if (col < Ki) {
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(dwp + (int64_t)(no + r) * Ki + col, acc[a][f][r]);
      }
      acc[a][f] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    if (do_db && l15 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(db + no + r, accb[a][r]);
    }
    accb[a] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
}

// ---- host side ----

// The bounds every launcher of the family checks: `cols`, the run-time width
// (of the operand that is cut into column tiles), is a whole number of 16 B
// slots and keeps 32-bit offsets; B leaves room for the tile past the last row
static inline bool lwg_bounds_ok(int cols, int64_t B) {
  return cols >= 8 && (cols & 7) == 0 && cols < (1 << 24) && B >= 1 &&
         B < (1LL << 31) - LWG_ROWS;
}

// column tile width in 16-column fragments: the one of {7, 8} that covers
// `cols` with fewer dead columns (784 = 7 x 112; 256 = 2 x 128)
static inline int lwg_nf(int cols) {
  const int c7 = (cols + 111) / 112 * 112, c8 = (cols + 127) / 128 * 128;
  return c7 < c8 ? 7 : 8;
}

// The persistent grid: ncol column tiles of nf fragments times `groups` row
// groups, groups * ncol blocks.
struct lwg_grid {
  int nf, ncol, groups, xcd_deal;
};

// max_blocks > 0 caps the row groups (tests force many tiles per block with it)
static inline lwg_grid lwg_grid_plan(int cols, int64_t B, int blocks_per_cu, int max_blocks,
                                     int num_cus) {
  lwg_grid g;
  g.nf = lwg_nf(cols);
  g.ncol = (cols + g.nf * 16 - 1) / (g.nf * 16);
  const int ntiles = (int)((B + LWG_ROWS - 1) / LWG_ROWS);
  g.groups = blocks_per_cu * (num_cus > 0 ? num_cus : 256) / g.ncol;
  if (g.groups < 1) g.groups = 1;
  // at least LWG_MIN_TILES tiles (512 rows, the split-K route's floor per
  // slice) per block: fewer, longer register chains and fewer flushes
  if (g.groups > ntiles / LWG_MIN_TILES) g.groups = ntiles / LWG_MIN_TILES;
  if (g.groups < 1) g.groups = 1;
  if (max_blocks > 0 && g.groups > max_blocks) g.groups = max_blocks;
  g.xcd_deal = 0;
  if (g.groups >= 8) {
    g.groups &= ~7;
    g.xcd_deal = 1;
  }
  return g;
}

// Calls launch(lwg_int<F>, lwg_int<NF>) for the F of FS... that equals frags
// and NF = nf in {7, 8}: the kernels' two template arguments.
template <int V>
using lwg_int = std::integral_constant<int, V>;

template <int... FS, typename L>
static inline void lwg_dispatch(int frags, int nf, L launch) {
  auto with_nf = [&](auto f) {
    if (nf == 7)
      launch(f, lwg_int<7>{});
    else
      launch(f, lwg_int<8>{});
  };
  ((frags == FS ? with_nf(lwg_int<FS>{}) : void()), ...);
}
