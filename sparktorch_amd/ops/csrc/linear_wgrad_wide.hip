// Batch-streaming weight/bias gradient of a WIDE Linear layer on a narrow
// input (an autoencoder's 256 -> 784 output layer) with a huge batch:
//
//   dw[No, Ki] += dz[B, No]^T @ x[B, Ki]     fp32, accumulate
//   db[No]     += colsum(dz)                 fp32, accumulate, optional
//
// dz and x are bf16, row-major, contiguous; Ki is 64, 128 or 256, No any
// multiple of 8.  This is the mirror image of linear_wgrad.hip, which holds
// all No <= 256 rows of dW in a block and cuts x into column tiles: its
// accumulators would not fit at No = 784.  Here
//
//   * a block owns one column tile of dz (112 or 128 columns, its rows of dW:
//     784 = 7 x 112 exactly) times ALL Ki columns of x, so dz, the big
//     operand, is read once chip-wide and the x tile (at most 16 KB) once per
//     column tile;
//   * the grid is persistent: (column tiles) x (row groups) resident blocks,
//     each walking the 32-row batch tiles of its row group with its dW / db
//     accumulators in registers and flushing with fp32 atomicAdd at the end
//     (and once half-way when the walk is long, to halve the fp32 chain);
//   * both tiles go global->LDS by DMA exactly as they lie in memory
//     (double-buffered, one barrier per tile; profiles/linear_wgrad_wide.md
//     has why two buffers stayed), 16 B slots XOR-swizzled by row, and both
//     MFMA operands come from the transposing LDS read (lwg_tr_frag);
//   * the dz fragment is the MFMA's A operand (dW rows), the x fragment its B
//     operand (dW columns): an accumulator's 16 lanes l15 run along Ki and
//     the flush is 64 B segments of atomics, as in linear_wgrad.hip.  The 4
//     waves split the Ki columns; every wave reads all dz fragments;
//   * every column tile produces the db of its own rows with a ones-fragment
//     MFMA on the dz fragments of its image, fragment f in wave f % 4;
//   * the column tiles of one row group share an XCD: their x re-reads hit
//     that XCD's L2.
//
// Rows past B: the (at most one) partial tile is staged through registers
// with zero fill after the DMA loop over the full tiles.  Columns past No in
// the last column tile are clamped into the row; their dW rows and db entries
// are never flushed.
//
// The images, the block deal, the walk's plan and the grid plan are
// linear_wgrad_tile.h's.  The accumulate step and the flush are this file's
// own: dW is held transposed to linear_wgrad.hip's and db is read in another
// order.

#include "launchers.h"
#include "linear_wgrad_tile.h"

#define LWW_THREADS 256

// MF: 16-column x fragments per wave (Ki = 64 * MF); NF: 16-column fragments
// of the dz tile (tile width 16 * NF = the block's rows of dW)
template <int MF, int NF>
__global__ __launch_bounds__(LWW_THREADS, 2) void linear_wgrad_wide_kernel(
    const bf16raw* __restrict__ dz, const bf16raw* __restrict__ x, float* __restrict__ dw,
    float* __restrict__ db, int B, int No, int ncol, int groups, int xcd_deal) {
  constexpr int KI = 64 * MF;
  constexpr int XSLOTS = KI / 8;                  // 16 B slots per x image row
  constexpr int ZSLOTS = LWG_XCOLS / 8;           // and per dz image row
  constexpr int NB = (NF + 3) / 4;                // db fragments per wave
  using ZI = lwg_slice_image<ZSLOTS, LWW_THREADS / 64>;  // dz: the block's column tile
  using XI = lwg_row_image<XSLOTS, LWW_THREADS / 64>;    // x: whole rows
  static_assert(MF == 1 || MF == 2 || MF == 4, "Ki must be 64, 128 or 256");
  static_assert(NF >= 1 && NF * 16 <= LWG_XCOLS, "dz tile wider than its image");

  // One LDS variable per buffer, selected at compile time (the tile loop is
  // unrolled by two): the compiler can then tell the DMA into one pair from
  // the fragment reads of the other and does not wait for the prefetch
  // before them.
  __shared__ __attribute__((aligned(16))) bf16raw zs0[LWG_ROWS * LWG_XCOLS];
  __shared__ __attribute__((aligned(16))) bf16raw zs1[LWG_ROWS * LWG_XCOLS];
  __shared__ __attribute__((aligned(16))) bf16raw xs0[LWG_ROWS * KI];
  __shared__ __attribute__((aligned(16))) bf16raw xs1[LWG_ROWS * KI];

  const int t = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int l15 = lane & 15, q = lane >> 4;

  int grp, ct;
  lwg_block_deal(ncol, xcd_deal, grp, ct);
  const int nfull = B / LWG_ROWS;   // full tiles: DMA, no bounds to check
  const int nslots = No >> 3;       // 16 B slots per dz row
  const int slot0 = ct * (NF * 2);  // first slot of this column tile
  const int row_base = ct * (NF * 16);  // and its first row of dW

  const unsigned xoff = XI::lane_off(wid, lane);
  const unsigned zoff = ZI::lane_off(wid, lane, No, slot0, nslots);
  auto stage = [&](bf16raw* zn, bf16raw* xn, int tile) {
    const int64_t row0 = (int64_t)tile * LWG_ROWS;
    ZI::dma(dz, zn, row0, zoff, wid, No);
    XI::dma(x, xn, row0, xoff, wid);
  };

  mt_frag_t ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (short)MT_BF16_ONE;

  floatx4 acc[NF][MF] = {};
  floatx4 accb[NB] = {};
  const bool do_db = db != nullptr;

  // db: wave w sums dz fragments w and w + 4, read once more from the image
  // and summed whether db is wanted or not: the tile loop stays free of
  // branches.  These reads use mfma_tile.h's k-ascending packing (lane group
  // g holds rows 8g .. 8g + 7), not lwg_tr_frag's: against a ones fragment
  // any pairing is right, and this one sums a tile's rows in the order of
  // gemm.hip's ones column, so a single chain gives that route's db.  (The
  // swizzle is laid out for lwg_tr_frag's rows; these 2 of a tile's 14 reads
  // take a 2-way bank conflict.)  With NF = 7 wave 3's second fragment is the
  // image's unused 16 columns: summed, never flushed.
  const int fb0 = wid * 16;

  auto mma = [&](const bf16raw* zb, const bf16raw* xb) {
    mt_frag_t bx[MF];
#pragma unroll
    for (int m = 0; m < MF; ++m) bx[m] = lwg_tr_frag<XSLOTS>(xb, q, l15, (wid * MF + m) * 16);
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const mt_frag_t az = mt_tr_frag<LWG_XCOLS, 8, 4, lwg_key<ZSLOTS>>(zb, 0, q, l15, fb0 + j * 64);
      accb[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az, ones, accb[j], 0, 0, 0);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const mt_frag_t az = lwg_tr_frag<ZSLOTS>(zb, q, l15, f * 16);
#pragma unroll
      for (int m = 0; m < MF; ++m)
        acc[f][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az, bx[m], acc[f][m], 0, 0, 0);
    }
  };

  int tile = grp;
  // one full tile: zb / xb hold it, zn / xn take the prefetch of the block's next
  auto step = [&](const bf16raw* zb, const bf16raw* xb, bf16raw* zn, bf16raw* xn) {
    // this tile's images are complete and every wave is done with the other pair
    __syncthreads();
    const int next = tile + groups;
    if (next < nfull) stage(zn, xn, next);
    mma(zb, xb);
    tile = next;
  };
  // flush: accumulator lane (l15, q), element r <-> dW row base + 4q + r,
  // column l15 of the fragment (16 lanes = one 64 B segment).  No is a
  // multiple of 8, so the 4 rows of a lane are all inside or all outside.
  auto flush = [&](int seg_end) {
    // A zero the compiler cannot see through, derived from the segment end:
    // the flush offsets are then formed here, not hoisted above the tile
    // loop where they would cost registers.  No < 2^24 keeps them in 32 bits.
    const unsigned zero = __builtin_amdgcn_readfirstlane(seg_end) - seg_end;
    const int no0 = row_base + q * 4;
    const unsigned o0 = (unsigned)(no0 + zero) * KI + wid * (MF * 16) + l15;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
#pragma unroll
      for (int m = 0; m < MF; ++m) {
        if (no0 + f * 16 < No) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            atomicAdd(dw + (o0 + (unsigned)((f * 16 + r) * KI + m * 16)), acc[f][m][r]);
        }
        acc[f][m] = floatx4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int fb = wid + 4 * j;
      const int no = no0 + fb * 16;
      if (do_db && l15 == 0 && fb < NF && no < No) {
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(db + no + r, accb[j][r]);
      }
      accb[j] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
  };

  // the half-way flush comes after an even count of tiles, so the buffer
  // pairs keep their turn
  const int half = lwg_half_walk<2>(lwg_my_tiles(grp, groups, nfull));
  int end = half ? grp + half * groups : nfull;
  if (tile < nfull) stage(zs0, xs0, tile);
  for (;;) {
    while (tile < end) {
      step(zs0, xs0, zs1, xs1);
      if (tile >= end) break;
      step(zs1, xs1, zs0, xs0);
    }
    const bool last = end >= nfull;
    // The partial last tile belongs to the row group next in turn.  It is
    // staged through registers: rows past B are zero in both images.
    if (last && B % LWG_ROWS != 0 && nfull % groups == grp) {
      __syncthreads();
      const int64_t row0 = (int64_t)nfull * LWG_ROWS;
      ZI::fill_tail(dz, zs0, row0, B, t, No, slot0, nslots);
      XI::fill_tail(x, xs0, row0, B, t);
      __syncthreads();
      mma(zs0, xs0);
    }
    flush(end);
    if (last) break;
    end = nfull;
  }
}

// Smallest measured batch: from it up the kernel beat the split-K route of
// gemm.hip in every run at (No, Ki) = (784, 256), and at each batch measured
// for (784, 128), (784, 64) and (1000, 256); below it, and for every other
// shape, nothing is measured (profiles/linear_wgrad_wide.md).
#define LWW_MIN_BATCH 2048

// 1 when the kernel can compute (No, Ki, B) at all
extern "C" int linear_wgrad_wide_can_run(int No, int Ki, int64_t B) {
  return (Ki == 64 || Ki == 128 || Ki == 256) && lwg_bounds_ok(No, B);
}

// 1 when linear_wgrad_into routes (No, Ki, B) here: layers that
// linear_wgrad.hip cannot hold (No > 256) from the measured batch up
extern "C" int linear_wgrad_wide_supported(int No, int Ki, int64_t B) {
  return linear_wgrad_wide_can_run(No, Ki, B) && No > 256 && B >= LWW_MIN_BATCH;
}

// max_blocks > 0 caps the blocks per column tile, i.e. the row groups (tests
// force many tiles per block with it).  dz and x must be 16-byte aligned.
// Serves any B >= 1; the batch threshold is the router's business.
extern "C" hipError_t launch_linear_wgrad_wide(const bf16raw* dz, const bf16raw* x, float* dw,
                                               float* db, int64_t B, int No, int Ki,
                                               int max_blocks, int num_cus, hipStream_t stream) {
  if (!linear_wgrad_wide_can_run(No, Ki, B)) return hipErrorInvalidValue;
  if ((((uintptr_t)dz) | ((uintptr_t)x)) & 15) return hipErrorInvalidValue;
  // two resident blocks per CU
  const lwg_grid g = lwg_grid_plan(No, B, 2, max_blocks, num_cus);
  lwg_dispatch<1, 2, 4>(Ki / 64, g.nf, [&](auto mf, auto nf) {
    linear_wgrad_wide_kernel<decltype(mf)::value, decltype(nf)::value>
        <<<g.groups * g.ncol, LWW_THREADS, 0, stream>>>(dz, x, dw, db, (int)B, No, g.ncol,
                                                        g.groups, g.xcd_deal);
  });
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
