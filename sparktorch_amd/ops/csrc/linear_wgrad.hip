// Batch-streaming weight/bias gradient of a Linear layer with a huge batch:
//
//   dw[No, Ki] += dz[B, No]^T @ x[B, Ki]     fp32, accumulate
//   db[No]     += colsum(dz)                 fp32, accumulate, optional
//
// dz and x are bf16, row-major, contiguous.  The reduction runs over the
// batch rows, the OUTER stride of both operands, so both MFMA operands need
// a transpose.  gemm.hip's split-K route does that through registers with
// 16-bit LDS stores, needs a dead 256-wide tile for the bias column and
// combines 1168 partial tiles with atomics; here
//
//   * a block owns ALL No rows of dW times one column tile of x (112 or 128
//     columns: 784 = 7 x 112 exactly), so x is read once chip-wide and dz
//     once per column tile;
//   * the grid is persistent: (column tiles) x (row groups) resident blocks,
//     each walking the 32-row batch tiles of its row group with its dW / db
//     accumulators in registers and flushing with fp32 atomicAdd at the end
//     (and once half-way when the walk is long, to halve the fp32 chain);
//   * both tiles go global->LDS by DMA exactly as they lie in memory
//     (double-buffered, one barrier per tile); 16 B slots are XOR-swizzled
//     by row so the transposing LDS read (ds_read_b64_tr_b16; lane semantics
//     in profiles/bench_resnet18_optimization_log.md, "TR-mode wgrad")
//     that builds both k-packed MFMA fragments is bank-conflict free;
//   * db is a ones-fragment MFMA on the dz fragments in the blocks of column
//     tile 0;
//   * the column tiles of one row group share an XCD: their dz re-reads hit
//     that XCD's L2.
//
// Rows past B: the (at most one) partial tile is staged through registers
// with zero fill after the DMA loop over the full tiles.  Columns past Ki in
// the last column tile are clamped into the row and never flushed.
//
// The images, the block deal, the walk's plan, the dW / db accumulate and flush
// and the grid plan are linear_wgrad_tile.h's, shared with
// linear_wgrad_wide.hip (the mirror image, for No > 256) and hidden_bwd.hip
// (this decomposition with a hidden layer's masked dgrad added).

#include "launchers.h"
#include "linear_wgrad_tile.h"

#define LWG_THREADS 256

// MF: 16-row dW fragments per wave (No = 64 * MF); NF: 16-column fragments
// of the x tile (tile width 16 * NF)
template <int MF, int NF>
__global__ __launch_bounds__(LWG_THREADS, 2) void linear_wgrad_kernel(
    const bf16raw* __restrict__ dz, const bf16raw* __restrict__ x, float* __restrict__ dw,
    float* __restrict__ db, int B, int Ki, int ncol, int groups, int xcd_deal) {
  constexpr int NO = 64 * MF;
  constexpr int ZSLOTS = NO / 8;                  // 16 B slots per dz image row
  constexpr int XSLOTS = LWG_XCOLS / 8;
  using ZI = lwg_row_image<ZSLOTS, LWG_THREADS / 64>;    // dz: whole rows
  using XI = lwg_slice_image<XSLOTS, LWG_THREADS / 64>;  // x: the block's column tile
  static_assert(MF == 1 || MF == 2 || MF == 4, "No must be 64, 128 or 256");
  static_assert(NF >= 1 && NF * 16 <= LWG_XCOLS, "x tile wider than its image");

  // One LDS variable per buffer, selected at compile time (the tile loop is
  // unrolled by two): the compiler can then tell the DMA into one pair from
  // the fragment reads of the other and does not wait for the prefetch
  // before them.
  __shared__ __attribute__((aligned(16))) bf16raw zs0[LWG_ROWS * NO];
  __shared__ __attribute__((aligned(16))) bf16raw zs1[LWG_ROWS * NO];
  __shared__ __attribute__((aligned(16))) bf16raw xs0[LWG_ROWS * LWG_XCOLS];
  __shared__ __attribute__((aligned(16))) bf16raw xs1[LWG_ROWS * LWG_XCOLS];

  const int t = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int l15 = lane & 15, q = lane >> 4;

  int grp, ct;
  lwg_block_deal(ncol, xcd_deal, grp, ct);
  const int nfull = B / LWG_ROWS;   // full tiles: DMA, no bounds to check
  const int kslots = Ki >> 3;       // 16 B slots per x row
  const int slot0 = ct * (NF * 2);  // first slot of this column tile

  const unsigned zoff = ZI::lane_off(wid, lane);
  const unsigned xoff = XI::lane_off(wid, lane, Ki, slot0, kslots);
  auto stage = [&](bf16raw* zn, bf16raw* xn, int tile) {
    const int64_t row0 = (int64_t)tile * LWG_ROWS;
    ZI::dma(dz, zn, row0, zoff, wid);
    XI::dma(x, xn, row0, xoff, wid, Ki);
  };

  mt_frag_t ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (short)MT_BF16_ONE;

  floatx4 acc[MF][NF] = {};
  floatx4 accb[MF] = {};
  const bool do_db = db != nullptr && ct == 0;

  auto mma = [&](const bf16raw* zb, const bf16raw* xb) {
    lwg_accumulate<MF, NF, ZSLOTS>(acc, accb, zb, xb, ones, do_db, wid, q, l15);
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
  auto flush = [&](int seg_end) {
    lwg_flush<MF, NF>(acc, accb, dw, db, Ki, ct, do_db, seg_end, wid, q, l15);
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
      ZI::fill_tail(dz, zs0, row0, B, t);
      XI::fill_tail(x, xs0, row0, B, t, Ki, slot0, kslots);
      __syncthreads();
      mma(zs0, xs0);
    }
    flush(end);
    if (last) break;
    end = nfull;
  }
}

// Smallest batch at which the kernel was measured against the split-K route
// of gemm.hip (and won at both flagship shapes); below it that route stays
// (profiles/bench_resnet18_optimization_log.md, "Streaming wgrad").
#define LWG_MIN_BATCH 32768

// 1 when the kernel can compute (No, Ki, B) at all
extern "C" int linear_wgrad_stream_can_run(int No, int Ki, int64_t B) {
  return (No == 64 || No == 128 || No == 256) && lwg_bounds_ok(Ki, B);
}

// 1 when linear_wgrad_into / linear_wgrad_bias_into route (No, Ki, B) here
extern "C" int linear_wgrad_stream_supported(int No, int Ki, int64_t B) {
  return linear_wgrad_stream_can_run(No, Ki, B) && B >= LWG_MIN_BATCH;
}

// max_blocks > 0 caps the blocks per column tile, i.e. the row groups (tests
// force many tiles per block with it).  dz and x must be 16-byte aligned.
// Serves any B >= 1; the batch threshold is the router's business.
extern "C" hipError_t launch_linear_wgrad_stream(const bf16raw* dz, const bf16raw* x, float* dw,
                                                 float* db, int64_t B, int No, int Ki,
                                                 int max_blocks, int num_cus, hipStream_t stream) {
  if (!linear_wgrad_stream_can_run(No, Ki, B)) return hipErrorInvalidValue;
  if ((((uintptr_t)dz) | ((uintptr_t)x)) & 15) return hipErrorInvalidValue;
  // two resident blocks per CU
  const lwg_grid g = lwg_grid_plan(Ki, B, 2, max_blocks, num_cus);
  lwg_dispatch<1, 2, 4>(No / 64, g.nf, [&](auto mf, auto nf) {
    linear_wgrad_kernel<decltype(mf)::value, decltype(nf)::value>
        <<<g.groups * g.ncol, LWG_THREADS, 0, stream>>>(dz, x, dw, db, (int)B, Ki, g.ncol,
                                                        g.groups, g.xcd_deal);
  });
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
