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
//     tile 0 — no virtual column, no extra tile;
//   * block ids are dealt so the column tiles of one row group share an XCD
//     and start together: their dz re-reads hit that XCD's L2.
//
// Rows past B: the (at most one) partial tile is staged through registers
// with zero fill after the DMA loop over the full tiles.  Columns past Ki in
// the last column tile are clamped to the row's last 16 B slot and are never
// flushed (MFMA output columns are independent).

#include "mfma_tile.h"

#define LWG_THREADS 256
#define LWG_ROWS 32    // batch rows per tile = one 16x16x32 k-step
#define LWG_SPLIT_TILES 64  // register chains this long (2048 rows) are flushed half-way
#define LWG_XCOLS 128  // x image row: 16 slots of 16 B (NF = 7 leaves two unused)

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

// MF: 16-row dW fragments per wave (No = 64 * MF); NF: 16-column fragments
// of the x tile (tile width 16 * NF)
template <int MF, int NF>
__global__ __launch_bounds__(LWG_THREADS, 2) void linear_wgrad_kernel(
    const bf16raw* __restrict__ dz, const bf16raw* __restrict__ x, float* __restrict__ dw,
    float* __restrict__ db, int B, int Ki, int ncol, int groups, int xcd_deal) {
  constexpr int NO = 64 * MF;
  constexpr int ZSLOTS = NO / 8;                  // 16 B slots per dz image row
  constexpr int XSLOTS = LWG_XCOLS / 8;
  constexpr int ZCH = LWG_ROWS * NO * 2 / 1024;   // 1 KB DMA chunks per dz tile
  constexpr int XCH = LWG_ROWS * LWG_XCOLS * 2 / 1024;
  static_assert(MF == 1 || MF == 2 || MF == 4, "No must be 64, 128 or 256");
  static_assert(NF >= 1 && NF * 16 <= LWG_XCOLS, "x tile wider than its image");
  static_assert(ZCH % 4 == 0 && XCH % 4 == 0, "DMA chunks are dealt evenly to the 4 waves");

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

  // block id -> (row group, column tile).  Hardware deals consecutive ids
  // round-robin over the 8 XCDs; with xcd_deal the ncol blocks of a group
  // are consecutive slots of ONE XCD.
  int grp, ct;
  if (xcd_deal) {
    const int xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
    grp = (j / ncol) * 8 + xcd;
    ct = j % ncol;
  } else {
    grp = blockIdx.x / ncol;
    ct = blockIdx.x % ncol;
  }
  const int nfull = B / LWG_ROWS;   // full tiles: DMA, no bounds to check
  const int kslots = Ki >> 3;       // 16 B slots per x row
  const int slot0 = ct * (NF * 2);  // first slot of this column tile

  // DMA source offsets.  Wave w issues chunks w, w + 4, ...: chunk c fills
  // image rows c * RPC ... + RPC - 1, so a lane's row advances by a multiple
  // of 8 from one of its chunks to the next, its swizzle key stays, and one
  // 32-bit lane offset (plus a wave-uniform base) serves all of them.
  constexpr int ZRPC = 64 / ZSLOTS, XRPC = 64 / XSLOTS;
  static_assert((4 * ZRPC) % 8 == 0 && (4 * XRPC) % 8 == 0, "key must not depend on the chunk");
  const int zr0 = wid * ZRPC + lane / ZSLOTS;
  const unsigned zoff = zr0 * NO + (((lane % ZSLOTS) ^ lwg_key<ZSLOTS>::key(zr0)) << 3);
  const int xr0 = wid * XRPC + lane / XSLOTS;
  int xgs = slot0 + ((lane % XSLOTS) ^ lwg_key<XSLOTS>::key(xr0));
  if (xgs > kslots - 1) xgs = kslots - 1;
  const unsigned xoff = xr0 * Ki + xgs * 8;

  auto stage = [&](bf16raw* zn, bf16raw* xn, int tile) {
    const int64_t row0 = (int64_t)tile * LWG_ROWS;
#pragma unroll
    for (int i = 0; i < ZCH / 4; ++i) {
      const bf16raw* g = dz + (row0 + i * 4 * ZRPC) * NO;
      mt_glds16(g + zoff, zn + (wid + 4 * i) * 512);
    }
#pragma unroll
    for (int i = 0; i < XCH / 4; ++i) {
      const bf16raw* g = x + (row0 + i * 4 * XRPC) * Ki;
      mt_glds16(g + xoff, xn + (wid + 4 * i) * 512);
    }
  };

  mt_frag_t ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (short)MT_BF16_ONE;

  floatx4 acc[MF][NF] = {};
  floatx4 accb[MF] = {};
  const bool do_db = db != nullptr && ct == 0;

  auto mma = [&](const bf16raw* zb, const bf16raw* xb) {
    mt_frag_t az[MF];
#pragma unroll
    for (int a = 0; a < MF; ++a)
      az[a] = lwg_tr_frag<ZSLOTS>(zb, q, l15, (wid * MF + a) * 16);
    if (do_db) {
#pragma unroll
      for (int a = 0; a < MF; ++a)
        accb[a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az[a], ones, accb[a], 0, 0, 0);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const mt_frag_t bx = lwg_tr_frag<XSLOTS>(xb, q, l15, f * 16);
#pragma unroll
      for (int a = 0; a < MF; ++a)
        acc[a][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(az[a], bx, acc[a][f], 0, 0, 0);
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
  // column l15 of the fragment (16 lanes = one 64 B segment)
  auto flush = [&](int seg_end) {
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
  };

  // A block with LWG_SPLIT_TILES or more tiles flushes once half-way (after
  // an even count, so the buffer pairs keep their turn): fp32 rounding grows
  // with the length and magnitude of one accumulator chain, and the extra
  // flush halves both for the price of one more pass of atomics.
  const int my_tiles = grp < nfull ? (nfull - grp + groups - 1) / groups : 0;
  const int half = my_tiles >= LWG_SPLIT_TILES ? (((my_tiles + 1) / 2 + 1) & ~1) : 0;
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
#pragma unroll
      for (int j = 0; j < MF; ++j) {
        const int u = t + j * LWG_THREADS;
        const int row = u / ZSLOTS;
        const int slot = (u % ZSLOTS) ^ lwg_key<ZSLOTS>::key(row);
        shortx8 v = {};
        if (row0 + row < B) v = *(const shortx8*)(dz + (row0 + row) * NO + slot * 8);
        *(shortx8*)(zs0 + u * 8) = v;
      }
#pragma unroll
      for (int j = 0; j < LWG_ROWS * XSLOTS / LWG_THREADS; ++j) {
        const int u = t + j * LWG_THREADS;
        const int row = u / XSLOTS;
        int gs = slot0 + ((u % XSLOTS) ^ lwg_key<XSLOTS>::key(row));
        if (gs > kslots - 1) gs = kslots - 1;
        shortx8 v = {};
        if (row0 + row < B) v = *(const shortx8*)(x + (row0 + row) * Ki + gs * 8);
        *(shortx8*)(xs0 + u * 8) = v;
      }
      __syncthreads();
      mma(zs0, xs0);
    }
    flush(end);
    if (last) break;
    end = nfull;
  }
}

// x tile width in 16-column fragments: the one of {7, 8} that covers Ki with
// fewer dead columns (784 = 7 x 112; 256 = 2 x 128)
static int lwg_nf(int Ki) {
  const int c7 = (Ki + 111) / 112 * 112, c8 = (Ki + 127) / 128 * 128;
  return c7 < c8 ? 7 : 8;
}

// Smallest batch at which the kernel was measured against the split-K route
// of gemm.hip (and won at both flagship shapes); below it that route stays
// (profiles/bench_resnet18_optimization_log.md, "Streaming wgrad").
#define LWG_MIN_BATCH 32768
#define LWG_MIN_TILES 16

// 1 when the kernel can compute (No, Ki, B) at all
extern "C" int linear_wgrad_stream_can_run(int No, int Ki, int64_t B) {
  return (No == 64 || No == 128 || No == 256) && Ki >= 8 && (Ki & 7) == 0 && Ki < (1 << 24) &&
         B >= 1 && B < (1LL << 31) - LWG_ROWS;
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
  const int nf = lwg_nf(Ki);
  const int ncol = (Ki + nf * 16 - 1) / (nf * 16);
  const int ntiles = (int)((B + LWG_ROWS - 1) / LWG_ROWS);
  // two resident blocks per CU
  int groups = 2 * (num_cus > 0 ? num_cus : 256) / ncol;
  if (groups < 1) groups = 1;
  // at least LWG_MIN_TILES tiles (512 rows, the split-K route's floor per
  // slice) per block: fewer, longer register chains and fewer flushes
  if (groups > ntiles / LWG_MIN_TILES) groups = ntiles / LWG_MIN_TILES;
  if (groups < 1) groups = 1;
  if (max_blocks > 0 && groups > max_blocks) groups = max_blocks;
  int xcd_deal = 0;
  if (groups >= 8) {
    groups &= ~7;
    xcd_deal = 1;
  }
  const dim3 grid(groups * ncol), block(LWG_THREADS);
#define LWG_LAUNCH(MF, NF)                                                                  \
  linear_wgrad_kernel<MF, NF><<<grid, block, 0, stream>>>(dz, x, dw, db, (int)B, Ki, ncol, \
                                                          groups, xcd_deal)
#define LWG_LAUNCH_NF(MF) \
  do {                    \
    if (nf == 7)          \
      LWG_LAUNCH(MF, 7);  \
    else                  \
      LWG_LAUNCH(MF, 8);  \
  } while (0)
  switch (No) {
    case 64: LWG_LAUNCH_NF(1); break;
    case 128: LWG_LAUNCH_NF(2); break;
    default: LWG_LAUNCH_NF(4); break;
  }
#undef LWG_LAUNCH_NF
#undef LWG_LAUNCH
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
