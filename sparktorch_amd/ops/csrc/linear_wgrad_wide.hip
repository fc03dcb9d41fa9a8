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
//   * block ids are dealt so the column tiles of one row group share an XCD
//     and start together: their x re-reads hit that XCD's L2.
//
// Rows past B: the (at most one) partial tile is staged through registers
// with zero fill after the DMA loop over the full tiles.  Columns past No in
// the last column tile are clamped to the row's last 16 B slot; their dW rows
// and db entries are never flushed (MFMA output rows are independent).

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
  constexpr int XCH = LWG_ROWS * KI * 2 / 1024;   // 1 KB DMA chunks per x tile
  constexpr int ZCH = LWG_ROWS * LWG_XCOLS * 2 / 1024;
  constexpr int NB = (NF + 3) / 4;                // db fragments per wave
  static_assert(MF == 1 || MF == 2 || MF == 4, "Ki must be 64, 128 or 256");
  static_assert(NF >= 1 && NF * 16 <= LWG_XCOLS, "dz tile wider than its image");
  static_assert(XCH % 4 == 0 && ZCH % 4 == 0, "DMA chunks are dealt evenly to the 4 waves");

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
  const int nslots = No >> 3;       // 16 B slots per dz row
  const int slot0 = ct * (NF * 2);  // first slot of this column tile
  const int row_base = ct * (NF * 16);  // and its first row of dW

  // DMA source offsets.  Wave w issues chunks w, w + 4, ...: chunk c fills
  // image rows c * RPC ... + RPC - 1, so a lane's row advances by a multiple
  // of 8 from one of its chunks to the next, its swizzle key stays, and one
  // 32-bit lane offset (plus a wave-uniform base) serves all of them.
  constexpr int XRPC = 64 / XSLOTS, ZRPC = 64 / ZSLOTS;
  static_assert(XCH == 4 || (4 * XRPC) % 8 == 0, "key must not depend on the chunk");
  static_assert((4 * ZRPC) % 8 == 0, "key must not depend on the chunk");
  const int xr0 = wid * XRPC + lane / XSLOTS;
  const unsigned xoff = xr0 * KI + (((lane % XSLOTS) ^ lwg_key<XSLOTS>::key(xr0)) << 3);
  const int zr0 = wid * ZRPC + lane / ZSLOTS;
  int zgs = slot0 + ((lane % ZSLOTS) ^ lwg_key<ZSLOTS>::key(zr0));
  if (zgs > nslots - 1) zgs = nslots - 1;
  const unsigned zoff = (unsigned)zr0 * No + zgs * 8;

  auto stage = [&](bf16raw* zn, bf16raw* xn, int tile) {
    const int64_t row0 = (int64_t)tile * LWG_ROWS;
#pragma unroll
    for (int i = 0; i < ZCH / 4; ++i) {
      const bf16raw* g = dz + (row0 + i * 4 * ZRPC) * No;
      mt_glds16(g + zoff, zn + (wid + 4 * i) * 512);
    }
#pragma unroll
    for (int i = 0; i < XCH / 4; ++i) {
      const bf16raw* g = x + (row0 + i * 4 * XRPC) * KI;
      mt_glds16(g + xoff, xn + (wid + 4 * i) * 512);
    }
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
      for (int j = 0; j < LWG_ROWS * ZSLOTS / LWW_THREADS; ++j) {
        const int u = t + j * LWW_THREADS;
        const int row = u / ZSLOTS;
        int gs = slot0 + ((u % ZSLOTS) ^ lwg_key<ZSLOTS>::key(row));
        if (gs > nslots - 1) gs = nslots - 1;
        shortx8 v = {};
        if (row0 + row < B) v = *(const shortx8*)(dz + (row0 + row) * No + gs * 8);
        *(shortx8*)(zs0 + u * 8) = v;
      }
#pragma unroll
      for (int j = 0; j < MF; ++j) {
        const int u = t + j * LWW_THREADS;
        const int row = u / XSLOTS;
        const int slot = (u % XSLOTS) ^ lwg_key<XSLOTS>::key(row);
        shortx8 v = {};
        if (row0 + row < B) v = *(const shortx8*)(x + (row0 + row) * KI + slot * 8);
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

// Smallest measured batch: from it up the kernel beat the split-K route of
// gemm.hip in every run at (No, Ki) = (784, 256), and at each batch measured
// for (784, 128), (784, 64) and (1000, 256); below it, and for every other
// shape, nothing is measured (profiles/linear_wgrad_wide.md).
#define LWW_MIN_BATCH 2048

// 1 when the kernel can compute (No, Ki, B) at all
extern "C" int linear_wgrad_wide_can_run(int No, int Ki, int64_t B) {
  return (Ki == 64 || Ki == 128 || Ki == 256) && No >= 8 && (No & 7) == 0 && No < (1 << 24) &&
         B >= 1 && B < (1LL << 31) - LWG_ROWS;
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
  const int nf = lwg_nf(No);
  const int ncol = (No + nf * 16 - 1) / (nf * 16);
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
  const dim3 grid(groups * ncol), block(LWW_THREADS);
#define LWW_LAUNCH(MF, NF)                                                                      \
  linear_wgrad_wide_kernel<MF, NF><<<grid, block, 0, stream>>>(dz, x, dw, db, (int)B, No, ncol, \
                                                               groups, xcd_deal)
#define LWW_LAUNCH_NF(MF) \
  do {                    \
    if (nf == 7)          \
      LWW_LAUNCH(MF, 7);  \
    else                  \
      LWW_LAUNCH(MF, 8);  \
  } while (0)
  switch (Ki) {
    case 64: LWW_LAUNCH_NF(1); break;
    case 128: LWW_LAUNCH_NF(2); break;
    default: LWW_LAUNCH_NF(4); break;
  }
#undef LWW_LAUNCH_NF
#undef LWW_LAUNCH
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
