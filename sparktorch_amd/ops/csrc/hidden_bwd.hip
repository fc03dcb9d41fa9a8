// One-pass backward of a hidden Linear layer W[No][Ki] whose input x[B][Ki] is
// a ReLU output, for a huge batch:
//
//   dz_in[B, Ki] = (dz[B, No] @ W) * (x > 0)    bf16
//   dw[No, Ki]  += dz^T @ x                     fp32, accumulate
//   db[No]      += colsum(dz)                   fp32, accumulate, optional
//
// linear_stream.hip's masked dgrad and linear_wgrad.hip's dW+db each read dz
// and x from HBM; this kernel reads them once for both.  It is
// linear_wgrad_kernel's decomposition with the dgrad added:
//
//   * a block owns all No rows of dW times one 112/128-column tile `ct` of x
//     and walks the 32-row batch tiles of its row group, persistent, dW / db
//     in registers, flushed by fp32 atomicAdd at the end and once half-way
//     through a long walk; the column tiles of a row group share an XCD.
//     That is linear_wgrad_kernel's contract, rule for rule, and each rule is
//     linear_wgrad_tile.h's code: the images, the block deal, the walk's plan,
//     the dW / db accumulate and flush, the grid plan;
//   * the full-width dz tile and the ct slice of x that the block stages for
//     dW are the operands of dz_in[rows, ct] = dz[rows, :] @ W[:, ct] and its
//     mask as well.  Wave w owns output columns 16w .. 16w+15 of the slice:
//     its W[:, those 16] sits in registers for the whole walk as k-packed B
//     fragments (No / 32 of them), the A fragments are 16 B reads of the dz
//     image along its rows, the mask is read from the x image;
//   * one fp32 accumulator per dz_in element, the reduction over No ascending
//     in 32-wide MFMA steps with mfma_tile.h's k-packing, rounded to bf16 and
//     then zeroed where x <= 0: bit-identical to linear_stream_kernel's and
//     gemm_kernel's EPI_BF16_MASK;
//   * 8 waves, one block per CU (64 dW accumulator registers a lane at No =
//     256).  With no second block to hide latency the tiles run two ahead
//     through a ring of three image sets, the newest left in flight across
//     the step's barrier by a counted vmcnt wait (as linear_stream.hip's A
//     ring);
//   * the dz_in tile goes through LDS so that every lane stores 16 B of one
//     row; the store is issued at the start of the next step, behind the
//     barrier that step needs anyway.
//
// Rows past B: the partial last tile is staged through registers with zero
// fill and its dz_in rows past B are not stored.  Columns past Ki in the last
// column tile: W fragments are zero, x slots are clamped into the row, and
// neither dW nor dz_in is stored there.
//
// Built without packed fp32 instructions (ops/build.py).

#include "launchers.h"
#include "linear_wgrad_tile.h"

#define HB_THREADS 512
#define HB_WAVES 8
#define HB_OPAD (LWG_XCOLS + 8)  // dz_in tile row stride: lanes 4 rows apart miss each other's banks

// RF: 16-row dW fragments per wave (No = 128 * RF); NF: 16-column fragments
// of the x tile (tile width 16 * NF)
template <int RF, int NF>
__global__ __launch_bounds__(HB_THREADS, 1) void hidden_bwd_kernel(
    const bf16raw* __restrict__ dz, const bf16raw* __restrict__ x, const bf16raw* __restrict__ w,
    bf16raw* __restrict__ dzin, float* __restrict__ dw, float* __restrict__ db, int B, int Ki,
    int ncol, int groups, int xcd_deal) {
  constexpr int NO = 128 * RF;
  constexpr int KS = NO / 32;  // MFMA k-steps of the dgrad
  constexpr int ZSLOTS = NO / 8;
  constexpr int XSLOTS = LWG_XCOLS / 8;
  constexpr int Z_EL = LWG_ROWS * NO, X_EL = LWG_ROWS * LWG_XCOLS, O_EL = LWG_ROWS * HB_OPAD;
  using ZI = lwg_row_image<ZSLOTS, HB_WAVES>;    // dz: whole rows
  using XI = lwg_slice_image<XSLOTS, HB_WAVES>;  // x: the block's column tile
  // DMA instructions a wave issues for one tile
  constexpr int Z_DMA = ZI::DMA, X_DMA = XI::DMA;
  static_assert(RF == 1 || RF == 2, "No must be 128 or 256");
  static_assert(NF >= 1 && NF <= HB_WAVES && NF * 16 <= LWG_XCOLS, "one wave per dz_in fragment");
  static_assert(Z_DMA >= 1 && X_DMA == 1, "every wave stages part of both images");
  static_assert(LWG_ROWS * XSLOTS == HB_THREADS, "one 16 B dz_in store per thread");

  // One LDS variable per buffer, each named at compile time in the unrolled
  // tile loop: the compiler can then tell the DMA into one set from the
  // fragment reads of another and does not wait for the prefetch before them.
  __shared__ __attribute__((aligned(16))) bf16raw zs0[Z_EL];
  __shared__ __attribute__((aligned(16))) bf16raw zs1[Z_EL];
  __shared__ __attribute__((aligned(16))) bf16raw zs2[Z_EL];
  __shared__ __attribute__((aligned(16))) bf16raw xs0[X_EL];
  __shared__ __attribute__((aligned(16))) bf16raw xs1[X_EL];
  __shared__ __attribute__((aligned(16))) bf16raw xs2[X_EL];
  __shared__ __attribute__((aligned(16))) bf16raw os0[O_EL];
  __shared__ __attribute__((aligned(16))) bf16raw os1[O_EL];
  __shared__ __attribute__((aligned(16))) bf16raw os2[O_EL];

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
  // End of a step: the tile after this one has landed in every wave's share
  // and every wave is done with this one.  The tile staged in this step is
  // each wave's newest Z_DMA + X_DMA memory instructions at least (the dz_in
  // store is issued before them) and stays in flight.
  auto publish = [&](bool in_flight) {
    if (in_flight)
      mt_wait_barrier<Z_DMA + X_DMA>();
    else
      mt_wait_barrier<0>();
  };

  // W[:, ct slice column 16 wid + l15] as the dgrad's B fragments: lane
  // (l15, q) holds k = 32 ks + 8 q .. + 7
  const bool dg_wave = wid < NF;
  mt_frag_t wk[KS];
  {
    const int wcol = ct * (NF * 16) + wid * 16 + l15;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      wk[ks] = mt_frag_t{};
      if (dg_wave && wcol < Ki) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          wk[ks][j] = (short)w[(int64_t)(ks * 32 + q * 8 + j) * Ki + wcol];
      }
    }
  }

  mt_frag_t ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (short)MT_BF16_ONE;

  floatx4 acc[RF][NF] = {};
  floatx4 accb[RF] = {};
  const bool do_db = db != nullptr && ct == 0;

  // dW / db: wave w owns dW rows 16 RF w .. + 16 RF - 1
  auto mma = [&](const bf16raw* zb, const bf16raw* xb) {
    lwg_accumulate<RF, NF, ZSLOTS>(acc, accb, zb, xb, ones, do_db, wid, q, l15);
  };

  // dz_in[32 rows][16 wid .. + 15] of the tile in (zb, xb) -> ob, bf16.
  // Accumulator lane (l15, q), element r <-> tile row 16 mi + 4 q + r,
  // column 16 wid + l15.
  auto dgrad = [&](const bf16raw* zb, const bf16raw* xb, bf16raw* ob) {
    if (!dg_wave) return;
    const int col = wid * 16 + l15;
    bf16raw m[2][4];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mi * 16 + q * 4 + r;
        m[mi][r] =
            xb[row * LWG_XCOLS + ((((col >> 3) ^ lwg_key<XSLOTS>::key(row)) << 3) | (col & 7))];
      }
    }
    floatx4 d[2] = {};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int row = mi * 16 + l15;
        const mt_frag_t a = *(const mt_frag_t*)&zb[row * NO + (((ks * 4 + q) ^
                                                                 lwg_key<ZSLOTS>::key(row)) << 3)];
        d[mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wk[ks], d[mi], 0, 0, 0);
      }
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        bf16raw o = f32_to_bf16(d[mi][r]);
        if (!(bf16_to_f32(m[mi][r]) > 0.f)) o = 0;
        ob[(mi * 16 + q * 4 + r) * HB_OPAD + col] = o;
      }
    }
  };

  // thread t stores 16 B: row t / 16 of the tile, slot t % 16 of the slice
  auto store = [&](const bf16raw* ob, int tile) {
    const int row = t >> 4, slot = t & 15;
    const int64_t grow = (int64_t)tile * LWG_ROWS + row;
    const int col = ct * (NF * 16) + slot * 8;
    if (slot < NF * 2 && col < Ki && grow < B)
      *(shortx8*)(dzin + grow * Ki + col) = *(const shortx8*)(ob + row * HB_OPAD + slot * 8);
  };

  int tile = grp;
  // One full tile.  On entry it has landed in (zb, xb) and every wave is done
  // with the step before, whose dz_in tile lies in op and whose images
  // (zp, xp) are free: they take the block's tile after next.
  auto step = [&](const bf16raw* zb, const bf16raw* xb, bf16raw* ob, bf16raw* zp, bf16raw* xp,
                  const bf16raw* op) {
    if (tile > grp) store(op, tile - groups);
    const int ahead = tile + 2 * groups;
    const bool in_flight = ahead < nfull;
    if (in_flight) stage(zp, xp, ahead);
    mma(zb, xb);
    dgrad(zb, xb, ob);
    publish(in_flight);
    tile += groups;
  };
  auto flush = [&](int seg_end) {
    lwg_flush<RF, NF>(acc, accb, dw, db, Ki, ct, do_db, seg_end, wid, q, l15);
  };

  // the half-way flush comes after a multiple of three tiles, so the ring
  // keeps its turn
  const int my_tiles = lwg_my_tiles(grp, groups, nfull);
  const int half = lwg_half_walk<3>(my_tiles);
  int end = half ? grp + half * groups : nfull;
  if (tile < nfull) {
    stage(zs0, xs0, tile);
    const bool in_flight = tile + groups < nfull;
    if (in_flight) stage(zs1, xs1, tile + groups);
    publish(in_flight);
  }
  for (;;) {
    for (;;) {
      if (tile >= end) break;
      step(zs0, xs0, os0, zs2, xs2, os2);
      if (tile >= end) break;
      step(zs1, xs1, os1, zs0, xs0, os0);
      if (tile >= end) break;
      step(zs2, xs2, os2, zs1, xs1, os1);
    }
    const bool last = end >= nfull;
    if (last) {
      // the last full tile's dz_in is still in LDS (its step's barrier is behind)
      if (my_tiles > 0) {
        const int s = (my_tiles - 1) % 3;
        store(s == 0 ? os0 : (s == 1 ? os1 : os2), tile - groups);
      }
      // The partial last tile belongs to the row group next in turn.  It is
      // staged through registers: rows past B are zero in both images.
      if (B % LWG_ROWS != 0 && nfull % groups == grp) {
        __syncthreads();  // the store above has read os0 if that was its tile
        const int64_t row0 = (int64_t)nfull * LWG_ROWS;
        // written out, not ZI / XI::fill_tail: through the helpers this kernel's
        // register count crosses an occupancy step
        // (profiles/wgrad_family_refactor.md)
#pragma unroll
        for (int j = 0; j < LWG_ROWS * ZSLOTS / HB_THREADS; ++j) {
          const int u = t + j * HB_THREADS;
          const int row = u / ZSLOTS;
          const int slot = (u % ZSLOTS) ^ lwg_key<ZSLOTS>::key(row);
          shortx8 v = {};
          if (row0 + row < B) v = *(const shortx8*)(dz + (row0 + row) * NO + slot * 8);
          *(shortx8*)(zs0 + u * 8) = v;
        }
        {
          const int row = t / XSLOTS;
          int gs = slot0 + ((t % XSLOTS) ^ lwg_key<XSLOTS>::key(row));
          if (gs > kslots - 1) gs = kslots - 1;
          shortx8 v = {};
          if (row0 + row < B) v = *(const shortx8*)(x + (row0 + row) * Ki + gs * 8);
          *(shortx8*)(xs0 + t * 8) = v;
        }
        __syncthreads();
        mma(zs0, xs0);
        dgrad(zs0, xs0, os0);
        __syncthreads();
        store(os0, nfull);
      }
    }
    flush(end);
    if (last) break;
    end = nfull;
  }
}

// Smallest batch at which tools/hidden_bwd_bench.hip measured this kernel not
// slower than the two launches it replaces at (No, Ki) = (256, 256)
// (profiles/hidden_bwd.md, "Threshold"); below it those two stay.
#define HB_MIN_BATCH 131072

// 1 when the kernel can compute (No, Ki, B) at all
extern "C" int hidden_bwd_can_run(int No, int Ki, int64_t B) {
  return (No == 128 || No == 256) && lwg_bounds_ok(Ki, B);
}

// 1 when functional.py routes (No, Ki, B) here
extern "C" int hidden_bwd_supported(int No, int Ki, int64_t B) {
  return hidden_bwd_can_run(No, Ki, B) && B >= HB_MIN_BATCH;
}

// w is the bf16 weight [No][Ki]; dzin receives [B][Ki].  max_blocks > 0 caps
// the blocks per column tile, i.e. the row groups (tests force many tiles per
// block with it).  dz, x and dzin must be 16-byte aligned.  Serves any
// B >= 1; the batch threshold is the router's business.
extern "C" hipError_t launch_hidden_bwd(const bf16raw* dz, const bf16raw* x, const bf16raw* w,
                                        bf16raw* dzin, float* dw, float* db, int64_t B, int No,
                                        int Ki, int max_blocks, int num_cus, hipStream_t stream) {
  if (!hidden_bwd_can_run(No, Ki, B)) return hipErrorInvalidValue;
  if ((((uintptr_t)dz) | ((uintptr_t)x) | ((uintptr_t)dzin)) & 15) return hipErrorInvalidValue;
  // one resident block per CU
  const lwg_grid g = lwg_grid_plan(Ki, B, 1, max_blocks, num_cus);
  lwg_dispatch<1, 2>(No / 128, g.nf, [&](auto rf, auto nf) {
    hidden_bwd_kernel<decltype(rf)::value, decltype(nf)::value>
        <<<g.groups * g.ncol, HB_THREADS, 0, stream>>>(dz, x, w, dzin, dw, db, (int)B, Ki, g.ncol,
                                                       g.groups, g.xcd_deal);
  });
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
