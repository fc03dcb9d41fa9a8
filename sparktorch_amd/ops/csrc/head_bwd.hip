// One-pass backward of a small classifier head (C <= 16 classes) that sits
// on a ReLU layer:  logits = y_in @ w^T,  y_in = relu(...)  [B, H] bf16.
//
//   dz_in = (dz_out @ w) * (y_in > 0)     bf16 [B, H]
//   dw   += dz_out^T @ y_in               fp32 [C, H]
//   db   += colsum(dz_out)                fp32 [C]
//
// The three-kernel route (wgrad GEMM with 10 live rows in a 128-row MFMA
// tile, K=10 dgrad GEMM, relu_bwd) reads y_in twice and writes + re-reads the
// unmasked dgrad; here y_in is read once and dz_in written once.
//
// Persistent blocks stride over ROWS-row tiles of y_in.  A tile is staged by
// async global->LDS DMA (double-buffered: tile t+1 is in flight while tile t
// is consumed; one barrier per tile) into a pad-free row-major image whose
// 16 B slots are XOR-swizzled by row (mfma_tile.h's k-major image, one slab as
// wide as H).  The image is used twice:
//   * dgrad computes dz_in^T = w^T[H,C] x dz_out^T[C,rows] so a lane's
//     accumulators are consecutive h of ONE row; two MFMAs whose M-rows are
//     interleaved in groups of four give each lane 8 consecutive h = one
//     16 B store, and the mask is the matching 16 B of the y_in image.
//   * wgrad computes dW^T[H,16] += y_in^T x dz_out over the tile rows.  The
//     k-packed fragments of the row-major image come from the transposing
//     LDS read (ds_read_b64_tr_b16; lane semantics in
//     profiles/bench_resnet18_optimization_log.md, "TR-mode wgrad"): every
//     lane of a 16-lane quarter passes the address of 4 consecutive columns
//     of one row and receives one column of the quarter's 4x16 block.
// dz_out's tile is tiny: it is staged through registers into a [rows][16]
// image with the class dimension zero-padded, read plainly (k-contiguous)
// by the dgrad and through the same transposing read by the wgrad.  Each
// wave owns 32-column groups of H for both products; w fragments and the
// dW/db accumulators stay in registers across all of a block's tiles and
// are flushed once with fp32 atomicAdd.
//
// head_ce_kernel runs the same tile loop for a train step under mean
// cross-entropy: it needs no dz_out from memory.  Once a y_in tile is in LDS
// it computes the tile's logits from that image (mfma_tile.h's small-head
// forward: one wave per 16 rows, w as a second set of register fragments),
// applies loss.hip's softmax / loss arithmetic per row and writes the bf16
// dlogits into the [rows][16] image itself; an LDS-only barrier publishes the
// image and the two stages above run unchanged.  The head's forward, the
// loss and the head's backward then read y_in once and the logits never reach
// HBM (profiles/head_ce.md).

#include "mfma_tile.h"

#define HEAD_THREADS 256
#define HEAD_CPAD 16  // class dim padded to 16 in the dz_out image

__host__ __device__ constexpr int head_rows(int H) { return H <= 256 ? 64 : 32; }

// slot ^= row & XM of the y_in image (0: the dz image is not swizzled)
template <int XM>
struct head_key {
  static __device__ __forceinline__ int key(int row) { return row & XM; }
};

// Tile loop shared by head_bwd_kernel (CE = false: the dz_out image is staged
// from global memory) and head_ce_kernel (CE = true: the image is computed
// from the resident y_in tile; dz_out is unused).
template <int H, bool CE>
__device__ __forceinline__ void head_tiles(
    const bf16raw* __restrict__ dz_out, const bf16raw* __restrict__ w,
    const bf16raw* __restrict__ y_in, bf16raw* __restrict__ dz_in, float* __restrict__ dw,
    float* __restrict__ db, int B, int C, const float* __restrict__ bias,
    const int64_t* __restrict__ tgt, float* __restrict__ loss, bf16raw* __restrict__ logits_out,
    float inv_B) {
  constexpr int ROWS = head_rows(H);
  constexpr int SLOTS = H / 8;                     // 16 B slots per image row
  constexpr int XM = (SLOTS % 16 == 0) ? 15 : 7;   // slot ^= row & XM
  constexpr int NP = H / 32;                       // 32-column groups
  constexpr int PW = (NP + 3) / 4;                 // groups per wave
  constexpr int NCH = ROWS * H * 2 / 1024;         // 1 KB DMA chunks per tile
  constexpr int EPT = ROWS * HEAD_CPAD / HEAD_THREADS;  // dz elements per thread
  static_assert(H % 64 == 0 && H <= 512, "unsupported H");

  __shared__ __attribute__((aligned(16))) bf16raw ys[2][ROWS * H];
  // CE fills and consumes the dz image inside one tile step: one buffer
  __shared__ __attribute__((aligned(16))) bf16raw dzs[CE ? 1 : 2][ROWS * HEAD_CPAD];

  const int t = threadIdx.x;
  const int wid = t >> 6, lane = t & 63;
  const int l15 = lane & 15, q = lane >> 4;
  const int ntiles = (B + ROWS - 1) / ROWS;

  // w fragments (dgrad A operand, M = h, K = class padded to 32).  M-row m of
  // fragment e of a group maps to h = group*32 + (m/4)*8 + e*4 + (m%4).
  mt_frag_t wf[PW][2];
#pragma unroll
  for (int pi = 0; pi < PW; ++pi) {
    const int p = wid + pi * 4;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int h = p * 32 + (l15 >> 2) * 8 + e * 4 + (l15 & 3);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int c = q * 8 + i;
        wf[pi][e][i] = (p < NP && c < C) ? (short)w[c * H + h] : (short)0;
      }
    }
  }
  mt_frag_t ones;
#pragma unroll
  for (int i = 0; i < 8; ++i) ones[i] = (short)MT_BF16_ONE;

  floatx4 accw[PW][2] = {};
  floatx4 accb = {0.f, 0.f, 0.f, 0.f};

  // CE: w again as the forward's B operand, the lane's bias, next tile's
  // targets and the block's loss
  mt_frag_t wk[H / 32];
  float bias_c = 0.f, lsum = 0.f;
  int tg[4] = {0, 0, 0, 0};
  if (CE) {
    mt_head_w_frags(wk, w, H, C, l15, q);
    if (bias != nullptr && l15 < C) bias_c = bias[l15];
  }
  // targets of the rows whose logits this lane receives (wave wid owns tile
  // rows wid*16 .. +15; accumulator element r <-> row wid*16 + q*4 + r)
  auto load_tgt = [&](int tile) {
    if (wid < ROWS / 16) {
      const int64_t gr = (int64_t)tile * ROWS + wid * 16 + q * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) tg[r] = (gr + r < B) ? (int)tgt[gr + r] : 0;
    }
  };

  // dz_out tile -> registers (class dim zero-padded, rows past B zero)
  const int zrow = (t * EPT) / HEAD_CPAD, zc0 = (t * EPT) % HEAD_CPAD;
  bf16raw zr[EPT];
  auto load_dz = [&](int tile) {
    const int64_t gr = (int64_t)tile * ROWS + zrow;
#pragma unroll
    for (int j = 0; j < EPT; ++j)
      zr[j] = (gr < B && zc0 + j < C) ? dz_out[gr * C + zc0 + j] : (bf16raw)0;
  };
  auto write_dz = [&](int b) {
#pragma unroll
    for (int j = 0; j < EPT; ++j) dzs[b][zrow * HEAD_CPAD + zc0 + j] = zr[j];
  };
  // y_in tile -> LDS by DMA; rows past B re-read row B-1 (their dz rows are
  // zero and their outputs are not stored)
  auto dma_y = [&](int b, int tile) {
#pragma unroll
    for (int c = wid; c < NCH; c += 4) {
      const int o = c * 1024 + lane * 16;
      const int row = o / (H * 2);
      const int slot = ((o % (H * 2)) >> 4) ^ (row & XM);
      int64_t gr = (int64_t)tile * ROWS + row;
      if (gr > B - 1) gr = B - 1;
      const bf16raw* g = y_in + gr * H + slot * 8;
      mt_glds16(g, ys[b] + c * 512);
    }
  };

  int tile = blockIdx.x;
  int buf = 0;
  if (tile < ntiles) {
    dma_y(0, tile);
    if (CE) {
      load_tgt(tile);
    } else {
      load_dz(tile);
      write_dz(0);
    }
  }
  for (; tile < ntiles; tile += gridDim.x) {
    // tile's images are complete and every wave is done with the other pair
    // (CE says so itself: each wave's DMA of this tile has landed)
    if (CE)
      mt_wait_barrier<0>();
    else
      __syncthreads();
    const int next = tile + gridDim.x;
    const bf16raw* yb = ys[buf];
    bf16raw* zb = dzs[CE ? 0 : buf];
    const int64_t row0 = (int64_t)tile * ROWS;
    if (CE) {
      int tc[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) tc[r] = tg[r];
      // The forward's y_in fragments are read before the next tile's DMA is
      // issued (LDS reads after it wait for it to land), so the logits and
      // the softmax run under the DMA.  H = 512 has no registers for that.
      constexpr bool EARLY = H <= 256;
      const bool fwd_wave = wid < ROWS / 16;  // one 16-row fragment per wave
      const int arow = wid * 16 + l15;
      mt_frag_t ay[H / 32];
      if (EARLY && fwd_wave) mt_head_a_frags<H / 32, H, XM>(ay, yb, arow, q);
      if (next < ntiles) {
        dma_y(buf ^ 1, next);
        load_tgt(next);
      }
      // ---- logits, softmax, loss and the dz image of this tile ----
      if (fwd_wave) {
#pragma clang fp reassociate(off)  // the class sums keep loss.hip's order
        const floatx4 lg = EARLY ? mt_head_logits(ay, wk)
                                 : mt_head_logits<H / 32, H, XM>(wk, yb, arow, H, q);
        // lane (class l15, q), element r <-> tile row wid*16 + q*4 + r.  The
        // per-row arithmetic is loss.hip's; RG rows go side by side so their
        // lane exchanges overlap (H = 512 has the registers for one).
        constexpr int RG = H <= 256 ? 4 : 1;
#pragma unroll
        for (int r0 = 0; r0 < 4; r0 += RG) {
          bf16raw xb[RG];
          float x[RG], mx[RG], e[RG], se[RG];
#pragma unroll
          for (int j = 0; j < RG; ++j) {
            xb[j] = f32_to_bf16(bias != nullptr ? lg[r0 + j] + bias_c : lg[r0 + j]);
            x[j] = bf16_to_f32(xb[j]);
            mx[j] = l15 < C ? fmaxf(-1e30f, x[j]) : -1e30f;
          }
#pragma unroll
          for (int off = 8; off; off >>= 1)
#pragma unroll
            for (int j = 0; j < RG; ++j) mx[j] = fmaxf(mx[j], __shfl_xor(mx[j], off, 16));
#pragma unroll
          for (int j = 0; j < RG; ++j) e[j] = l15 < C ? __expf(x[j] - mx[j]) : 0.f;
          if (B <= CE_WAVE_MAX_B) {  // ce_fused_wave_kernel's butterfly
#pragma unroll
            for (int j = 0; j < RG; ++j) se[j] = e[j];
#pragma unroll
            for (int off = 8; off; off >>= 1)
#pragma unroll
              for (int j = 0; j < RG; ++j) se[j] += __shfl_xor(se[j], off, 16);
          } else {  // ce_fused_kernel's class-ascending sum
#pragma unroll
            for (int j = 0; j < RG; ++j) se[j] = 0.f;
            for (int c = 0; c < C; ++c)
#pragma unroll
              for (int j = 0; j < RG; ++j) se[j] += __shfl(e[j], c, 16);
          }
#pragma unroll
          for (int j = 0; j < RG; ++j) {
            const int r = r0 + j;
            const int lrow = wid * 16 + q * 4 + r;
            const bool live = row0 + lrow < B;
            const float xt = __shfl(x[j], tc[r] & 15, 16);
            const float inv_se = 1.f / se[j];
            // the target class in one fma: loss.hip's kernels compile to it
            // under -ffast-math, and dz must keep their bits
            const float p =
                l15 == tc[r] ? __builtin_fmaf(e[j], inv_se, -1.f) : e[j] * inv_se;
            zb[lrow * HEAD_CPAD + l15] =
                (live && l15 < C) ? f32_to_bf16(p * inv_B) : (bf16raw)0;
            if (live && l15 == 0) lsum += (__logf(se[j]) + mx[j] - xt) * inv_B;
            if (logits_out != nullptr && live && l15 < C)
              logits_out[(row0 + lrow) * C + l15] = xb[j];
          }
        }
      }
      // publish the dz image; the next tile's DMA stays in flight
      mt_lds_barrier();
    } else if (next < ntiles) {
      load_dz(next);
      dma_y(buf ^ 1, next);
    }

    // ---- dgrad + mask ----
#pragma unroll
    for (int rf = 0; rf < ROWS / 16; ++rf) {
      const int row = rf * 16 + l15;
      mt_frag_t bz = {};
      if (q < 2) bz = mt_ld_frag<HEAD_CPAD, 0>(zb, row, q);
#pragma unroll
      for (int pi = 0; pi < PW; ++pi) {
        const int p = wid + pi * 4;
        if (p < NP) {
          floatx4 z = {0.f, 0.f, 0.f, 0.f};
          floatx4 a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[pi][0], bz, z, 0, 0, 0);
          floatx4 a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[pi][1], bz, z, 0, 0, 0);
          const int slot = p * 4 + q;
          const shortx8 mk = mt_ld_frag<H, XM>(yb, row, slot);
          shortx8 out;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            out[j] = bf16_to_f32((bf16raw)mk[j]) > 0.f ? (short)f32_to_bf16(a0[j]) : (short)0;
            out[4 + j] =
                bf16_to_f32((bf16raw)mk[4 + j]) > 0.f ? (short)f32_to_bf16(a1[j]) : (short)0;
          }
          if (row0 + row < B) *(shortx8*)(dz_in + (row0 + row) * H + slot * 8) = out;
        }
      }
    }

    // ---- wgrad + bias grad ----
#pragma unroll
    for (int ks = 0; ks < ROWS / 32; ++ks) {
      // fragment value i <-> tile row ks*32 + (i/4)*16 + q*4 + (i%4), the same
      // row order for both operands
      const mt_frag_t bz = mt_tr_frag<HEAD_CPAD, 4, 16, head_key<0>>(zb, ks * 32, q, l15, 0);
      if (wid == 0)
        accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bz, accb, 0, 0, 0);
#pragma unroll
      for (int pi = 0; pi < PW; ++pi) {
        const int p = wid + pi * 4;
        if (p < NP) {
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const mt_frag_t ay =
                mt_tr_frag<H, 4, 16, head_key<XM>>(yb, ks * 32, q, l15, p * 32 + e * 16);
            accw[pi][e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ay, bz, accw[pi][e], 0, 0, 0);
          }
        }
      }
    }

    if (!CE && next < ntiles) write_dz(buf ^ 1);
    buf ^= 1;
  }

  if (CE) {
    // one loss atomic per block
    __shared__ float lred[HEAD_THREADS / 64];
#pragma unroll
    for (int off = 32; off; off >>= 1) lsum += __shfl_xor(lsum, off, 64);
    if (lane == 0) lred[wid] = lsum;
    __syncthreads();
    if (t == 0) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < HEAD_THREADS / 64; ++i) s += lred[i];
      if (s != 0.f) atomicAdd(loss, s);
    }
  }

  // flush: accumulator lane (c = l15, q), element r <-> h = base + 4q + r
  if (l15 < C) {
#pragma unroll
    for (int pi = 0; pi < PW; ++pi) {
      const int p = wid + pi * 4;
      if (p < NP) {
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            atomicAdd(dw + l15 * H + p * 32 + e * 16 + q * 4 + r, accw[pi][e][r]);
      }
    }
    if (db != nullptr && wid == 0 && q == 0) atomicAdd(db + l15, accb[0]);
  }
}

template <int H>
__global__ __launch_bounds__(HEAD_THREADS, 2) void head_bwd_kernel(
    const bf16raw* __restrict__ dz_out, const bf16raw* __restrict__ w,
    const bf16raw* __restrict__ y_in, bf16raw* __restrict__ dz_in, float* __restrict__ dw,
    float* __restrict__ db, int B, int C) {
  head_tiles<H, false>(dz_out, w, y_in, dz_in, dw, db, B, C, nullptr, nullptr, nullptr, nullptr,
                       0.f);
}

// Head forward + cross-entropy (mean over B) + head backward in one pass:
// with logits = y_in @ w^T + bias rounded to bf16 (gemm_kernel's EPI_BIAS
// arithmetic) and dz_out = d loss / d logits as ce_fused produces it,
//   loss  += sum_b (lse_b - logit_b[t_b]) / B      (the launcher zeroes it)
//   dz_in, dw, db as head_bwd_kernel; logits_out (nullable) gets the logits.
template <int H>
__global__ __launch_bounds__(HEAD_THREADS, 2) void head_ce_kernel(
    const bf16raw* __restrict__ w, const float* __restrict__ bias,
    const bf16raw* __restrict__ y_in, const int64_t* __restrict__ tgt,
    bf16raw* __restrict__ dz_in, float* __restrict__ dw, float* __restrict__ db,
    float* __restrict__ loss, bf16raw* __restrict__ logits_out, int B, int C, float inv_B) {
  head_tiles<H, true>(nullptr, w, y_in, dz_in, dw, db, B, C, bias, tgt, loss, logits_out,
                      inv_B);
}

// 1 when (C, H) is served by the fused kernel
extern "C" int head_bwd_supported(int C, int H) {
  return C >= 1 && C <= HEAD_CPAD && (H == 64 || H == 128 || H == 256 || H == 512);
}

// max_blocks > 0 caps the grid (tests force several tiles per block with it)
extern "C" hipError_t launch_head_bwd(const bf16raw* dz_out, const bf16raw* w,
                                      const bf16raw* y_in, bf16raw* dz_in, float* dw, float* db,
                                      int B, int C, int H, int max_blocks, int num_cus,
                                      hipStream_t stream) {
  if (!head_bwd_supported(C, H) || B < 1) return hipErrorInvalidValue;
  const int ntiles = (B + head_rows(H) - 1) / head_rows(H);
  int grid = 2 * (num_cus > 0 ? num_cus : 256);
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  if (grid > ntiles) grid = ntiles;
#define HEAD_LAUNCH(HH)                                                                      \
  head_bwd_kernel<HH><<<dim3(grid), dim3(HEAD_THREADS), 0, stream>>>(dz_out, w, y_in, dz_in, dw, \
                                                                      db, B, C)
  switch (H) {
    case 64: HEAD_LAUNCH(64); break;
    case 128: HEAD_LAUNCH(128); break;
    case 256: HEAD_LAUNCH(256); break;
    default: HEAD_LAUNCH(512); break;
  }
#undef HEAD_LAUNCH
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}

// Same shape range and grid rule as launch_head_bwd.  loss is defined, not
// accumulated: it is zeroed on the stream first.
extern "C" hipError_t launch_head_ce(const bf16raw* w, const float* bias, const bf16raw* y_in,
                                     const int64_t* tgt, bf16raw* dz_in, float* dw, float* db,
                                     float* loss, bf16raw* logits_out, int B, int C, int H,
                                     int max_blocks, int num_cus, hipStream_t stream) {
  if (!head_bwd_supported(C, H) || B < 1) return hipErrorInvalidValue;
  const int ntiles = (B + head_rows(H) - 1) / head_rows(H);
  int grid = 2 * (num_cus > 0 ? num_cus : 256);
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  if (grid > ntiles) grid = ntiles;
  hipError_t err = hipMemsetAsync(loss, 0, sizeof(float), stream);
  if (err != hipSuccess) return err;
#define HEAD_CE_LAUNCH(HH)                                                    \
  head_ce_kernel<HH><<<dim3(grid), dim3(HEAD_THREADS), 0, stream>>>(          \
      w, bias, y_in, tgt, dz_in, dw, db, loss, logits_out, B, C, 1.0f / B)
  switch (H) {
    case 64: HEAD_CE_LAUNCH(64); break;
    case 128: HEAD_CE_LAUNCH(128); break;
    case 256: HEAD_CE_LAUNCH(256); break;
    default: HEAD_CE_LAUNCH(512); break;
  }
#undef HEAD_CE_LAUNCH
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
