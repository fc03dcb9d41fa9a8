// Whole-MLP inference in one launch: bf16 rows x[M,K0] go through L hidden
// layers h_l = relu(h_{l-1} W_l^T + b_l) and a small head
// logits = h_L W_h^T + b_h (C <= 16 classes); the kernel writes each row's
// class id (int32 argmax of the bf16 logits) and, when asked, the logits.
// Hidden activations never reach global memory.
//
// The per-layer route (linear_stream.hip / gemm.hip per layer, logits to the
// host, numpy argmax) moves 1568 + 4 x 512 + 20 bytes per row at 784-256-256-10;
// this one reads x once and writes 4 bytes.
//
//   * A persistent block of 8 waves (2 x 4, a 64x64 sub-tile each, as
//     linear_stream.hip) owns 128-row tiles and ALL columns of every layer.
//   * Layer 1 is linear_stream_kernel's forward k-loop in arithmetic: A and W
//     go global->LDS by DMA in 32-deep slabs (mfma_tile.h's k-major image),
//     one fp32 accumulator per output, K ascending in 32-wide MFMA steps, K
//     tail and rows past M zero-filled.  With 158 KB of LDS a CU holds ONE
//     block, so the rings are deeper than linear_stream's: A (from HBM) runs
//     four slabs ahead through a ring of five, W (from L2) two ahead through
//     a ring of three, and a counted vmcnt wait leaves everything newer than
//     the next step's slabs in flight across the step's one barrier.
//   * The epilogue (+bias, relu, bf16 rounding, in mfma_tile.h's order)
//     stores into an LDS activation image [128][256] whose 16 B k-slots are
//     XOR-swizzled by row: a ds_read_b128 of it (mt_ld_frag) IS the next
//     layer's A fragment.
//   * Layers 2..L read A from the image (all of K resident) and stream W_l
//     through the same W ring; the accumulators hold the whole output, so
//     after the k-loop's closing barrier the epilogue overwrites the image in
//     place.
//   * The head is mfma_tile.h's small-head forward: one wave per 16 rows, w
//     as k-ascending B fragments in registers, lane (class l15, q) receives
//     the logits of rows q*4 .. q*4+3, f32_to_bf16(lg + bias).
//   * argmax over the C live lanes by 16-wide shuffles of an integer key made
//     from the bf16 bits (sign-magnitude -> ordered, NaN forced to the top)
//     with 15 - class in the low bits: the lowest index wins ties and the
//     first NaN wins, as np.argmax; no float compare for -ffast-math to bend.
//   * The A ring is separate from the image, so once layer 1's k-loop is done
//     the block puts the first four A slabs of its NEXT tile in flight and
//     the HBM stream continues under the hidden layers; the next layer's
//     first two W slabs are issued before each epilogue.  Biases live in LDS
//     so the epilogue issues no vector-memory load that would have to wait
//     behind those DMAs.
//
// Every fragment carries mfma_tile.h's k-packing and K ascends, so the
// logits are bit-identical to the per-layer linear_fwd chain.
//
// LDS: 40 KB A ring + 48 KB W ring + 64 KB image + 4 KB biases = 156 KB, one
// block per CU.  Widths 64 / 128 / 192 leave wave columns idle in that layer
// (they still help staging).

#include "mfma_tile.h"

#define MP_THREADS 512
#define MP_WAVES 8
#define MP_BM 128
#define MP_BN 256  // widest layer; the image's row stride
#define MP_BK 32
#define MP_NA 5  // A ring: slab s + 4 is issued in step s
#define MP_NW 3  // W ring: slab s + 2 is issued in step s
#define MP_MAX_HIDDEN 4
#define MP_CMAX 16

struct MlpPredictArgs {
  const bf16raw* x;
  const bf16raw* w[MP_MAX_HIDDEN + 1];  // hidden layers, then the head
  const float* b[MP_MAX_HIDDEN + 1];    // nullptr = no bias
  int n[MP_MAX_HIDDEN];                 // hidden widths
  int L, K0, C, M;
  int* classes;
  bf16raw* logits;  // nullptr = not wanted
};

// DMA instructions a wave issues per slab
#define MP_A_DMA (MP_BM * MP_BK * 2 / 1024 / MP_WAVES)
#define MP_W_DMA (MP_BN * MP_BK * 2 / 1024 / MP_WAVES)

// End of a step: the wave's memory instructions other than its newest
// `newer` have completed (vmcnt retires in order) and so have its LDS reads
// and writes; then the block's barrier.  __syncthreads() would drain the
// DMAs that are meant to stay in flight.
__device__ __forceinline__ void mp_publish(int newer) {
  static_assert(MP_A_DMA == 1 && MP_W_DMA == 2, "the cases below are written for these counts");
  switch (newer) {
    case 4: mt_wait_barrier<4>(); break;
    case 3: mt_wait_barrier<3>(); break;
    case 2: mt_wait_barrier<2>(); break;
    case 1: mt_wait_barrier<1>(); break;
    default: mt_wait_barrier<0>(); break;
  }
}

__global__ __launch_bounds__(MP_THREADS, 2) void mlp_predict_kernel(const MlpPredictArgs p) {
  constexpr int BKT = MP_BK;
  constexpr int SLOTS = BKT / 8;
  constexpr int A_EL = MP_BM * BKT, B_EL = MP_BN * BKT;
  constexpr int IMG_XM = 15;  // image slot ^= row & 15 (32 slots a row)
  constexpr int IMG_EL = MP_BM * MP_BN;
  constexpr int SB_EL = MP_MAX_HIDDEN * MP_BN * 2;  // hidden biases, in bf16 units
  // one array: the A ring, the W ring, the activation image and the biases
  __shared__ __attribute__((aligned(16)))
  bf16raw smem[MP_NA * A_EL + MP_NW * B_EL + IMG_EL + SB_EL];
  bf16raw* const a_ring = smem;
  bf16raw* const b_ring = smem + MP_NA * A_EL;
  bf16raw* const img = smem + MP_NA * A_EL + MP_NW * B_EL;
  float* const sbias = (float*)(smem + MP_NA * A_EL + MP_NW * B_EL + IMG_EL);

  const int t = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int wr = wid >> 2, wc = wid & 3;
  const int l15 = lane & 15, kg = lane >> 4;
  const int M = p.M, L = p.L, K0 = p.K0, C = p.C;
  const int ntiles = (int)ceil_div_i64(M, MP_BM);

  // biases of the hidden layers -> LDS (published by the first barrier below)
  for (int l = 0; l < L; ++l)
    if (p.b[l] != nullptr)
      for (int n = t; n < p.n[l]; n += MP_THREADS) sbias[l * MP_BN + n] = p.b[l][n];

  // head: w as the B operand (N = class, k ascending: lane (class l15, kg)
  // holds k = ks*32 + kg*8 .. +7) and the lane's bias
  const int H = p.n[L - 1];
  const bf16raw* const wh = p.w[L];
  mt_frag_t wk[MP_BN / 32];
  mt_head_w_frags(wk, wh, H, C, l15, kg);
  const bool head_bias = p.b[L] != nullptr;
  float bias_c = 0.f;
  if (head_bias && l15 < C) bias_c = p.b[L][l15];

  // x slab kt of the tile at m0 -> ring slot; true when it went by DMA
  // (MP_A_DMA instructions per wave, in flight)
  auto stage_a = [&](int slot, int64_t m0, int kt) -> bool {
    bf16raw* an = a_ring + slot * A_EL;
    if (m0 + MP_BM <= M && kt + BKT <= K0) {
      mt_dma_kmajor<MP_WAVES, MP_BM, BKT, true>(p.x, an, m0, MP_BM, K0, kt, wid, lane);
      return true;
    }
    mt_fill_kmajor<MP_THREADS, MP_BM, BKT>(p.x, an, m0, M, K0, kt, K0, t);
    return false;
  };
  // W[N][K] slab kt -> ring slot; true when it went by DMA (MP_W_DMA per wave)
  auto stage_b = [&](int slot, const bf16raw* W, int N, int K, int kt) -> bool {
    bf16raw* bn = b_ring + slot * B_EL;
    if (kt + BKT <= K) {
      mt_dma_kmajor<MP_WAVES, MP_BN, BKT, true>(W, bn, 0, N, K, kt, wid, lane);
      return true;
    }
    mt_fill_kmajor<MP_THREADS, MP_BN, BKT>(W, bn, 0, N, K, kt, K, t);
    return false;
  };

  floatx4 acc[4][4];
  auto zero_acc = [&]() {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = floatx4{0.f, 0.f, 0.f, 0.f};
  };

  // one 32-wide MFMA step of the wave's 64x64 sub-tile; A fragments from a
  // staged slab (ab) or, for ab == nullptr, from columns kt.. of the image
  auto mma = [&](const bf16raw* ab, const bf16raw* bb, int kt, bool from_img, bool active) {
    if (!active) return;
    mt_frag_t a[4], b[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int row = wr * 64 + mi * 16 + l15;
      if (from_img)
        a[mi] = mt_ld_frag<MP_BN, IMG_XM>(img, row, (kt >> 3) + kg);
      else
        a[mi] = mt_ld_frag<BKT, SLOTS - 1>(ab, row, kg);
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int rowb = wc * 64 + ni * 16 + l15;
      b[ni] = mt_ld_frag<BKT, SLOTS - 1>(bb, rowb, kg);
    }
    mt_mma_tile(acc, a, b);
  };

  // acc -> relu(acc + bias) as bf16 into the image (mt_epi_slice's rounding
  // order; the store differs, so it stays here).  Accumulator element r of
  // lane (l15, kg) is row mi*16 + kg*4 + r, column ni*16 + l15 of the wave's
  // sub-tile: 16 lanes write 32 contiguous bytes and the four lane groups
  // land 64 B apart, so the 2-byte stores are conflict-free.
  auto epilogue = [&](int l, bool has_bias) {
    const float* bl = sbias + l * MP_BN;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int col = wc * 64 + ni * 16 + l15;
      const float bv = has_bias ? bl[col] : 0.f;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wr * 64 + mi * 16 + kg * 4 + r;
          float val = acc[mi][ni][r];
          if (has_bias) val += bv;
          val = fmaxf(val, 0.f);
          img[row * MP_BN + ((((col >> 3) ^ (row & IMG_XM)) << 3) | (col & 7))] = f32_to_bf16(val);
        }
    }
  };

  bool staged = false;  // this tile's first A and W_1 slabs are already issued
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t m0 = (int64_t)tile * MP_BM;
    const int next = tile + gridDim.x;
    const int64_t m0_next = (int64_t)next * MP_BM;

    // ---- layer 1: x from HBM ----
    {
      const bf16raw* W = p.w[0];
      const int N = p.n[0], K = K0;
      const bool active = wc * 64 < N;
      zero_acc();
      if (!staged) {
#pragma unroll
        for (int j = 0; j < MP_NA - 1; ++j)
          if (j * BKT < K) stage_a(j, m0, j * BKT);
#pragma unroll
        for (int j = 0; j < MP_NW - 1; ++j)
          if (j * BKT < K) stage_b(j, W, N, K, j * BKT);
      }  // else: issued under the tile before, which also waited for them
      mp_publish(0);
      // Step on slab kt (ring slots ia / ib): issue W(kt+2) THEN A(kt+4) into
      // the slots that the step before was the last to read (its barrier
      // closed them), multiply, publish.  The next step needs W(kt+1), issued
      // in the step before this one after that step's A; what may stay in
      // flight is whatever was issued after it: that A slab and this step's
      // two issues.
      int ia = 0, ib = 0;
      bool a_prev = false;
      for (int kt = 0; kt < K; kt += BKT) {
        int newer = a_prev ? MP_A_DMA : 0;
        if (kt + (MP_NW - 1) * BKT < K) {
          const int slot = ib == 0 ? MP_NW - 1 : ib - 1;
          if (stage_b(slot, W, N, K, kt + (MP_NW - 1) * BKT)) newer += MP_W_DMA;
        }
        a_prev = false;
        if (kt + (MP_NA - 1) * BKT < K) {
          const int slot = ia == 0 ? MP_NA - 1 : ia - 1;
          a_prev = stage_a(slot, m0, kt + (MP_NA - 1) * BKT);
          if (a_prev) newer += MP_A_DMA;
        }
        mma(a_ring + ia * A_EL, b_ring + ib * B_EL, kt, false, active);
        mp_publish(newer);
        ia = ia == MP_NA - 1 ? 0 : ia + 1;
        ib = ib == MP_NW - 1 ? 0 : ib + 1;
      }
    }
    // Every ring slot is idle (closing barrier above).  The next tile's first
    // A slabs go in flight now and land under the hidden layers.
    if (next < ntiles) {
#pragma unroll
      for (int j = 0; j < MP_NA - 1; ++j)
        if (j * BKT < K0) stage_a(j, m0_next, j * BKT);
    }

    // ---- epilogue of layer l, then layer l + 1 from the image ----
    for (int l = 0; l < L; ++l) {
      const int Nl = p.n[l];
      // first W slabs of what comes next: layer l + 1, or layer 1 of the next tile
      if (l + 1 < L) {
#pragma unroll
        for (int j = 0; j < MP_NW - 1; ++j)
          if (j * BKT < Nl) stage_b(j, p.w[l + 1], p.n[l + 1], Nl, j * BKT);
      } else if (next < ntiles) {
#pragma unroll
        for (int j = 0; j < MP_NW - 1; ++j)
          if (j * BKT < K0) stage_b(j, p.w[0], p.n[0], K0, j * BKT);
      }
      if (wc * 64 < Nl) epilogue(l, p.b[l] != nullptr);
      // the image is complete, the W slabs (and the A slabs) have landed
      mp_publish(0);
      if (l + 1 < L) {
        const bf16raw* W = p.w[l + 1];
        const int N = p.n[l + 1], K = Nl;
        const bool active = wc * 64 < N;
        zero_acc();
        int ib = 0;
        for (int kt = 0; kt < K; kt += BKT) {
          int newer = 0;
          if (kt + (MP_NW - 1) * BKT < K) {
            const int slot = ib == 0 ? MP_NW - 1 : ib - 1;
            if (stage_b(slot, W, N, K, kt + (MP_NW - 1) * BKT)) newer = MP_W_DMA;
          }
          mma(nullptr, b_ring + ib * B_EL, kt, true, active);
          mp_publish(newer);
          ib = ib == MP_NW - 1 ? 0 : ib + 1;
        }
      }
    }

    // ---- head: logits of rows wid*16 .. +15 from the image, argmax ----
    {
      const int arow = wid * 16 + l15;
      const floatx4 lg = mt_head_logits<MP_BN / 32, MP_BN, IMG_XM>(wk, img, arow, H, kg);
      // lane (class l15, kg), element r <-> tile row wid*16 + kg*4 + r
      int best[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bf16raw xb = f32_to_bf16(head_bias ? lg[r] + bias_c : lg[r]);
        const int64_t grow = m0 + wid * 16 + kg * 4 + r;
        if (p.logits != nullptr && grow < M && l15 < C) p.logits[grow * C + l15] = xb;
        // ordered integer key of the bf16 value: -x < -0 == +0 < +x < NaN
        const int mag = xb & 0x7FFF;
        int key = (xb & 0x8000) ? 0x8000 - mag : 0x8000 + mag;
        if (mag > 0x7F80) key = 0x1FFFF;
        int comb = l15 < C ? ((key << 4) | (15 - l15)) : -1;
#pragma unroll
        for (int off = 8; off; off >>= 1) {
          const int o = __shfl_xor(comb, off, 16);
          comb = o > comb ? o : comb;
        }
        best[r] = 15 - (comb & 15);
      }
      if (l15 < 4) {
        const int64_t grow = m0 + wid * 16 + kg * 4 + l15;
        const int v = l15 == 0 ? best[0] : l15 == 1 ? best[1] : l15 == 2 ? best[2] : best[3];
        if (grow < M) p.classes[grow] = v;
      }
    }
    // The next tile's layer-1 barriers separate these image reads from its
    // first image write.
    staged = next < ntiles;
  }
}

static bool mp_width_ok(int n) { return n == 64 || n == 128 || n == 192 || n == 256; }

// 1 when the kernel serves x[M,K0] -> widths[0..L-1] -> C classes
extern "C" int mlp_predict_supported(int K0, const int* widths, int L, int C, int64_t M) {
  if (L < 1 || L > MP_MAX_HIDDEN || widths == nullptr) return 0;
  for (int l = 0; l < L; ++l)
    if (!mp_width_ok(widths[l])) return 0;
  return K0 >= 8 && K0 % 8 == 0 && C >= 2 && C <= MP_CMAX && M >= 1 && M < (1LL << 31) - MP_BM;
}

// Rows from which MnistMLPFused.forward routes an inference batch here: the
// smallest M at which tools/mlp_predict_bench.hip measured the fused launch
// not slower than the three launches it replaces at 784-256-256-10
// (profiles/mlp_predict.md, "Threshold").
#define MP_MIN_ROWS 4096
extern "C" int64_t mlp_predict_min_rows() { return MP_MIN_ROWS; }

// w / b: L hidden layers then the head (b entries may be null); max_blocks > 0
// caps the persistent grid (tests force several tiles per block with it).
// All pointers 16-byte aligned.
extern "C" hipError_t launch_mlp_predict(const bf16raw* x, const bf16raw* const* w,
                                         const float* const* b, const int* widths, int L, int K0,
                                         int C, int64_t M, int* classes, bf16raw* logits,
                                         int max_blocks, int num_cus, hipStream_t stream) {
  if (!mlp_predict_supported(K0, widths, L, C, M)) return hipErrorInvalidValue;
  if (x == nullptr || classes == nullptr || w == nullptr || b == nullptr)
    return hipErrorInvalidValue;
  uintptr_t bits = (uintptr_t)x | (uintptr_t)classes | (uintptr_t)logits;
  MlpPredictArgs a = {};
  a.x = x;
  for (int l = 0; l <= L; ++l) {
    if (w[l] == nullptr) return hipErrorInvalidValue;
    a.w[l] = w[l];
    a.b[l] = b[l];
    bits |= (uintptr_t)w[l] | (uintptr_t)b[l];
    if (l < L) a.n[l] = widths[l];
  }
  if (bits & 15) return hipErrorInvalidValue;
  a.L = L;
  a.K0 = K0;
  a.C = C;
  a.M = (int)M;
  a.classes = classes;
  a.logits = logits;
  const int64_t ntiles = ceil_div_i64(M, MP_BM);
  int64_t grid = num_cus > 0 ? num_cus : 256;  // 156 KB of LDS: one block per CU
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  if (grid > ntiles) grid = ntiles;
  mlp_predict_kernel<<<dim3((unsigned)grid), dim3(MP_THREADS), 0, stream>>>(a);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
