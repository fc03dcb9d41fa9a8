// The last hidden layer's forward fused into the classifier head's loss pass:
// per 128-row tile, what linear_fwd(x, w2, b2, relu) followed by
// linear_head_ce(h2, w3, b3, labels, dw3, db3) compute,
//
//   h2     = relu(x @ w2^T + b2)                 bf16 [B, H]   (stays in LDS)
//   logits = h2 @ w3^T + b3                      bf16 [B, C]   (stays in registers)
//   loss   = mean cross-entropy(logits, labels)  fp32
//   dz2    = (dlogits @ w3) * (h2 > 0)           bf16 [B, H]
//   dw3   += dlogits^T @ h2,  db3 += colsum(dlogits)
//
// so the step reads x and the labels and writes dz2; h2's round trip through
// HBM (one write by the forward, one read by head_ce_kernel) is gone.
//
// Persistent blocks of 8 waves stride over 128-row tiles.  A tile runs
//
//   1. linear_stream_kernel's k-loop (K <= 256): x through a ring of three
//      32-deep slabs two ahead, w2 through a ring of two one ahead, both by
//      global->LDS DMA; one fp32 accumulator per output, K ascending in
//      32-wide MFMA steps; + bias, relu, round to bf16 as mfma_tile.h's
//      epilogue orders them: h2 has linear_stream_kernel's bits;
//   2. the bf16 tile goes from the accumulators into head_bwd.hip's y_in
//      image (row-major, 16 B slots XOR-swizzled by row), which aliases the
//      rings: they are dead once the k-loop's last barrier has passed;
//   3. head_ce_kernel's stages on that image: logits (one wave per 16 rows),
//      loss.hip's softmax / loss arithmetic per row, the bf16 dlogits into the
//      [rows][16] image, then dgrad + mask and wgrad + bias grad with each wave
//      on one 32-column group of H.  dz2 and the requested logits have
//      head_ce_kernel's bits; dw3 / db3 / the loss differ by the order of the
//      fp32 sums only.
//
// Two blocks share a CU (<= 76 KB of LDS each), so one block's head stages run
// under the other's k-loop.  w3's fragments live in LDS (8 KB at H = 256),
// not in registers as in head_ce_kernel: the GEMM's 64 accumulators are live
// at the same time.  Rows past B are staged as zeros; their h2 is
// relu(b2), finite, their dlogits are zero and nothing of them is stored.
// Measurements: profiles/hidden_head_ce.md.

#include "launchers.h"
#include "mfma_tile.h"

#define HH_THREADS 512
#define HH_WAVES 8
#define HH_BM 128   // rows per tile
#define HH_BK 32    // k-slab depth
#define HH_CPAD 16  // class dim padded to 16 in the dlogits image

struct hh_key0 {
  static __device__ __forceinline__ int key(int) { return 0; }
};
struct hh_key15 {
  static __device__ __forceinline__ int key(int row) { return row & 15; }
};

template <int H>
__global__ __launch_bounds__(HH_THREADS, 4) void hidden_head_ce_kernel(
    const bf16raw* __restrict__ x, const bf16raw* __restrict__ w2, const float* __restrict__ b2,
    const bf16raw* __restrict__ w3, const float* __restrict__ b3,
    const int64_t* __restrict__ tgt, bf16raw* __restrict__ dz_in, float* __restrict__ dw,
    float* __restrict__ db, float* __restrict__ loss, bf16raw* __restrict__ logits_out,
    bf16raw* __restrict__ h2_out, int B, int K, int C, float inv_B) {
  static_assert(H == 128 || H == 256, "unsupported H");
  constexpr int BKT = HH_BK;
  // the GEMM's wave grid: 64 output columns a wave, all H columns a block
  constexpr int WC = H / 64, WR = HH_WAVES / WC;
  constexpr int MF = HH_BM / WR / 16;  // 16-row fragments per wave
  constexpr int A_EL = HH_BM * BKT, B_EL = H * BKT;
  constexpr int RING_EL = 3 * A_EL + 2 * B_EL;
  constexpr int IMG_EL = HH_BM * H;
  constexpr int SLOTS = H / 8;  // 16 B slots per image row
  constexpr int XM = 15;        // slot ^= row & XM (head_bwd.hip's key at these H)
  constexpr int NP = H / 32;    // 32-column groups of the head stages
  constexpr int WPG = HH_WAVES / NP;  // waves per group: they split the tile's rows
  constexpr int NK = H / 32;          // k-steps of the logits
  // DMA instructions a wave issues for one x slab: publish() counts them
  constexpr int A_DMA = HH_BM * BKT * 2 / 1024 / HH_WAVES;
  static_assert(A_DMA == 1, "the counted wait below is written for this");
  static_assert(SLOTS % 16 == 0, "XM = 15 is head_bwd.hip's key only for these widths");

  // rings of the k-loop, then the h2 image
  __shared__ __attribute__((aligned(16))) bf16raw smem[IMG_EL > RING_EL ? IMG_EL : RING_EL];
  __shared__ __attribute__((aligned(16))) bf16raw dzs[HH_BM * HH_CPAD];
  // w3 as the logits' B fragments: entry ks * 64 + lane is lane's 8 values
  __shared__ __attribute__((aligned(16))) bf16raw w3s[NK * 64 * 8];
  __shared__ float lred[HH_WAVES];
  bf16raw* const a0 = smem;
  bf16raw* const a1 = smem + A_EL;
  bf16raw* const a2 = smem + 2 * A_EL;
  bf16raw* const r0 = smem + 3 * A_EL;
  bf16raw* const r1 = smem + 3 * A_EL + B_EL;
  bf16raw* const ys = smem;

  const int t = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = wid / WC, wc = wid % WC;
  int lane = t & 63;
  int l15 = lane & 15, q = lane >> 4;
  const int p = wid % NP, sub = wid / NP;  // head stages: column group, row share
  const int ntiles = (B + HH_BM - 1) / HH_BM;

  // w3 -> LDS (lane (class l15, q) of step ks holds k = ks*32 + q*8 .. +7;
  // classes at or past C are zero).  The k-loop's barriers publish it.
  for (int u = t; u < NK * 64; u += HH_THREADS) {
    const int ks = u >> 6, c = u & 15, kq = (u & 63) >> 4;
    shortx8 v = {};
    if (c < C) v = *(const shortx8*)&w3[c * H + ks * 32 + kq * 8];
    *(shortx8*)&w3s[u * 8] = v;
  }

  floatx4 accw[2] = {};
  floatx4 accb = {0.f, 0.f, 0.f, 0.f};
  float bias_c = 0.f, lsum = 0.f;
  if (b3 != nullptr && l15 < C) bias_c = b3[l15];
  const bool has_b2 = b2 != nullptr;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t m0 = (int64_t)tile * HH_BM;
    const bool rows_full = m0 + HH_BM <= B;
    // Everything below that depends on the lane alone is the same in every
    // tile; hoisted out of this loop it costs more registers than the kernel
    // has (the GEMM's accumulators are live), so the lane id is made opaque
    // here and each stage derives its addresses where it uses them.
    asm volatile("" : "+v"(lane));
    l15 = lane & 15;
    q = lane >> 4;
    const int tt = wid * 64 + lane;  // threadIdx.x, as opaque

    // ---- h2 tile: linear_stream_kernel's k-loop ----
    // true when the slab went by DMA (A_DMA instructions per wave, in flight)
    auto stage_a = [&](bf16raw* an, int kt) -> bool {
      if (rows_full) {
        mt_dma_kmajor<HH_WAVES, HH_BM, BKT, false>(x, an, m0, HH_BM, K, kt, wid, lane);
        return true;
      }
      mt_fill_kmajor<HH_THREADS, HH_BM, BKT>(x, an, m0, B, K, kt, K, tt);
      return false;
    };
    auto stage_b = [&](bf16raw* bn, int kt) {
      mt_dma_kmajor<HH_WAVES, H, BKT, false>(w2, bn, 0, H, K, kt, wid, lane);
    };
    // an x slab staged two ahead by DMA is each wave's LAST A_DMA memory
    // instructions and stays in flight across the barrier
    auto publish = [&](bool a_in_flight) {
      if (a_in_flight)
        mt_wait_barrier<A_DMA>();
      else
        mt_wait_barrier<0>();
    };
    floatx4 acc[MF][4] = {};
    auto step = [&](const bf16raw* ab, const bf16raw* bb, bf16raw* bn, bf16raw* an2, int kt) {
      if (kt + BKT < K) stage_b(bn, kt + BKT);
      bool a_in_flight = false;
      if (kt + 2 * BKT < K) a_in_flight = stage_a(an2, kt + 2 * BKT);
      mt_frag_t a[MF], b[4];
#pragma unroll
      for (int mi = 0; mi < MF; ++mi)
        a[mi] = mt_ld_frag<BKT, BKT / 8 - 1>(ab, wr * (MF * 16) + mi * 16 + l15, q);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        b[ni] = mt_ld_frag<BKT, BKT / 8 - 1>(bb, wc * 64 + ni * 16 + l15, q);
      mt_mma_tile(acc, a, b);
      publish(a_in_flight);
    };

    stage_a(a0, 0);
    stage_b(r0, 0);
    publish(BKT < K ? stage_a(a1, BKT) : false);
    // the rings return to (a0, r0) every six slabs; buffers are compile-time
    // constants in each step (linear_stream.hip)
    for (int kt = 0;; kt += 6 * BKT) {
      step(a0, r0, r1, a2, kt);
      if (kt + 1 * BKT >= K) break;
      step(a1, r1, r0, a0, kt + 1 * BKT);
      if (kt + 2 * BKT >= K) break;
      step(a2, r0, r1, a1, kt + 2 * BKT);
      if (kt + 3 * BKT >= K) break;
      step(a0, r1, r0, a2, kt + 3 * BKT);
      if (kt + 4 * BKT >= K) break;
      step(a1, r0, r1, a0, kt + 4 * BKT);
      if (kt + 5 * BKT >= K) break;
      step(a2, r1, r0, a1, kt + 5 * BKT);
      if (kt + 6 * BKT >= K) break;
    }

    // class ids of the rows whose logits this lane receives (wave wid owns
    // tile rows wid*16 .. +15; accumulator element r <-> row wid*16 + q*4 + r)
    // (fetched here, after the k-loop, so they land under the image's stores
    // without holding registers through the GEMM)
    int tc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t gr = m0 + wid * 16 + q * 4 + r;
      tc[r] = gr < B ? (int)tgt[gr] : 0;
    }

    // ---- + bias, relu, round: the tile into the y_in image ----
    // The last step waited for everything and its barrier left the rings
    // idle.  Accumulator element r of (mi, ni) <-> tile row
    // wr*MF*16 + mi*16 + q*4 + r, column wc*64 + ni*16 + l15.
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int col = wc * 64 + ni * 16 + l15;
      const float bv = has_b2 ? b2[col] : 0.f;
#pragma unroll
      for (int mi = 0; mi < MF; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wr * (MF * 16) + mi * 16 + q * 4 + r;
          float val = acc[mi][ni][r];
          if (has_b2) val += bv;
          val = fmaxf(val, 0.f);
          ys[row * H + (((col >> 3) ^ (row & XM)) << 3) + (col & 7)] = f32_to_bf16(val);
        }
    }
    mt_lds_barrier();

    if (h2_out != nullptr) {
#pragma unroll
      for (int u = tt; u < HH_BM * SLOTS; u += HH_THREADS) {
        const int row = u / SLOTS, slot = u % SLOTS;
        if (m0 + row < B)
          *(shortx8*)(h2_out + (m0 + row) * H + slot * 8) = mt_ld_frag<H, XM>(ys, row, slot);
      }
    }

    // ---- logits, softmax, loss and the dlogits image (head_ce_kernel) ----
    {
#pragma clang fp reassociate(off)  // the class sums keep loss.hip's order
      const int arow = wid * 16 + l15;
      floatx4 lg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        const mt_frag_t ay = mt_ld_frag<H, XM>(ys, arow, ks * 4 + q);
        const mt_frag_t wk = *(const mt_frag_t*)&w3s[(ks * 64 + lane) * 8];
        lg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ay, wk, lg, 0, 0, 0);
      }
      // lane (class l15, q), element r <-> tile row wid*16 + q*4 + r.  The
      // per-row arithmetic is loss.hip's; the four rows go side by side so
      // their lane exchanges overlap.
      bf16raw xb[4];
      float xv[4], mx[4], e[4], se[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xb[j] = f32_to_bf16(b3 != nullptr ? lg[j] + bias_c : lg[j]);
        xv[j] = bf16_to_f32(xb[j]);
        mx[j] = l15 < C ? fmaxf(-1e30f, xv[j]) : -1e30f;
      }
#pragma unroll
      for (int off = 8; off; off >>= 1)
#pragma unroll
        for (int j = 0; j < 4; ++j) mx[j] = fmaxf(mx[j], __shfl_xor(mx[j], off, 16));
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = l15 < C ? __expf(xv[j] - mx[j]) : 0.f;
      if (B <= CE_WAVE_MAX_B) {  // ce_fused_wave_kernel's butterfly
#pragma unroll
        for (int j = 0; j < 4; ++j) se[j] = e[j];
#pragma unroll
        for (int off = 8; off; off >>= 1)
#pragma unroll
          for (int j = 0; j < 4; ++j) se[j] += __shfl_xor(se[j], off, 16);
      } else {  // ce_fused_kernel's class-ascending sum
#pragma unroll
        for (int j = 0; j < 4; ++j) se[j] = 0.f;
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int j = 0; j < 4; ++j) se[j] += __shfl(e[j], c, 16);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int lrow = wid * 16 + q * 4 + j;
        const bool live = m0 + lrow < B;
        const float xt = __shfl(xv[j], tc[j] & 15, 16);
        const float inv_se = 1.f / se[j];
        // the target class in one fma: loss.hip's kernels compile to it under
        // -ffast-math, and dz must keep their bits
        const float pr = l15 == tc[j] ? __builtin_fmaf(e[j], inv_se, -1.f) : e[j] * inv_se;
        dzs[lrow * HH_CPAD + l15] = (live && l15 < C) ? f32_to_bf16(pr * inv_B) : (bf16raw)0;
        if (live && l15 == 0) lsum += (__logf(se[j]) + mx[j] - xt) * inv_B;
        if (logits_out != nullptr && live && l15 < C)
          logits_out[(m0 + lrow) * C + l15] = xb[j];
      }
    }
    mt_lds_barrier();

    // ---- dgrad + mask: this wave's share of the tile's 16-row fragments ----
    // w3 as the A operand (M = h, K = class padded to 32), gathered from the
    // LDS copy each tile: held in registers through the GEMM it spills.  M-row
    // m of fragment e maps to h = p*32 + (m/4)*8 + e*4 + (m%4), which the
    // copy holds at step p, lane group m/4, value e*4 + (m%4) of class c.
    mt_frag_t wf[2];
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int i = 0; i < 8; ++i)
        wf[e][i] = q < 2 ? (short)w3s[(p * 64 + (l15 >> 2) * 16 + q * 8 + i) * 8 + e * 4 + (l15 & 3)]
                         : (short)0;
#pragma unroll
    for (int rfi = 0; rfi < HH_BM / 16 / WPG; ++rfi) {
      const int row = (rfi * WPG + sub) * 16 + l15;
      mt_frag_t bz = {};
      if (q < 2) bz = mt_ld_frag<HH_CPAD, 0>(dzs, row, q);
      const floatx4 z = {0.f, 0.f, 0.f, 0.f};
      const floatx4 d0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0], bz, z, 0, 0, 0);
      const floatx4 d1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1], bz, z, 0, 0, 0);
      const int slot = p * 4 + q;
      const shortx8 mk = mt_ld_frag<H, XM>(ys, row, slot);
      shortx8 out;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        out[j] = bf16_to_f32((bf16raw)mk[j]) > 0.f ? (short)f32_to_bf16(d0[j]) : (short)0;
        out[4 + j] = bf16_to_f32((bf16raw)mk[4 + j]) > 0.f ? (short)f32_to_bf16(d1[j]) : (short)0;
      }
      if (m0 + row < B) *(shortx8*)(dz_in + (m0 + row) * H + slot * 8) = out;
    }

    // ---- wgrad + bias grad: this wave's share of the tile's 32-row steps ----
    mt_frag_t ones;
#pragma unroll
    for (int i = 0; i < 8; ++i) ones[i] = (short)MT_BF16_ONE;
#pragma unroll
    for (int ksi = 0; ksi < HH_BM / 32 / WPG; ++ksi) {
      const int ks = ksi * WPG + sub;
      // fragment value i <-> tile row ks*32 + (i/4)*16 + q*4 + (i%4), the same
      // row order for both operands
      const mt_frag_t bz = mt_tr_frag<HH_CPAD, 4, 16, hh_key0>(dzs, ks * 32, q, l15, 0);
      if (p == 0) accb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, bz, accb, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const mt_frag_t ay = mt_tr_frag<H, 4, 16, hh_key15>(ys, ks * 32, q, l15, p * 32 + e * 16);
        accw[e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ay, bz, accw[e], 0, 0, 0);
      }
    }
    // every wave is done with both images before the next tile's slabs land
    mt_lds_barrier();
  }

  // one loss atomic per block
#pragma unroll
  for (int off = 32; off; off >>= 1) lsum += __shfl_xor(lsum, off, 64);
  if (lane == 0) lred[wid] = lsum;
  __syncthreads();
  if (wid == 0 && lane == 0) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < HH_WAVES; ++i) s += lred[i];
    if (s != 0.f) atomicAdd(loss, s);
  }

  // flush: accumulator lane (c = l15, q), element r <-> h = base + 4q + r
  if (l15 < C) {
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int r = 0; r < 4; ++r) atomicAdd(dw + l15 * H + p * 32 + e * 16 + q * 4 + r, accw[e][r]);
    if (db != nullptr && p == 0 && q == 0) atomicAdd(db + l15, accb[0]);
  }
}

// the loss scalar's zero, as a launch: a graph capture records it as a kernel
__global__ void hidden_head_zero_loss_kernel(float* loss) { *loss = 0.f; }

// 1 when a hidden layer K_in -> H under a head of C classes is served
extern "C" int hidden_head_ce_supported(int K_in, int H, int C) {
  return K_in >= HH_BK && K_in <= 256 && K_in % HH_BK == 0 && (H == 128 || H == 256) && C >= 1 &&
         C <= HH_CPAD;
}

// Rows from which functional._mlp_chain_step routes a supported stack here.
// tools/hidden_head_ce_bench.hip measured this kernel faster than the two
// launches at every B from 4096 up (profiles/hidden_head_ce.md, "Threshold"),
// but below linear_fwd_stream_min_rows() the library's linear_fwd is
// gemm_kernel, which the tool does not time: the threshold is the smallest
// measured B at which the timed pair is the pair the step would launch.
#define HH_MIN_ROWS 32768
extern "C" int64_t hidden_head_ce_min_rows() { return HH_MIN_ROWS; }

// loss is defined, not accumulated: a one-thread kernel zeroes it on the
// stream first.  max_blocks > 0 caps the grid (tests force several tiles per
// block with it).  x, w2, w3, dz_in and h2_out 16-byte aligned.
extern "C" hipError_t launch_hidden_head_ce(const bf16raw* x, const bf16raw* w2, const float* b2,
                                            const bf16raw* w3, const float* b3,
                                            const int64_t* tgt, bf16raw* dz_in, float* dw,
                                            float* db, float* loss, bf16raw* logits_out,
                                            bf16raw* h2_out, int B, int K_in, int H, int C,
                                            int max_blocks, int num_cus, hipStream_t stream) {
  if (!hidden_head_ce_supported(K_in, H, C) || B < 1 || B > (1LL << 31) - 1 - HH_BM)
    return hipErrorInvalidValue;
  if ((((uintptr_t)x) | ((uintptr_t)w2) | ((uintptr_t)w3) | ((uintptr_t)dz_in) |
       ((uintptr_t)h2_out)) & 15)
    return hipErrorInvalidValue;
  const int ntiles = (B + HH_BM - 1) / HH_BM;
  int grid = 2 * (num_cus > 0 ? num_cus : 256);
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  if (grid > ntiles) grid = ntiles;
  hidden_head_zero_loss_kernel<<<dim3(1), dim3(1), 0, stream>>>(loss);
#define HH_LAUNCH(HH)                                                                    \
  hidden_head_ce_kernel<HH><<<dim3(grid), dim3(HH_THREADS), 0, stream>>>(                \
      x, w2, b2, w3, b3, tgt, dz_in, dw, db, loss, logits_out, h2_out, B, K_in, C, 1.0f / B)
  if (H == 128)
    HH_LAUNCH(128);
  else
    HH_LAUNCH(256);
#undef HH_LAUNCH
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
