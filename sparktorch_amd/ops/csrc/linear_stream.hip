// Full-N streaming GEMM for the big-batch Linear forward and input gradient:
//
//   fwd    Y[M,N]  = X[M,K]  W[N,K]^T  (+bias)(+relu)
//   dgrad  dX[M,N] = dZ[M,K] W[K,N]    (zeroed where mask[M,N] <= 0, optional)
//
// A (x / h / dz) is bf16 row-major with M in the millions; W is a small bf16
// matrix.  gemm.hip's 128x128 tile covers N = 256 with two blocks that are
// scheduled far apart, so every A row comes from HBM twice.  Here
//
//   * one block of 8 waves (2 x 4, a 64x64 sub-tile each, as gemm.hip's <2,4>
//     tile) owns 128 rows times ALL N <= 256 output columns: A is read once
//     chip-wide and W is re-staged once per 128 rows instead of twice;
//   * both operands go global->LDS by DMA, one barrier per k-slab: W (from
//     L2) one slab ahead through two buffers, A (from HBM) two slabs ahead
//     through three, its newest slab left in flight across the barrier by a
//     counted vmcnt wait.  A and the forward's k-contiguous W land in
//     mfma_tile.h's k-major image (ds_read_b128 fragments);
//   * k-slabs are 32 deep: 56 KB of LDS, two blocks (16 waves) per CU.  64
//     deep (one block per CU) was 3 % faster at K = 784 and 9-25 % slower at
//     K = 256 (profiles/linear_stream.md); the launcher keeps it selectable
//     for tools/linear_stream_bench.hip;
//   * the dgrad's W is read along its outer stride.  Its slab is staged as it
//     lies in memory ([k][n], 16 B slots XOR-swizzled by k-row) and the B
//     fragments come from the transposing LDS read (ds_read_b64_tr_b16, lane
//     semantics in profiles/bench_resnet18_optimization_log.md), addressed so
//     that lane group kg gets k = 8kg .. 8kg+7 of the 32-wide MFMA step —
//     mfma_tile.h's k-packing, as every other fragment here;
//   * one fp32 accumulator per output, K ascending in 32-wide MFMA steps,
//     mfma_tile.h's epilogue (per-wave LDS transpose, 16 B stores): the bf16
//     results are bit-identical to gemm_kernel's.
//
// Rows past M and a K tail take a guarded, zero-filling stage of the same
// images.  N = 192 leaves wave column 3 idle (it still helps staging).

#include "launchers.h"
#include "mfma_tile.h"

#define LS_THREADS 512
#define LS_WAVES 8
#define LS_BM 128
#define LS_BN 256

// ---- dgrad W: image [BKT k-rows][256 n], 32 slots a row ----

// A transposing read's 32-lane half covers 8 k-rows (k = 8kg + 4jh + 0..3 for
// two kg) x 32 B; the key moves them onto the 8 distinct 32 B bank groups.
struct ls_tkey {
  static __device__ __forceinline__ int key(int row) {
    return ((row & 3) | (((row >> 3) & 1) << 2)) << 1;
  }
};

// Image slot -> source slot, clamped into the row for N < 256 (columns past
// N are then copies of valid ones and are never stored).
template <int BKT>
__device__ __forceinline__ void ls_dma_nmajor(const bf16raw* __restrict__ src,
                                              bf16raw* __restrict__ lds, int kt, int N, int wid,
                                              int lane) {
  constexpr int NCHUNK = BKT / 2;  // 1 KB = two 512 B image rows
  const int r_in = lane >> 5;
#pragma unroll
  for (int c0 = 0; c0 < NCHUNK; c0 += LS_WAVES) {
    const int c = c0 + wid;
    const int row = c * 2 + r_in;
    int sslot = (lane & 31) ^ ls_tkey::key(row);
    if (sslot > (N >> 3) - 1) sslot = (N >> 3) - 1;
    const bf16raw* g = src + (int64_t)(kt + row) * N + sslot * 8;
    mt_glds16(g, lds + c * 2 * LS_BN);
  }
}

template <int BKT>
__device__ __forceinline__ void ls_fill_nmajor(const bf16raw* __restrict__ src,
                                               bf16raw* __restrict__ lds, int kt, int kmax, int N,
                                               int t) {
#pragma unroll
  for (int u = t; u < BKT * 32; u += LS_THREADS) {
    const int row = u >> 5;
    int sslot = (u & 31) ^ ls_tkey::key(row);
    if (sslot > (N >> 3) - 1) sslot = (N >> 3) - 1;
    shortx8 v = {};
    if (kt + row < kmax) v = *(const shortx8*)(src + (int64_t)(kt + row) * N + sslot * 8);
    *(shortx8*)(lds + u * 8) = v;
  }
}

// BT: B is W[K][N] (dgrad); else W[N][K] (forward)
template <int EPI, int BKT, bool BT>
__global__ __launch_bounds__(LS_THREADS, BKT == 32 ? 4 : 2) void linear_stream_kernel(
    const bf16raw* __restrict__ A, const bf16raw* __restrict__ B, bf16raw* __restrict__ C,
    const float* __restrict__ bias, const bf16raw* __restrict__ mask, int M, int N, int K) {
  constexpr int SUBS = BKT / 32;  // MFMA k-steps per slab
  constexpr int A_EL = LS_BM * BKT, B_EL = LS_BN * BKT;
  constexpr int EP_EL = LS_WAVES * 16 * MT_EPAD * 2;  // epilogue scratch, in bf16 units
  constexpr int ST_EL = 3 * A_EL + 2 * B_EL;
  // DMA instructions a wave issues for one A slab (chunks are dealt evenly)
  constexpr int A_DMA = LS_BM * BKT * 2 / 1024 / LS_WAVES;
  static_assert(A_DMA == 1 || A_DMA == 2, "the counted wait below is written for these");
  // one array: a ring of three A slabs and two W slabs; the epilogue's
  // per-wave scratch reuses it
  __shared__ __attribute__((aligned(16))) bf16raw smem[ST_EL > EP_EL ? ST_EL : EP_EL];
  bf16raw* const a0 = smem;
  bf16raw* const a1 = smem + A_EL;
  bf16raw* const a2 = smem + 2 * A_EL;
  bf16raw* const b0 = smem + 3 * A_EL;
  bf16raw* const b1 = smem + 3 * A_EL + B_EL;

  const int t = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int wr = wid >> 2, wc = wid & 3;
  const int l15 = lane & 15, kg = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * LS_BM;
  const bool rows_full = m0 + LS_BM <= M;
  const bool active = wc * 64 < N;  // N = 192: wave column 3 has no outputs

  // true when the slab went by DMA (A_DMA instructions per wave, in flight)
  auto stage_a = [&](bf16raw* an, int kt) -> bool {
    if (rows_full && kt + BKT <= K) {
      mt_dma_kmajor<LS_WAVES, LS_BM, BKT, false>(A, an, m0, LS_BM, K, kt, wid, lane);
      return true;
    }
    mt_fill_kmajor<LS_THREADS, LS_BM, BKT>(A, an, m0, M, K, kt, K, t);
    return false;
  };
  auto stage_b = [&](bf16raw* bn, int kt) {
    if (kt + BKT <= K) {
      if (BT)
        ls_dma_nmajor<BKT>(B, bn, kt, N, wid, lane);
      else
        mt_dma_kmajor<LS_WAVES, LS_BN, BKT, false>(B, bn, 0, N, K, kt, wid, lane);
    } else {
      if (BT)
        ls_fill_nmajor<BKT>(B, bn, kt, K, N, t);
      else
        mt_fill_kmajor<LS_THREADS, LS_BN, BKT>(B, bn, 0, N, K, kt, K, t);
    }
  };
  // End of a step: every wave's loads for the next slab have landed and its
  // fragment reads of this one are done.  An A slab staged two ahead by DMA
  // is each wave's LAST A_DMA memory instructions and stays in flight across
  // the barrier (vmcnt retires in order).  __syncthreads() would drain it.
  auto publish = [&](bool a_in_flight) {
    if (a_in_flight)
      mt_wait_barrier<A_DMA>();
    else
      mt_wait_barrier<0>();
  };

  floatx4 acc[4][4] = {};

  auto mma = [&](const bf16raw* ab, const bf16raw* bb, int kt) {
    if (!active) return;
#pragma unroll
    for (int sub = 0; sub < SUBS; ++sub) {
      if (sub > 0 && kt + sub * 32 >= K) break;  // an all-zero step of the K tail
      mt_frag_t a[4], b[4];
      const int kq = kg + sub * 4;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
        a[mi] = mt_ld_frag<BKT, BKT / 8 - 1>(ab, wr * 64 + mi * 16 + l15, kq);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        if (BT)
          b[ni] = mt_tr_frag<LS_BN, 8, 4, ls_tkey>(bb, sub * 32, kg, l15, wc * 64 + ni * 16);
        else
          b[ni] = mt_ld_frag<BKT, BKT / 8 - 1>(bb, wc * 64 + ni * 16 + l15, kq);
      }
      mt_mma_tile(acc, a, b);
    }
  };

  // The A stream comes from HBM and one slab in flight per block leaves the
  // k-loop latency-bound (profiles/linear_stream.md), so A runs two slabs
  // ahead through a ring of three; W comes from L2, one slab ahead, ring of
  // two.  Step on slab kt (in ab / bb): issue W(kt+1) into bn, THEN A(kt+2)
  // into an2 (the order publish() relies on), multiply, publish.  Both
  // targets were last read in the step before, which its barrier closed.
  auto step = [&](const bf16raw* ab, const bf16raw* bb, bf16raw* bn, bf16raw* an2, int kt) {
    if (kt + BKT < K) stage_b(bn, kt + BKT);
    bool a_in_flight = false;
    if (kt + 2 * BKT < K) a_in_flight = stage_a(an2, kt + 2 * BKT);
    mma(ab, bb, kt);
    publish(a_in_flight);
  };

  stage_a(a0, 0);
  stage_b(b0, 0);
  publish(BKT < K ? stage_a(a1, BKT) : false);
  // the rings return to (a0, b0) every six slabs; buffers are compile-time
  // constants in each step so the compiler can tell the DMA targets from the
  // images the fragment reads use
  for (int kt = 0;; kt += 6 * BKT) {
    step(a0, b0, b1, a2, kt);
    if (kt + 1 * BKT >= K) break;
    step(a1, b1, b0, a0, kt + 1 * BKT);
    if (kt + 2 * BKT >= K) break;
    step(a2, b0, b1, a1, kt + 2 * BKT);
    if (kt + 3 * BKT >= K) break;
    step(a0, b1, b0, a2, kt + 3 * BKT);
    if (kt + 4 * BKT >= K) break;
    step(a1, b0, b1, a0, kt + 4 * BKT);
    if (kt + 5 * BKT >= K) break;
    step(a2, b1, b0, a1, kt + 5 * BKT);
    if (kt + 6 * BKT >= K) break;
  }

  // Epilogue: mt_epi_slice's arithmetic and scratch layout, written out.
  // Through the helper the 64-deep-slab kernels measured 2 % slower
  // (profiles/tile_refactor.md), so this kernel keeps its own copy.  The
  // staging images are idle (trailing barrier above).
  if (!active) return;
  const int64_t m_base = m0 + wr * 64;
  const int n_base = wc * 64;
  float* ep = (float*)smem + wid * 16 * MT_EPAD;
  const int orow = lane >> 2;  // output row of the slice
  const int oct = lane & 3;    // which 16 columns of the wave's 64
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int64_t m = m_base + mi * 16 + orow;
    // fetched before the transpose so the global load overlaps it
    shortx8 mk[2] = {};
    if (EPI == EPI_BF16_MASK && m < M) {
      const bf16raw* mp = mask + m * N + n_base + oct * 16;
      mk[0] = *(const shortx8*)mp;
      mk[1] = *(const shortx8*)(mp + 8);
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) ep[(kg * 4 + r) * MT_EPAD + ni * 16 + l15] = acc[mi][ni][r];
    __builtin_amdgcn_s_waitcnt(0);  // own-wave LDS writes visible
    if (m < M) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c0 = oct * 16 + h * 8;
        const int n = n_base + c0;
        alignas(16) short outp[8];
        const float* src = ep + orow * MT_EPAD + c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float val = src[j];
          if (EPI == EPI_BIAS || EPI == EPI_BIAS_RELU) val += bias[n + j];
          if (EPI == EPI_BIAS_RELU || EPI == EPI_RELU) val = fmaxf(val, 0.f);
          outp[j] = (short)f32_to_bf16(val);
          if (EPI == EPI_BF16_MASK && !(bf16_to_f32((bf16raw)mk[h][j]) > 0.f)) outp[j] = 0;
        }
        *(shortx8*)(C + m * N + n) = *(const shortx8*)outp;
      }
    }
    __builtin_amdgcn_s_waitcnt(0);  // all lanes done reading before reuse
  }
}

// ---- deep-K forward: K > 256, where W does not fit a CU ----
//
// At K = 784 the kernel above re-stages all of W once per 128 rows and each
// wave runs DMA issue, fragment reads, wait, MFMAs, barrier one after the
// other (profiles/linear_stream_deep.md).  This one is the same arithmetic on
//
//   * 256 rows x all N <= 256 columns per block: 16 waves (4 x 4, the same
//     64x64 sub-tile each), one block per CU.  W is staged once per 256 rows;
//   * 32-deep slabs, A through a ring of five and W through a ring of three
//     (128 KB of LDS).  Step s multiplies slab s from registers, reads the
//     fragments of slab s+1 under those MFMAs (each into the registers its
//     last MFMA of the step has just freed: one fragment set, 128 VGPRs),
//     issues W(s+3) then A(s+5) into the slots slab s left in step s-1, and
//     ends on a counted wait for slab s+2 and the step's one barrier: three
//     slabs of A stay in flight across it;
//   * KEY is the image's slot key (mfma_tile.h).  A key that also separates
//     rows r and r+4 measured the same (profiles/linear_stream_deep.md) and
//     was dropped.
//
// Ring slots are compile-time constants in every step (15 steps unrolled, the
// rings' common period), so the compiler can tell the DMA targets from the
// images the fragment reads use and puts no full wait in front of the MFMAs.
// Epilogue, edges and bits are those of the kernel above.

#define LD_THREADS 1024
#define LD_WAVES 16
#define LD_BM 256
#define LD_BK 32
#define LD_NA 5
#define LD_NW 3

template <int EPI, typename KEY>
__global__ __launch_bounds__(LD_THREADS, 4) void linear_stream_deep_kernel(
    const bf16raw* __restrict__ A, const bf16raw* __restrict__ B, bf16raw* __restrict__ C,
    const float* __restrict__ bias, int M, int N, int K) {
  constexpr int BKT = LD_BK;
  constexpr int A_EL = LD_BM * BKT, B_EL = LS_BN * BKT;
  constexpr int EP_EL = LD_WAVES * 16 * MT_EPAD * 2;  // epilogue scratch, in bf16 units
  constexpr int ST_EL = LD_NA * A_EL + LD_NW * B_EL;
  static_assert(LD_BM * BKT * 2 / 1024 == LD_WAVES && LS_BN * BKT * 2 / 1024 == LD_WAVES,
                "one DMA instruction per wave and slab: publish() counts them");
  static_assert(ST_EL >= EP_EL, "the epilogue's scratch reuses the rings");
  __shared__ __attribute__((aligned(16))) bf16raw smem[ST_EL];
#define LD_B(i) (smem + ((i) % LD_NW) * B_EL)
#define LD_A(i) (smem + LD_NW * B_EL + ((i) % LD_NA) * A_EL)

  const int t = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int wr = wid >> 2, wc = wid & 3;
  const int l15 = lane & 15, kg = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * LD_BM;
  const bool rows_full = m0 + LD_BM <= M;
  const bool active = wc * 64 < N;  // N = 192: wave column 3 has no outputs

  // Both images are 256 rows x 4 slots and a wave's 1 KB DMA chunk is 16 rows,
  // so thread t stages the 16 B at image offset t * 16 whether by DMA or by
  // the guarded copy: image row t / 4, whose source k-slot the key picks.
  // One 32-bit byte offset per operand, added to a wave-uniform slab address,
  // keeps the address registers few (K <= 65536 bounds it).  W's image rows
  // at or past N get copies of valid rows by DMA, so every wave issues one.
  const int srow = t >> 2;
  const int sk = ((lane & 3) ^ KEY::template key<4>(srow)) << 3;
  const uint32_t a_off = (uint32_t)(srow * K + sk) * 2;
  const uint32_t b_off = (uint32_t)((srow < N ? srow : (srow & 63)) * K + sk) * 2;
  const char* const a_tile = (const char*)(A + m0 * K);

  // 1 when the slab went by DMA (one instruction per wave, in flight), else 0
  auto stage_a = [&](bf16raw* an, int kt) -> int {
    const char* src = a_tile + kt * 2;
    if (rows_full && kt + BKT <= K) {
      mt_glds16((const bf16raw*)(src + a_off), an + wid * 512);
      return 1;
    }
    shortx8 v = {};
    if (m0 + srow < M && kt + sk < K) v = *(const shortx8*)(src + a_off);
    *(shortx8*)(an + t * 8) = v;
    return 0;
  };
  auto stage_b = [&](bf16raw* bn, int kt) -> int {
    const char* src = (const char*)(B + kt);
    if (kt + BKT <= K) {
      mt_glds16((const bf16raw*)(src + b_off), bn + wid * 512);
      return 1;
    }
    shortx8 v = {};
    if (srow < N && kt + sk < K) v = *(const shortx8*)(src + b_off);
    *(shortx8*)(bn + t * 8) = v;
    return 0;
  };
  // the wave's memory instructions other than its newest `newer` are complete
  auto publish = [&](int newer) {
    switch (newer) {
      case 4: mt_wait_barrier<4>(); break;
      case 3: mt_wait_barrier<3>(); break;
      case 2: mt_wait_barrier<2>(); break;
      case 1: mt_wait_barrier<1>(); break;
      default: mt_wait_barrier<0>(); break;
    }
  };

  floatx4 acc[4][4] = {};
  mt_frag_t a[4], b[4];
  auto ld_a = [&](const bf16raw* ab, int mi) {
    return mt_ld_frag32<KEY>(ab, wr * 64 + mi * 16 + l15, kg);
  };
  auto ld_b = [&](const bf16raw* bb, int ni) {
    return mt_ld_frag32<KEY>(bb, wc * 64 + ni * 16 + l15, kg);
  };

  // K > 256: slabs 0 .. 4 of A and 0 .. 2 of W exist and only A can need the
  // guarded stage (rows past M).  Issue order: everything slabs 0 and 1 need,
  // then A2 A3 W2 A4; the wait leaves those four in flight.
  int a_last = 0;  // A(s+4) of the step before went by DMA
  {
    int newer = 0;
    stage_a(LD_A(0), 0);
    stage_b(LD_B(0), 0);
    stage_a(LD_A(1), BKT);
    stage_b(LD_B(1), BKT);
    newer += stage_a(LD_A(2), 2 * BKT);
    newer += stage_a(LD_A(3), 3 * BKT);
    newer += stage_b(LD_B(2), 2 * BKT);
    newer += a_last = stage_a(LD_A(4), 4 * BKT);
    publish(newer);
  }
  if (active) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = ld_a(LD_A(0), i);
      b[i] = ld_b(LD_B(0), i);
    }
  }
  // slot 0 of both rings is the first DMA target below
  mt_lds_barrier();

  // Step on slab kt (in a / b); `an`, `bn` hold slab kt + BKT, published by
  // the step before; `ai`, `bi` held slab kt, last read in the step before.
  // At its end slab kt + 2 BKT must have landed: W of it was issued in the
  // step before, ahead of that step's A, so what may stay in flight is that A
  // and this step's two issues.
  auto step = [&](const bf16raw* an, const bf16raw* bn, bf16raw* ai, bf16raw* bi, int kt) {
    int newer = a_last;
    if (kt + LD_NW * BKT < K) newer += stage_b(bi, kt + LD_NW * BKT);
    a_last = 0;
    if (kt + LD_NA * BKT < K) newer += a_last = stage_a(ai, kt + LD_NA * BKT);
    if (active) {
      // Each fragment of slab kt + BKT goes into the registers its last MFMA
      // of this step has just freed: a[mi] after row mi, b[ni] inside the
      // last row.  Past the last slab these read a stale image, unused.
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
          if (mi == 3) b[ni] = ld_b(bn, ni);
        }
        a[mi] = ld_a(an, mi);
      }
    }
    publish(newer);
  };

  for (int kt = 0;; kt += 15 * BKT) {
#define LD_STEP(j)                                                                \
  step(LD_A(j + 1), LD_B(j + 1), LD_A(j), LD_B(j), kt + (j) * BKT);               \
  if (kt + ((j) + 1) * BKT >= K) break;
    LD_STEP(0) LD_STEP(1) LD_STEP(2) LD_STEP(3) LD_STEP(4)
    LD_STEP(5) LD_STEP(6) LD_STEP(7) LD_STEP(8) LD_STEP(9)
    LD_STEP(10) LD_STEP(11) LD_STEP(12) LD_STEP(13) LD_STEP(14)
#undef LD_STEP
  }
#undef LD_A
#undef LD_B

  // Epilogue, as above: the last step waited for everything and its barrier
  // left the rings idle.
  if (!active) return;
  const int64_t m_base = m0 + wr * 64;
  const int n_base = wc * 64;
  float* ep = (float*)smem + wid * MT_EP_FLOATS;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int64_t m = m_base + mi * 16 + (lane >> 2);
    mt_epi_slice<EPI>(ep, acc[mi], lane, l15, kg, m < M, m, N, n_base, C, bias, nullptr);
  }
}

// 1 when the deep-K forward serves this shape
extern "C" int linear_fwd_stream_deep_supported(int N, int K, int64_t M) {
  return N > 128 && N <= LS_BN && N % 64 == 0 && K > 256 && K <= 65536 && K % 8 == 0 && M >= 1 &&
         M < (1LL << 31) - LD_BM;
}

// 1 when the kernel can compute C[M,N] = A[M,K] B for this shape
extern "C" int linear_fwd_stream_supported(int N, int K, int64_t M) {
  return N > 128 && N <= LS_BN && N % 64 == 0 && K >= 8 && K % 8 == 0 && M >= 1 &&
         M < (1LL << 31) - LS_BM;
}

// Rows from which the linear_fwd / linear_dgrad / linear_dgrad_relu bindings
// route a supported shape here: the smallest M at which
// tools/linear_stream_bench.hip measured this kernel not slower than
// gemm_kernel's 128x128 tile at any of the three flagship shapes
// (profiles/linear_stream.md, "Threshold": at 16384 rows the 256 -> 256
// forward is still 11.4 us against 9.1).
#define LS_MIN_ROWS 32768
extern "C" int64_t linear_fwd_stream_min_rows() { return LS_MIN_ROWS; }

// Rows from which the automatic choice gives a K > 256 forward to the deep
// kernel: the smallest M at which tools/linear_stream_bench.hip measured it
// not slower than the kernel above at 784 -> 256
// (profiles/linear_stream_deep.md, "Threshold").  Its grid is one 256-row
// block per CU, which loses while the blocks do not fill the chip.
#define LS_DEEP_MIN_ROWS 65536
extern "C" int64_t linear_fwd_stream_deep_min_rows() { return LS_DEEP_MIN_ROWS; }

// epi: EPI_BF16 / BIAS / BIAS_RELU / RELU (mfma_tile.h) for the forward
// (b_kn = 0, B = W[N][K]); EPI_BF16 / EPI_BF16_MASK for the dgrad (b_kn = 1,
// B = W[K][N]).  bk: k-slab depth of linear_stream_kernel, 32 or 64, 0 = the
// measured default.  fwd_path: which forward kernel, LS_PATH_*; the dgrad has
// one.  All pointers 16-byte aligned.
extern "C" hipError_t launch_linear_stream(const bf16raw* A, const bf16raw* B, bf16raw* C,
                                           const float* bias, const bf16raw* mask, int64_t M,
                                           int N, int K, int epi, int b_kn, int bk, int fwd_path,
                                           hipStream_t stream) {
  if (!linear_fwd_stream_supported(N, K, M)) return hipErrorInvalidValue;
  if ((((uintptr_t)A) | ((uintptr_t)B) | ((uintptr_t)C) | ((uintptr_t)mask)) & 15)
    return hipErrorInvalidValue;
  if ((epi == EPI_BIAS || epi == EPI_BIAS_RELU) && bias == nullptr)
    return hipErrorInvalidValue;
  if (epi == EPI_BF16_MASK && mask == nullptr) return hipErrorInvalidValue;
  if (bk == 0) bk = 32;
  if (bk != 32 && bk != 64) return hipErrorInvalidValue;
  if (fwd_path < LS_PATH_AUTO || fwd_path > LS_PATH_DEEP) return hipErrorInvalidValue;
  if (fwd_path == LS_PATH_AUTO)
    fwd_path = !b_kn && M >= LS_DEEP_MIN_ROWS && linear_fwd_stream_deep_supported(N, K, M)
                   ? LS_PATH_DEEP
                   : LS_PATH_TILE128;
  if (fwd_path == LS_PATH_DEEP) {
    if (b_kn || !linear_fwd_stream_deep_supported(N, K, M)) return hipErrorInvalidValue;
    const dim3 dgrid((unsigned)ceil_div_i64(M, LD_BM)), dblock(LD_THREADS);
#define LS_LAUNCH_DEEP(EPIC)                                                     \
  linear_stream_deep_kernel<EPIC, mt_key_row><<<dgrid, dblock, 0, stream>>>(     \
      A, B, C, bias, (int)M, N, K)
    if (epi == EPI_BF16) LS_LAUNCH_DEEP(EPI_BF16);
    else if (epi == EPI_BIAS) LS_LAUNCH_DEEP(EPI_BIAS);
    else if (epi == EPI_BIAS_RELU) LS_LAUNCH_DEEP(EPI_BIAS_RELU);
    else if (epi == EPI_RELU) LS_LAUNCH_DEEP(EPI_RELU);
    else return hipErrorInvalidValue;
#undef LS_LAUNCH_DEEP
    HIP_CHECK_LAUNCH();
    return hipSuccess;
  }
  const dim3 grid((unsigned)ceil_div_i64(M, LS_BM)), block(LS_THREADS);
#define LS_LAUNCH(EPIC, BT)                                                                   \
  do {                                                                                        \
    if (bk == 32)                                                                             \
      linear_stream_kernel<EPIC, 32, BT><<<grid, block, 0, stream>>>(A, B, C, bias, mask,     \
                                                                     (int)M, N, K);           \
    else                                                                                      \
      linear_stream_kernel<EPIC, 64, BT><<<grid, block, 0, stream>>>(A, B, C, bias, mask,     \
                                                                     (int)M, N, K);           \
  } while (0)
  if (b_kn) {
    if (epi == EPI_BF16) LS_LAUNCH(EPI_BF16, true);
    else if (epi == EPI_BF16_MASK) LS_LAUNCH(EPI_BF16_MASK, true);
    else return hipErrorInvalidValue;
  } else {
    if (epi == EPI_BF16) LS_LAUNCH(EPI_BF16, false);
    else if (epi == EPI_BIAS) LS_LAUNCH(EPI_BIAS, false);
    else if (epi == EPI_BIAS_RELU) LS_LAUNCH(EPI_BIAS_RELU, false);
    else if (epi == EPI_RELU) LS_LAUNCH(EPI_RELU, false);
    else return hipErrorInvalidValue;
  }
#undef LS_LAUNCH
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
