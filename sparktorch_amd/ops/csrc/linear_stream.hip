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

// epi: EPI_BF16 / BIAS / BIAS_RELU / RELU (mfma_tile.h) for the forward
// (b_kn = 0, B = W[N][K]); EPI_BF16 / EPI_BF16_MASK for the dgrad (b_kn = 1,
// B = W[K][N]).  bk: k-slab depth 32 or 64, 0 = the measured default.  All
// pointers 16-byte aligned.
extern "C" hipError_t launch_linear_stream(const bf16raw* A, const bf16raw* B, bf16raw* C,
                                           const float* bias, const bf16raw* mask, int64_t M,
                                           int N, int K, int epi, int b_kn, int bk,
                                           hipStream_t stream) {
  if (!linear_fwd_stream_supported(N, K, M)) return hipErrorInvalidValue;
  if ((((uintptr_t)A) | ((uintptr_t)B) | ((uintptr_t)C) | ((uintptr_t)mask)) & 15)
    return hipErrorInvalidValue;
  if ((epi == EPI_BIAS || epi == EPI_BIAS_RELU) && bias == nullptr)
    return hipErrorInvalidValue;
  if (epi == EPI_BF16_MASK && mask == nullptr) return hipErrorInvalidValue;
  if (bk == 0) bk = 32;
  if (bk != 32 && bk != 64) return hipErrorInvalidValue;
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
