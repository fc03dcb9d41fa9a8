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
//     gemm.hip's pad-free image (16 B k-slots XOR-swizzled by row,
//     ds_read_b128 fragments);
//   * k-slabs are 32 deep: 56 KB of LDS, two blocks (16 waves) per CU.  64
//     deep (one block per CU) was 3 % faster at K = 784 and 9-25 % slower at
//     K = 256 (profiles/linear_stream.md); the launcher keeps it selectable
//     for tools/linear_stream_bench.hip;
//   * the dgrad's W is read along its outer stride.  Its slab is staged as it
//     lies in memory ([k][n], 16 B slots XOR-swizzled by k-row) and the B
//     fragments come from the transposing LDS read (ds_read_b64_tr_b16, lane
//     semantics in profiles/bench_resnet18_optimization_log.md), addressed so
//     that lane group kg gets k = 8kg .. 8kg+7 of the 32-wide MFMA step —
//     the packing of every other fragment here and in gemm.hip;
//   * one fp32 accumulator per output, K ascending in 32-wide MFMA steps,
//     gemm.hip's epilogue (per-wave LDS transpose, 16 B stores): the bf16
//     results are bit-identical to gemm_kernel's.
//
// Rows past M and a K tail take a guarded, zero-filling stage of the same
// images.  N = 192 leaves wave column 3 idle (it still helps staging).

#include "common.h"

typedef shortx8 ls_frag_t;  // 8 bf16 (4 VGPRs)

#define LS_THREADS 512
#define LS_WAVES 8
#define LS_BM 128
#define LS_BN 256

// epilogue codes: gemm.hip's EPI_* values
#define LS_EPI_BF16 1
#define LS_EPI_BIAS 2
#define LS_EPI_BIAS_RELU 3
#define LS_EPI_RELU 4
#define LS_EPI_MASK 6

// ---- k-contiguous operand: image [ROWS][BKT], slot ^= row & (SLOTS - 1) ----

// rows row0 .. row0 + nrows - 1 must exist; nrows is a multiple of 16
template <int ROWS, int BKT>
__device__ __forceinline__ void ls_dma_kmajor(const bf16raw* __restrict__ src,
                                              bf16raw* __restrict__ lds, int64_t row0, int nrows,
                                              int ld, int kt, int wid, int lane) {
  constexpr int SLOTS = BKT / 8;       // 16 B slots per image row
  constexpr int CH_ROWS = 64 / SLOTS;  // rows per 1 KB wave chunk
  constexpr int NCHUNK = ROWS / CH_ROWS;
  const int r_in = lane / SLOTS;
  const int slot = lane % SLOTS;
#pragma unroll
  for (int c0 = 0; c0 < NCHUNK; c0 += LS_WAVES) {
    const int c = c0 + wid;
    if (c * CH_ROWS < nrows) {
      const int row = c * CH_ROWS + r_in;
      const int sslot = slot ^ (row & (SLOTS - 1));
      const bf16raw* g = src + (row0 + row) * ld + kt + sslot * 8;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)g,
          (__attribute__((address_space(3))) unsigned int*)(lds + c * CH_ROWS * BKT), 16, 0, 0);
    }
  }
}

// the same image with zero fill: rows at or past rmax, k at or past kmax
// (K is a multiple of 8, so a slot is wholly inside or wholly outside)
template <int ROWS, int BKT>
__device__ __forceinline__ void ls_fill_kmajor(const bf16raw* __restrict__ src,
                                               bf16raw* __restrict__ lds, int64_t row0,
                                               int64_t rmax, int ld, int kt, int kmax, int t) {
  constexpr int SLOTS = BKT / 8;
#pragma unroll
  for (int u = t; u < ROWS * SLOTS; u += LS_THREADS) {
    const int row = u / SLOTS;
    const int k = kt + (((u % SLOTS) ^ (row & (SLOTS - 1))) << 3);
    shortx8 v = {};
    if (row0 + row < rmax && k < kmax) v = *(const shortx8*)(src + (row0 + row) * ld + k);
    *(shortx8*)(lds + u * 8) = v;
  }
}

// ---- dgrad W: image [BKT k-rows][256 n], 32 slots a row ----

// A transposing read's 32-lane half covers 8 k-rows (k = 8kg + 4jh + 0..3 for
// two kg) x 32 B; the key moves them onto the 8 distinct 32 B bank groups.
__device__ __forceinline__ int ls_tkey(int row) {
  return ((row & 3) | (((row >> 3) & 1) << 2)) << 1;
}

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
    int sslot = (lane & 31) ^ ls_tkey(row);
    if (sslot > (N >> 3) - 1) sslot = (N >> 3) - 1;
    const bf16raw* g = src + (int64_t)(kt + row) * N + sslot * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)g,
        (__attribute__((address_space(3))) unsigned int*)(lds + c * 2 * LS_BN), 16, 0, 0);
  }
}

template <int BKT>
__device__ __forceinline__ void ls_fill_nmajor(const bf16raw* __restrict__ src,
                                               bf16raw* __restrict__ lds, int kt, int kmax, int N,
                                               int t) {
#pragma unroll
  for (int u = t; u < BKT * 32; u += LS_THREADS) {
    const int row = u >> 5;
    int sslot = (u & 31) ^ ls_tkey(row);
    if (sslot > (N >> 3) - 1) sslot = (N >> 3) - 1;
    shortx8 v = {};
    if (kt + row < kmax) v = *(const shortx8*)(src + (int64_t)(kt + row) * N + sslot * 8);
    *(shortx8*)(lds + u * 8) = v;
  }
}

// B fragment of MFMA step `krow0 / 32` for output columns col0 .. col0 + 15:
// value jh*4 + j of lane (kg, l15) is image row krow0 + 8kg + 4jh + j, column
// col0 + l15.
__device__ __forceinline__ ls_frag_t ls_tr_frag(const bf16raw* __restrict__ img, int krow0, int kg,
                                                int l15, int col0) {
  ls_frag_t f;
  const int col = col0 + 4 * (l15 & 3);
#pragma unroll
  for (int jh = 0; jh < 2; ++jh) {
    const int row = krow0 + kg * 8 + jh * 4 + (l15 >> 2);
    const bf16raw* p = img + row * LS_BN + ((((col >> 3) ^ ls_tkey(row)) << 3) | (col & 7));
    shortx4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) shortx4*)p);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[jh * 4 + j] = v[j];
  }
  return f;
}

// BT: B is W[K][N] (dgrad); else W[N][K] (forward)
template <int EPI, int BKT, bool BT>
__global__ __launch_bounds__(LS_THREADS, BKT == 32 ? 4 : 2) void linear_stream_kernel(
    const bf16raw* __restrict__ A, const bf16raw* __restrict__ B, bf16raw* __restrict__ C,
    const float* __restrict__ bias, const bf16raw* __restrict__ mask, int M, int N, int K) {
  constexpr int SUBS = BKT / 32;  // MFMA k-steps per slab
  constexpr int SLOTS = BKT / 8;
  constexpr int A_EL = LS_BM * BKT, B_EL = LS_BN * BKT;
  constexpr int EPAD = 68;
  constexpr int EP_EL = LS_WAVES * 16 * EPAD * 2;  // epilogue scratch, in bf16 units
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
      ls_dma_kmajor<LS_BM, BKT>(A, an, m0, LS_BM, K, kt, wid, lane);
      return true;
    }
    ls_fill_kmajor<LS_BM, BKT>(A, an, m0, M, K, kt, K, t);
    return false;
  };
  auto stage_b = [&](bf16raw* bn, int kt) {
    if (kt + BKT <= K) {
      if (BT)
        ls_dma_nmajor<BKT>(B, bn, kt, N, wid, lane);
      else
        ls_dma_kmajor<LS_BN, BKT>(B, bn, 0, N, K, kt, wid, lane);
    } else {
      if (BT)
        ls_fill_nmajor<BKT>(B, bn, kt, K, N, t);
      else
        ls_fill_kmajor<LS_BN, BKT>(B, bn, 0, N, K, kt, K, t);
    }
  };
  // End of a step: every wave's loads for the next slab have landed and its
  // fragment reads of this one are done.  An A slab staged two ahead by DMA
  // is each wave's LAST A_DMA memory instructions and stays in flight across
  // the barrier (vmcnt retires in order).  __syncthreads() would drain it.
  auto publish = [&](bool a_in_flight) {
    if (a_in_flight) {
      if (A_DMA == 1)
        asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
  };

  floatx4 acc[4][4] = {};

  auto mma = [&](const bf16raw* ab, const bf16raw* bb, int kt) {
    if (!active) return;
#pragma unroll
    for (int sub = 0; sub < SUBS; ++sub) {
      if (sub > 0 && kt + sub * 32 >= K) break;  // an all-zero step of the K tail
      ls_frag_t a[4], b[4];
      const int kq = kg + sub * 4;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int row = wr * 64 + mi * 16 + l15;
        a[mi] = *(const ls_frag_t*)&ab[row * BKT + ((kq ^ (row & (SLOTS - 1))) << 3)];
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        if (BT) {
          b[ni] = ls_tr_frag(bb, sub * 32, kg, l15, wc * 64 + ni * 16);
        } else {
          const int rowb = wc * 64 + ni * 16 + l15;
          b[ni] = *(const ls_frag_t*)&bb[rowb * BKT + ((kq ^ (rowb & (SLOTS - 1))) << 3)];
        }
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
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

  // Epilogue, as gemm_kernel's: each 16-row slice of the wave's sub-tile goes
  // through a per-wave [16][68] fp32 scratch so that every lane stores 16
  // contiguous bytes.  The staging images are idle (trailing barrier above).
  if (!active) return;
  const int64_t m_base = m0 + wr * 64;
  const int n_base = wc * 64;
  float* ep = (float*)smem + wid * 16 * EPAD;
  const int orow = lane >> 2;  // output row of the slice
  const int oct = lane & 3;    // which 16 columns of the wave's 64
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int64_t m = m_base + mi * 16 + orow;
    // fetched before the transpose so the global load overlaps it
    shortx8 mk[2] = {};
    if (EPI == LS_EPI_MASK && m < M) {
      const bf16raw* mp = mask + m * N + n_base + oct * 16;
      mk[0] = *(const shortx8*)mp;
      mk[1] = *(const shortx8*)(mp + 8);
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) ep[(kg * 4 + r) * EPAD + ni * 16 + l15] = acc[mi][ni][r];
    __builtin_amdgcn_s_waitcnt(0);  // own-wave LDS writes visible
    if (m < M) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c0 = oct * 16 + h * 8;
        const int n = n_base + c0;
        alignas(16) short outp[8];
        const float* src = ep + orow * EPAD + c0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float val = src[j];
          if (EPI == LS_EPI_BIAS || EPI == LS_EPI_BIAS_RELU) val += bias[n + j];
          if (EPI == LS_EPI_BIAS_RELU || EPI == LS_EPI_RELU) val = fmaxf(val, 0.f);
          outp[j] = (short)f32_to_bf16(val);
          if (EPI == LS_EPI_MASK && !(bf16_to_f32((bf16raw)mk[h][j]) > 0.f)) outp[j] = 0;
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

// epi: gemm.hip's EPI_BF16 / BIAS / BIAS_RELU / RELU for the forward
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
  if ((epi == LS_EPI_BIAS || epi == LS_EPI_BIAS_RELU) && bias == nullptr)
    return hipErrorInvalidValue;
  if (epi == LS_EPI_MASK && mask == nullptr) return hipErrorInvalidValue;
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
    if (epi == LS_EPI_BF16) LS_LAUNCH(LS_EPI_BF16, true);
    else if (epi == LS_EPI_MASK) LS_LAUNCH(LS_EPI_MASK, true);
    else return hipErrorInvalidValue;
  } else {
    if (epi == LS_EPI_BF16) LS_LAUNCH(LS_EPI_BF16, false);
    else if (epi == LS_EPI_BIAS) LS_LAUNCH(LS_EPI_BIAS, false);
    else if (epi == LS_EPI_BIAS_RELU) LS_LAUNCH(LS_EPI_BIAS_RELU, false);
    else if (epi == LS_EPI_RELU) LS_LAUNCH(LS_EPI_RELU, false);
    else return hipErrorInvalidValue;
  }
#undef LS_LAUNCH
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
