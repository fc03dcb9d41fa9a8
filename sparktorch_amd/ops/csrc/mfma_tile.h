// Tile-level primitives shared by the MFMA GEMM-family kernels (gemm.hip,
// conv_implicit.hip, linear_stream.hip, mlp_predict.hip, head_bwd.hip,
// linear_wgrad.hip).  Each rule that makes those kernels bit-identical to one
// another is written here once:
//
//   * the k-major LDS image: pad-free [ROWS][BKT] bf16, the 16 B k-slot of
//     each row XOR-swizzled by (row & (BKT / 8 - 1)) — lane-linear for the
//     global->LDS DMA (destination = wave-uniform base + lane * 16),
//     bank-spread for the ds_read_b128 fragment reads.  The swizzle permutes
//     16 B pieces inside one 128 B line of the source row, so global
//     coalescing is kept;
//   * the k-packing of a fragment: lane (l15, kg) of a 16x16x32 MFMA operand
//     holds row l15, k = 8kg .. 8kg+7 of the 32-wide step, whether it comes
//     from a ds_read_b128 of a k-major image or from the transposing read of
//     an image stored as it lies in memory;
//   * the counted vmcnt wait that leaves a wave's newest DMAs in flight
//     across a barrier;
//   * the bf16 epilogue's rounding order (+bias, relu, round, mask).
//
// Everything is a __device__ __forceinline__ template on compile-time sizes;
// nothing here decides anything at run time.  Names carry the mt_ / MT_
// prefix (EPI_* for the epilogue codes): the tools include several .hip
// files into one translation unit.
#pragma once

#include "common.h"

typedef shortx8 mt_frag_t;  // 8 bf16 (4 VGPRs): one lane's share of an MFMA operand

// 1.0; a fragment of it as one MFMA operand sums the other operand over k
#define MT_BF16_ONE ((bf16raw)0x3F80)

// Epilogue codes of gemm_kernel and linear_stream_kernel
#define EPI_F32 0        // fp32 store (atomicAdd when SPLITK)
#define EPI_BF16 1       // bf16 store
#define EPI_BIAS 2       // bf16 store, + bias[n]
#define EPI_BIAS_RELU 3  // bf16 store, + bias[n], relu
#define EPI_RELU 4       // bf16 store, relu (no bias)
#define EPI_F32_SLAB 5   // fp32 per-slice slab store (split-K without atomics;
                         // a separate reduce kernel combines the slabs —
                         // guide §5 "splitk-seam": slab reducer beats an
                         // fp32-atomicAdd accumulator)
#define EPI_BF16_MASK 6  // bf16 store, zeroed where mask[m][n] <= 0 (mask: bf16
                         // [M][N], same layout as C) — dgrad with the upstream
                         // ReLU backward folded in

// ---- waits ----

// The wave's memory instructions other than its newest N have completed
// (vmcnt retires in order) and so have its LDS reads and writes; then the
// block's barrier.  __syncthreads() would drain the DMAs that are meant to
// stay in flight.  What N may be is the call site's business: it asserts its
// DMA-per-wave constants there.
template <int N>
__device__ __forceinline__ void mt_wait_barrier() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

// LDS-only publish: every DMA stays in flight
__device__ __forceinline__ void mt_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// ---- global -> LDS DMA ----

// 16 B per lane: lane i's bytes land at lds + i * 16 (lds is wave-uniform)
__device__ __forceinline__ void mt_glds16(const bf16raw* g, bf16raw* lds) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) unsigned int*)g,
                                   (__attribute__((address_space(3))) unsigned int*)lds, 16, 0, 0);
}

// k-contiguous operand src[row0 + row][kt ..] (row stride ld) -> k-major image.
// Source rows row0 .. row0 + nrows - 1 must exist; nrows is a multiple of 16.
// PAD_ROWS = false: chunks past nrows are skipped.
// PAD_ROWS = true (nrows >= 64): image rows at or past nrows get copies of
// valid rows (never read), so that every wave issues the same
// ROWS * BKT * 2 / 1024 / WAVES instructions whatever nrows is.
// mlp_predict_kernel's counted waits rely on it.
template <int WAVES, int ROWS, int BKT, bool PAD_ROWS>
__device__ __forceinline__ void mt_dma_kmajor(const bf16raw* __restrict__ src,
                                              bf16raw* __restrict__ lds, int64_t row0, int nrows,
                                              int64_t ld, int kt, int wid, int lane) {
  constexpr int SLOTS = BKT / 8;       // 16 B slots per image row
  constexpr int CH_ROWS = 64 / SLOTS;  // rows per 1 KB wave chunk
  constexpr int NCHUNK = ROWS / CH_ROWS;
  static_assert(NCHUNK % WAVES == 0, "chunks are dealt evenly to the waves");
  const int r_in = lane / SLOTS;
  const int slot = lane % SLOTS;
#pragma unroll
  for (int c0 = 0; c0 < NCHUNK; c0 += WAVES) {
    const int c = c0 + wid;
    if (PAD_ROWS || c * CH_ROWS < nrows) {
      const int row = c * CH_ROWS + r_in;
      const int srow = PAD_ROWS ? (row < nrows ? row : (row & 63)) : row;
      const int sslot = slot ^ (row & (SLOTS - 1));
      const bf16raw* g = src + (row0 + srow) * ld + kt + sslot * 8;
      mt_glds16(g, lds + c * CH_ROWS * BKT);
    }
  }
}

// the same image with zero fill: rows at or past rmax, k at or past kmax
// (K is a multiple of 8, so a slot is wholly inside or wholly outside)
template <int THREADS, int ROWS, int BKT>
__device__ __forceinline__ void mt_fill_kmajor(const bf16raw* __restrict__ src,
                                               bf16raw* __restrict__ lds, int64_t row0,
                                               int64_t rmax, int ld, int kt, int kmax, int t) {
  constexpr int SLOTS = BKT / 8;
#pragma unroll
  for (int u = t; u < ROWS * SLOTS; u += THREADS) {
    const int row = u / SLOTS;
    const int k = kt + (((u % SLOTS) ^ (row & (SLOTS - 1))) << 3);
    shortx8 v = {};
    if (row0 + row < rmax && k < kmax) v = *(const shortx8*)(src + (row0 + row) * ld + k);
    *(shortx8*)(lds + u * 8) = v;
  }
}

// ---- fragments ----

// ds_read_b128 of a row-major image with row stride STRIDE whose 16 B slots
// are XOR-swizzled by (row & XM): the lane's 8 consecutive k of slot `slot`
template <int STRIDE, int XM>
__device__ __forceinline__ mt_frag_t mt_ld_frag(const bf16raw* img, int row, int slot) {
  return *(const mt_frag_t*)&img[row * STRIDE + ((slot ^ (row & XM)) << 3)];
}

// Transposing read (ds_read_b64_tr_b16) of an image stored as it lies in
// memory, [k-row][column] with row stride STRIDE, 16 B slots XOR-ed by
// KEY::key(row): fragment value jh*4 + j of lane (l15, lane group g) is image
// row rb + g * GSTEP + jh * JSTEP + j, column col0 + l15.  GSTEP = 8,
// JSTEP = 4 is the k-packing above (group g gets k = 8g .. 8g+7 of the step
// at rb); GSTEP = 4, JSTEP = 16 pairs rows the same way for both operands of a
// product that reduces over them.
template <int STRIDE, int GSTEP, int JSTEP, typename KEY>
__device__ __forceinline__ mt_frag_t mt_tr_frag(const bf16raw* __restrict__ img, int rb, int g,
                                                int l15, int col0) {
  mt_frag_t f;
  const int col = col0 + 4 * (l15 & 3);
#pragma unroll
  for (int jh = 0; jh < 2; ++jh) {
    const int row = rb + g * GSTEP + jh * JSTEP + (l15 >> 2);
    const bf16raw* p = img + row * STRIDE + ((((col >> 3) ^ KEY::key(row)) << 3) | (col & 7));
    shortx4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) shortx4*)p);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[jh * 4 + j] = v[j];
  }
  return f;
}

// one 32-wide k-step of a wave's (16 MF) x (16 NF) sub-tile
template <int MF, int NF>
__device__ __forceinline__ void mt_mma_tile(floatx4 (&acc)[MF][NF], const mt_frag_t (&a)[MF],
                                            const mt_frag_t (&b)[NF]) {
#pragma unroll
  for (int mi = 0; mi < MF; ++mi)
#pragma unroll
    for (int ni = 0; ni < NF; ++ni)
      acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
}

// ---- small-head forward (C <= 16 classes): one wave per 16 rows ----
//
// logits[16 rows][class] = A[16][H] w[C][H]^T, K ascending in 32-wide steps
// ks; lane (class l15, kg) receives rows kg*4 .. kg*4+3.  The caller rounds
// lg + bias with f32_to_bf16: what gemm_kernel's EPI_BIAS stores.

// w as k-ascending B fragments held in registers: lane (class l15, kg) holds
// k = ks*32 + kg*8 .. +7; classes at or past C and k at or past H are zero
template <int NK>
__device__ __forceinline__ void mt_head_w_frags(mt_frag_t (&wk)[NK], const bf16raw* w, int H,
                                                int C, int l15, int kg) {
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) {
    wk[ks] = mt_frag_t{};
    if (ks * 32 < H && l15 < C) wk[ks] = *(const mt_frag_t*)&w[l15 * H + ks * 32 + kg * 8];
  }
}

// the A fragments: row arow of an image with row stride STRIDE, slots XOR-ed
// by row & XM, all NK * 32 columns live
template <int NK, int STRIDE, int XM>
__device__ __forceinline__ void mt_head_a_frags(mt_frag_t (&ay)[NK], const bf16raw* img,
                                                int arow, int kg) {
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) ay[ks] = mt_ld_frag<STRIDE, XM>(img, arow, ks * 4 + kg);
}

// logits from A fragments read earlier (mt_head_a_frags, under a DMA) ...
template <int NK>
__device__ __forceinline__ floatx4 mt_head_logits(const mt_frag_t (&ay)[NK],
                                                  const mt_frag_t (&wk)[NK]) {
  floatx4 lg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < NK; ++ks)
    lg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ay[ks], wk[ks], lg, 0, 0, 0);
  return lg;
}

// ... or each read just before its MFMA, columns at or past H left out
template <int NK, int STRIDE, int XM>
__device__ __forceinline__ floatx4 mt_head_logits(const mt_frag_t (&wk)[NK], const bf16raw* img,
                                                  int arow, int H, int kg) {
  floatx4 lg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) {
    if (ks * 32 < H) {
      const mt_frag_t ay = mt_ld_frag<STRIDE, XM>(img, arow, ks * 4 + kg);
      lg = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ay, wk[ks], lg, 0, 0, 0);
    }
  }
  return lg;
}

// ---- bf16 epilogue ----
//
// The MFMA accumulator layout (column = lane & 15, row = 4 * (lane >> 4) + r)
// cannot give contiguous per-lane stores, so each 16-row slice of a wave's
// sub-tile goes through a per-wave [16][MT_EPAD] fp32 scratch and every lane
// stores 16 contiguous bytes (scalar 2 B stores measured the C-write path at
// ~2.3 TB/s against ~4.4 for reads).

#define MT_EPAD 68
#define MT_EP_FLOATS (16 * MT_EPAD)  // scratch per wave

// One 16-row slice of a wave's 64-column sub-tile (accumulators acc[0 .. 3],
// 16 columns each) -> C[mout][n_base ..] for the bf16 EPI_* codes: + bias,
// relu, round to bf16, mask, in that order.  ep: the wave's MT_EP_FLOATS of
// idle LDS.  Lane `lane` stores columns (lane & 3) * 16 .. + 15 of slice row
// lane >> 2, and nothing unless `live`; mout is that row's place in C (and in
// mask).  All 64 columns must exist.
template <int EPI>
__device__ __forceinline__ void mt_epi_slice(float* ep, const floatx4 (&acc)[4], int lane,
                                             int l15, int kg, bool live, int64_t mout, int N,
                                             int n_base, bf16raw* C, const float* bias,
                                             const bf16raw* mask) {
  const int orow = lane >> 2;  // output row of the slice
  const int oct = lane & 3;    // which 16 columns of the wave's 64
  // mask octets are fetched before the slice goes through the scratch so the
  // global load overlaps the transpose
  shortx8 mk[2] = {};
  if (EPI == EPI_BF16_MASK && live) {
    const bf16raw* mp = mask + mout * N + n_base + oct * 16;
    mk[0] = *(const shortx8*)mp;
    mk[1] = *(const shortx8*)(mp + 8);
  }
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
#pragma unroll
    for (int r = 0; r < 4; ++r) ep[(kg * 4 + r) * MT_EPAD + ni * 16 + l15] = acc[ni][r];
  __builtin_amdgcn_s_waitcnt(0);  // own-wave LDS writes visible
  if (live) {
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
      *(shortx8*)(C + mout * N + n) = *(const shortx8*)outp;
    }
  }
  __builtin_amdgcn_s_waitcnt(0);  // all lanes done reading before reuse
}

// ---- block ids ----

// Bijective XCD-aware swizzle of the flattened (x, y) block id, gx = gridDim.x
// (guide §5.5 T1): hardware deals consecutive ids round-robin over the 8 XCDs; the
// returned id is consecutive within an XCD, so consecutive output tiles land
// on one XCD and their shared operand rows stay in that XCD's L2.
__device__ __forceinline__ int mt_xcd_block_id(int gx) {
  int nwg = gx * gridDim.y;
  int orig = blockIdx.y * gx + blockIdx.x;
  int q = nwg >> 3, rr = nwg & 7;
  return ((orig & 7) < rr ? (orig & 7) * (q + 1) : rr * (q + 1) + ((orig & 7) - rr) * q) +
         (orig >> 3);
}
