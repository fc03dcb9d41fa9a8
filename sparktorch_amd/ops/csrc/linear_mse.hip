// Forward of a wide output layer and its mean-squared-error loss in one pass
// (an autoencoder's last layer: N = the input width):
//
//   pred  = bf16( h[B,H] W[N,H]^T + bias[N] )     never stored unless asked for
//   dpred = bf16( 2 (pred - t) / (B N) )          t: bf16 [B,N]
//   loss  = sum (pred - t)^2 / (B N)              fp32 scalar
//
// linear_fwd -> mse_fused writes pred (2N bytes a row), reads it back and
// drops it, and gemm_kernel re-reads h once per 128 output columns.  Here h
// and the target are read once and dpred is written once: 2H + 4N bytes a row.
//
//   * persistent blocks of 8 waves stride over 128-row tiles of h.  A wave
//     owns 16 rows of the tile for the whole column walk and keeps them as
//     H / 32 A fragments in registers (32 VGPRs at H = 256), loaded straight
//     from memory in mfma_tile.h's k-packing: h never passes through LDS;
//   * W (L2-resident, N * H * 2 bytes) is streamed in chunks of
//     CW = 8192 / H columns: a 16 KB k-major image (mfma_tile.h's, one slab as
//     wide as H, slots XOR-ed by row) filled by global->LDS DMA through two
//     buffers, the next chunk in flight under this chunk's MFMAs and epilogue,
//     one barrier per chunk.  The walk is flat over (tile, chunk): the first
//     chunk of the next tile is staged under the last chunk of this one;
//   * a chunk is 16 columns x 8192 / H / 16 fragments per wave, one fp32
//     accumulator per output, K ascending in 32-wide steps: gemm_kernel's sum;
//   * the last chunk of a row is narrower when N % CW != 0.  Its MFMAs, loads
//     and stores stop at the last 16-column fragment that exists; image rows
//     past it are DMA copies of valid W rows (so every wave issues the same
//     two DMA instructions per chunk) and are never multiplied;
//   * epilogue, 32 columns at a time through the wave's [16][MT_EPAD] fp32
//     scratch: a lane gets 8 consecutive columns of one row, adds the bias,
//     rounds to bf16 (gemm_kernel's EPI_BIAS order), applies mse_fused_kernel's
//     arithmetic against the 16 B of the target it fetched into registers one
//     chunk earlier (ahead of that chunk's DMA), and stores 16 B of dpred;
//   * a wave's memory instructions after a chunk's DMA are the epilogue's
//     stores, NST of them when the wave has rows and the chunk is full: the
//     step's barrier waits with vmcnt(NST) and leaves them in flight.  Every
//     other step (a tail chunk, a wave past B, the A fragments of a new tile
//     issued after the stores) waits for everything.  (The compiler adds a
//     vmcnt(0) of its own in front of each chunk's first fragment read, so
//     today the DMA has landed before the MFMAs start: profiles/linear_mse.md);
//   * LDS: 2 x 16 KB W + 8 x 4352 B scratch = 66.8 KB, two blocks (16 waves)
//     a CU, 4 waves a SIMD and 128 registers a lane.  A 32 KB chunk leaves one
//     block a CU; profiles/linear_mse.md has the budget per instantiation;
//   * rows past B: their A fragments are zero, they load no target, store
//     nothing and add nothing to the loss; a wave wholly past B only helps
//     staging.  Each lane keeps a loss sum, each block issues one atomicAdd.
//
// The translation unit is compiled without packed fp32 instructions
// (v_pk_*_f32), as hidden_bwd.hip is: dpred keeps mse_fused_kernel's bits.

#include "launchers.h"
#include "mfma_tile.h"

#define LM_THREADS 512
#define LM_WAVES 8
#define LM_BM 128
#define LM_CHUNK_EL 8192  // bf16 elements of one W chunk image

// LDS-only wait of one wave on itself (the scratch transpose): the W DMA and
// the stores stay in flight, which __builtin_amdgcn_s_waitcnt(0) would drain
__device__ __forceinline__ void lm_lds_wait() {
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0), vmcnt and expcnt unconstrained
}

// mt_wait_barrier<N> as builtins.  This kernel also loads registers (the
// target, the A fragments) inside its chunk loop; the compiler cannot see
// through an asm wait, takes those loads and the DMA for still pending after
// it and puts a vmcnt(0) of its own in front of the next fragment read.  It
// does account for a wait instruction it can see.
template <int N>
__device__ __forceinline__ void lm_wait_barrier() {
  static_assert(N >= 0 && N < 16, "vmcnt's low four bits");
  __builtin_amdgcn_s_waitcnt(0x0070 | N);  // vmcnt(N) lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
}

// W columns n0 .. n0 + ncols - 1 -> rows of a chunk image (k-major, one slab
// as wide as H, slot ^= row & XM); image rows at or past ncols copy row
// (row & 15) of the chunk, which exists (ncols >= 16).  __restrict__ is what
// lets the compiler tell this DMA's target from the image being read.
template <int H, int XM, int W_DMA>
__device__ __forceinline__ void lm_dma_w(const bf16raw* __restrict__ w, bf16raw* __restrict__ img,
                                         int n0, int ncols, int wid, int lane) {
#pragma unroll
  for (int i = 0; i < W_DMA; ++i) {
    const int ch = wid + i * LM_WAVES;
    const int o = ch * 1024 + lane * 16;
    const int row = o / (H * 2);
    const int sslot = ((o % (H * 2)) >> 4) ^ (row & XM);
    const int srow = row < ncols ? row : (row & 15);
    mt_glds16(w + (int64_t)(n0 + srow) * H + sslot * 8, img + ch * 512);
  }
}

template <int H, bool PRED>
__global__ __launch_bounds__(LM_THREADS, 4) void linear_mse_kernel(
    const bf16raw* __restrict__ h, const bf16raw* __restrict__ w, const float* __restrict__ bias,
    const bf16raw* __restrict__ target, bf16raw* __restrict__ dpred, bf16raw* __restrict__ pred,
    float* __restrict__ loss, int B, int N, float inv_n) {
  constexpr int CW = LM_CHUNK_EL / H;  // columns per chunk
  constexpr int NF = CW / 16;          // fragments per wave and chunk
  constexpr int NG = CW / 32;          // 32-column epilogue groups
  constexpr int NK = H / 32;           // MFMA k-steps
  constexpr int XM = H / 8 >= 16 ? 15 : 7;  // slot ^= row & XM
  constexpr int W_DMA = LM_CHUNK_EL * 2 / 1024 / LM_WAVES;
  constexpr int NST = NG * (PRED ? 2 : 1);  // 16 B stores per wave and full chunk
  static_assert(H == 64 || H == 128 || H == 256, "unsupported H");
  static_assert(W_DMA == 2 && NG >= 1, "1 KB DMA chunks are dealt evenly to the waves");

  __shared__ __attribute__((aligned(16))) bf16raw wimg[2 * LM_CHUNK_EL];
  bf16raw* const wimg0 = wimg;
  bf16raw* const wimg1 = wimg + LM_CHUNK_EL;
  __shared__ __attribute__((aligned(16))) float eps[LM_WAVES * MT_EP_FLOATS];
  __shared__ float lred[LM_WAVES];

  const int t = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int l15 = lane & 15, kg = lane >> 4;
  const int orow = lane >> 2;       // epilogue: row of the wave's 16
  const int oc = (lane & 3) * 8;    // and first of 8 columns of a 32-column group
  const int ntiles = (int)(((int64_t)B + LM_BM - 1) / LM_BM);
  const int nch = (N + CW - 1) / CW;
  float* const ep = eps + wid * MT_EP_FLOATS;

  // the wave's 16 rows of a tile as A fragments: lane (row l15, kg) holds
  // k = 32 ks + 8 kg .. + 7
  mt_frag_t a[NK];
  auto load_a = [&](int tile) {
    const int64_t r = (int64_t)tile * LM_BM + wid * 16 + l15;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      a[ks] = mt_frag_t{};
      if (r < B) a[ks] = *(const mt_frag_t*)(h + r * H + ks * 32 + kg * 8);
    }
  };
  // the lane's 16 B of the target in each group of chunk c of a tile
  auto load_t = [&](shortx8 (&tv)[NG], int tile, int c) {
    const int64_t r = (int64_t)tile * LM_BM + wid * 16 + orow;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int n = c * CW + g * 32 + oc;
      tv[g] = shortx8{};
      if (r < B && n < N) tv[g] = *(const shortx8*)(target + r * N + n);
    }
  };

  int tile = blockIdx.x, c = 0;  // the launcher keeps the grid within ntiles
  float lsum = 0.f;
  shortx8 tc[NG];
  load_a(tile);
  load_t(tc, tile, 0);
  lm_dma_w<H, XM, W_DMA>(w, wimg0, 0, N < CW ? N : CW, wid, lane);
  lm_wait_barrier<0>();

  // Chunk c of `tile` from image wc, the next (tile, chunk) staged into wn.
  // False after the block's last chunk.  The images are compile-time
  // constants in each call so the compiler can tell the DMA target from the
  // image the fragment reads use.
  auto step = [&](const bf16raw* wc, bf16raw* wn) -> bool {
    int nc = c + 1, ntile = tile;
    if (nc == nch) {
      nc = 0;
      ntile = tile + gridDim.x;
    }
    const bool more = ntile < ntiles;
    const int n0 = c * CW;
    const int ncols = N - n0 < CW ? N - n0 : CW;
    const int64_t wrow0 = (int64_t)tile * LM_BM + wid * 16;
    const bool wave_live = wrow0 < B;

    shortx8 tn[NG];
    if (more) {
      load_t(tn, ntile, nc);  // ahead of the DMA: it may stay in flight too
      lm_dma_w<H, XM, W_DMA>(w, wn, nc * CW, N - nc * CW < CW ? N - nc * CW : CW, wid, lane);
    }

    if (wave_live) {
      floatx4 acc[1][NF] = {};
      if (ncols == CW) {
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
          const mt_frag_t ak[1] = {a[ks]};
          mt_frag_t b[NF];
#pragma unroll
          for (int ni = 0; ni < NF; ++ni) b[ni] = mt_ld_frag<H, XM>(wc, ni * 16 + l15, ks * 4 + kg);
          mt_mma_tile(acc, ak, b);
        }
      } else {
        // the row's last chunk: only the fragments that exist
#pragma unroll
        for (int ks = 0; ks < NK; ++ks)
#pragma unroll
          for (int ni = 0; ni < NF; ++ni)
            if (ni * 16 < ncols)
              acc[0][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a[ks], mt_ld_frag<H, XM>(wc, ni * 16 + l15, ks * 4 + kg), acc[0][ni], 0, 0, 0);
      }

      const int64_t r = wrow0 + orow;
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        if (g * 32 < ncols) {
          // accumulator lane (column l15, kg), element r <-> row 4 kg + r
#pragma unroll
          for (int f = 0; f < 2; ++f)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              ep[(kg * 4 + e) * MT_EPAD + f * 16 + l15] = acc[0][g * 2 + f][e];
          lm_lds_wait();  // own-wave LDS writes visible
          const int n = n0 + g * 32 + oc;
          if (r < B && n < N) {
            const float* src = ep + orow * MT_EPAD + oc;
            floatx4 bv[2] = {};
            if (bias != nullptr) {
              bv[0] = *(const floatx4*)(bias + n);
              bv[1] = *(const floatx4*)(bias + n + 4);
            }
            alignas(16) short pb[8], dp[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              float val = src[j];
              if (bias != nullptr) val += bv[j >> 2][j & 3];
              const bf16raw p = f32_to_bf16(val);
              // mse_fused_kernel's arithmetic on the rounded pred
              const float d = bf16_to_f32(p) - bf16_to_f32((bf16raw)tc[g][j]);
              lsum += d * d * inv_n;
              pb[j] = (short)p;
              dp[j] = (short)f32_to_bf16(2.f * d * inv_n);
            }
            if (PRED) *(shortx8*)(pred + r * N + n) = *(const shortx8*)pb;
            *(shortx8*)(dpred + r * N + n) = *(const shortx8*)dp;
          }
          lm_lds_wait();  // all lanes done reading before the scratch is reused
        }
      }
    }

    if (!more) return false;
    // the only place the A fragments change: after their last use, and after
    // the stores, so this step's wait below is the full one
    if (nc == 0) load_a(ntile);
#pragma unroll
    for (int g = 0; g < NG; ++g) tc[g] = tn[g];
    // chunk (ntile, nc) has landed in every wave's share and every wave is
    // done with wc
    if (wave_live && ncols == CW && nc != 0)
      lm_wait_barrier<NST>();
    else
      lm_wait_barrier<0>();
    tile = ntile;
    c = nc;
    return true;
  };

  while (step(wimg0, wimg1) && step(wimg1, wimg0)) {
  }

  // one loss atomic per block
#pragma unroll
  for (int off = 32; off; off >>= 1) lsum += __shfl_xor(lsum, off, 64);
  if (lane == 0) lred[wid] = lsum;
  __syncthreads();
  if (t == 0) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LM_WAVES; ++i) s += lred[i];
    if (s != 0.f) atomicAdd(loss, s);
  }
}

// the loss scalar's zero, as a launch: a graph capture records kernels only
__global__ void linear_mse_zero_loss_kernel(float* loss) { *loss = 0.f; }

// 1 when the kernel serves an H -> N layer
extern "C" int linear_mse_supported(int N, int H) {
  return (H == 64 || H == 128 || H == 256) && N >= 32 && N % 16 == 0;
}

// Rows from which functional.linear_mse routes a served shape here: the
// smallest B at which tools/linear_mse_bench.hip measured this kernel not
// slower than gemm_kernel's forward + mse_fused_kernel at 256 -> 784
// (profiles/linear_mse.md, "Threshold": at 512 rows 36.8 us against 35.2, at
// 1024 rows 37.0 against 41.6).  A block walks its tile's 25 chunks one after
// the other, so four tiles take as long as one.
#define LM_MIN_ROWS 1024
extern "C" int64_t linear_mse_min_rows() { return LM_MIN_ROWS; }

// columns of one W chunk at width H: a row's last chunk is narrower when N is
// no multiple of it (tests pick N around it)
extern "C" int linear_mse_chunk_cols(int H) { return H > 0 ? LM_CHUNK_EL / H : 0; }

// h [B,H], w [N,H], target / dpred / pred [B,N] bf16, 16-byte aligned; bias
// fp32 [N] or null; pred null unless wanted.  loss is defined, not
// accumulated: a one-thread kernel zeroes it on the stream first.  max_blocks
// > 0 caps the grid (tests force several tiles per block with it).
extern "C" hipError_t launch_linear_mse(const bf16raw* h, const bf16raw* w, const float* bias,
                                        const bf16raw* target, bf16raw* dpred, bf16raw* pred,
                                        float* loss, int B, int N, int H, int max_blocks,
                                        int num_cus, hipStream_t stream) {
  if (!linear_mse_supported(N, H) || B < 1) return hipErrorInvalidValue;
  if ((((uintptr_t)h) | ((uintptr_t)w) | ((uintptr_t)target) | ((uintptr_t)dpred) |
       ((uintptr_t)pred) | ((uintptr_t)bias)) & 15)
    return hipErrorInvalidValue;
  const int ntiles = (int)(((int64_t)B + LM_BM - 1) / LM_BM);
  int grid = 2 * (num_cus > 0 ? num_cus : 256);
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  if (grid > ntiles) grid = ntiles;
  const float inv_n = 1.0f / ((int64_t)B * N);
  linear_mse_zero_loss_kernel<<<dim3(1), dim3(1), 0, stream>>>(loss);
#define LM_LAUNCH(HH)                                                                       \
  do {                                                                                      \
    if (pred != nullptr)                                                                    \
      linear_mse_kernel<HH, true><<<dim3(grid), dim3(LM_THREADS), 0, stream>>>(             \
          h, w, bias, target, dpred, pred, loss, B, N, inv_n);                              \
    else                                                                                    \
      linear_mse_kernel<HH, false><<<dim3(grid), dim3(LM_THREADS), 0, stream>>>(            \
          h, w, bias, target, dpred, nullptr, loss, B, N, inv_n);                           \
  } while (0)
  switch (H) {
    case 64: LM_LAUNCH(64); break;
    case 128: LM_LAUNCH(128); break;
    default: LM_LAUNCH(256); break;
  }
#undef LM_LAUNCH
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
