// Minibatch draw + row gather in one launch:
//
//   idx[j] = P_{seed,t}(j)                 j = 0..k-1, t read from device memory
//   xb[j, :] = x[idx[j], :]                bf16 or fp32 rows
//   yb[j, :] = y[idx[j], :]                optional labels, 4- or 8-byte elements
//
// P is the keyed bijection on [0, n) specified in
// sparktorch_amd/utils/sampling.py (offset + 6-round balanced Feistel network
// over 2^b >= n values, cycle-walked back below n); that docstring is the
// definition and the Python there is the oracle.  Each output slot is
// computed on its own, so the batch is drawn without replacement with no
// sort, no atomics and no traffic between waves.
//
//   * t comes from step_dev, not from a launch argument: a captured launch
//     followed by a captured increment_i32 draws a new batch on every replay.
//   * A wave owns output rows j = wave, wave + nwaves, ...  The wave id goes
//     through readfirstlane, so the whole index computation (hashes and the
//     cycle walk) is wave-uniform and costs no vector work.
//   * The row copy is 16 B per lane (1568 B MNIST rows: 98 granules, two
//     loads in flight per lane) when the row size and all three base pointers
//     allow it, else one element per lane.  Labels travel as 32-bit words.
//   * The next row's index is drawn between this row's loads and stores, so
//     the scalar chain runs under the loads' latency.
//   * Persistent grid-stride grid: up to 8 blocks of 4 waves per CU.
//
// Measured (tools/sample_gather_bench.hip, n = 2 097 152 x 784 bf16,
// k = 131072): 3.6-4.0 TB/s against 5.3-5.4 TB/s for a plain copy of the same
// bytes.  With the draw still computed but the rows taken in order the same
// kernel reaches the copy's figure, so the gap is what HBM gives scattered
// 1568 B rows, not the kernel; half the grid and non-temporal accesses moved
// it by 3 % or less.

#include "common.h"

#define SG_ROUNDS 6
#define SG_THREADS 256
#define SG_BLOCKS_PER_CU 8

typedef uint32_t sg_u4 __attribute__((ext_vector_type(4)));  // one 16 B granule

struct sg_keys {
  uint32_t rk[SG_ROUNDS];
  uint32_t offset, mask, hmask;
  int h, fshift;
};

// one application of the offset + Feistel network on [0, 2^(2h))
__host__ __device__ __forceinline__ uint32_t sg_network(uint32_t v, const sg_keys& K) {
  v = (v + K.offset) & K.mask;
  uint32_t l = v >> K.h, r = v & K.hmask;
#pragma unroll
  for (int i = 0; i < SG_ROUNDS; ++i) {
    const uint32_t f = (hash_u32(r, K.rk[i]) >> K.fshift) & K.hmask;
    const uint32_t nr = l ^ f;
    l = r;
    r = nr;
  }
  return (l << K.h) | r;
}

__host__ __device__ __forceinline__ sg_keys sg_make_keys(uint32_t t, uint32_t seed, int h) {
  sg_keys K;
  const uint32_t key = hash_u32(t, seed);
#pragma unroll
  for (int i = 0; i < SG_ROUNDS; ++i) K.rk[i] = hash_u32((uint32_t)i + 1u, key);
  K.h = h;
  K.mask = h == 16 ? 0xFFFFFFFFu : (1u << (2 * h)) - 1u;
  K.hmask = (1u << h) - 1u;
  K.fshift = (32 - h) >> 1;
  K.offset = hash_u32(0u, key) & K.mask;
  return K;
}

// T: the element of x as raw bits (uint16_t / uint32_t).  F elements per x
// row, yw 32-bit words per label row.  vec: rows are whole 16 B granules and
// x / xb are 16 B aligned.
template <typename T>
__global__ __launch_bounds__(SG_THREADS) void sample_gather_kernel(
    const T* __restrict__ x, const uint32_t* __restrict__ y, T* __restrict__ xb,
    uint32_t* __restrict__ yb, int* __restrict__ idx_out, const int* __restrict__ step_dev,
    uint32_t seed, uint32_t n, int k, int F, int yw, int h, int vec) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave =
      __builtin_amdgcn_readfirstlane((int)((blockIdx.x * SG_THREADS + threadIdx.x) / WAVE));
  const int nwaves = gridDim.x * (SG_THREADS / WAVE);
  const sg_keys K = sg_make_keys((uint32_t)*step_dev, seed, h);

  auto draw = [&](int j) {
    uint32_t v = (uint32_t)j;
    do {
      v = sg_network(v, K);
    } while (v >= n);
    return v;
  };

  uint32_t v = wave < k ? draw(wave) : 0u;
  for (int j = wave; j < k; j += nwaves) {
    const size_t src = (size_t)v * F, dst = (size_t)j * F;
    const uint32_t cur = v;
    // The next row's index is scalar work with no memory behind it: placed
    // between this row's loads and stores it runs while the loads are in flight.
    if (vec) {
      const sg_u4* __restrict__ s = (const sg_u4*)(x + src);
      sg_u4* __restrict__ d = (sg_u4*)(xb + dst);
      const int G = (int)(F * sizeof(T) / 16);
      if (G <= 2 * WAVE) {
        const bool one = lane < G, two = lane + WAVE < G;
        sg_u4 a = {}, b = {};
        if (one) a = s[lane];
        if (two) b = s[lane + WAVE];
        if (j + nwaves < k) v = draw(j + nwaves);
        if (one) d[lane] = a;
        if (two) d[lane + WAVE] = b;
      } else {
        if (j + nwaves < k) v = draw(j + nwaves);
        for (int g = lane; g < G; g += 2 * WAVE) {
          const bool two = g + WAVE < G;
          const sg_u4 a = s[g];
          sg_u4 b = a;
          if (two) b = s[g + WAVE];
          d[g] = a;
          if (two) d[g + WAVE] = b;
        }
      }
    } else {
      if (j + nwaves < k) v = draw(j + nwaves);
      for (int c = lane; c < F; c += WAVE) xb[dst + c] = x[src + c];
    }
    if (y != nullptr) {
      for (int c = lane; c < yw; c += WAVE) yb[(size_t)j * yw + c] = y[(size_t)cur * yw + c];
    }
    if (idx_out != nullptr && lane == 0) idx_out[j] = (int)cur;
  }
}

// half the bit width of the Feistel domain: the smallest h >= 1 with 4^h >= n
extern "C" int sample_gather_half_bits(int64_t n) {
  int h = 1;
  while (h < 16 && (1LL << (2 * h)) < n) ++h;
  return h;
}

// x_es: element size of x (2 or 4); y_es: of y (4 or 8), y may be null.
extern "C" hipError_t launch_sample_gather(const void* x, int x_es, const void* y, int y_es,
                                           void* xb, void* yb, int* idx_out,
                                           const int* step_dev, uint32_t seed, int64_t n, int k,
                                           int F, int L, int num_cus, hipStream_t stream) {
  if (n < 1 || n >= (1LL << 31) || k < 0 || k > n || F < 1 || F >= (1 << 24) || L < 0 ||
      L >= (1 << 24))
    return hipErrorInvalidValue;
  if ((x_es != 2 && x_es != 4) || (y != nullptr && y_es != 4 && y_es != 8))
    return hipErrorInvalidValue;
  if ((y != nullptr) != (yb != nullptr)) return hipErrorInvalidValue;
  if (k == 0) return hipSuccess;
  const int h = sample_gather_half_bits(n);
  const int vec = ((size_t)F * x_es) % 16 == 0 && ((((uintptr_t)x) | ((uintptr_t)xb)) & 15) == 0;
  const int yw = y != nullptr ? L * (y_es / 4) : 0;
  const int waves_per_block = SG_THREADS / WAVE;
  int grid = (k + waves_per_block - 1) / waves_per_block;
  const int cap = SG_BLOCKS_PER_CU * (num_cus > 0 ? num_cus : 256);
  if (grid > cap) grid = cap;
  if (x_es == 2)
    sample_gather_kernel<uint16_t><<<grid, SG_THREADS, 0, stream>>>(
        (const uint16_t*)x, (const uint32_t*)y, (uint16_t*)xb, (uint32_t*)yb, idx_out, step_dev,
        seed, (uint32_t)n, k, F, yw, h, vec);
  else
    sample_gather_kernel<uint32_t><<<grid, SG_THREADS, 0, stream>>>(
        (const uint32_t*)x, (const uint32_t*)y, (uint32_t*)xb, (uint32_t*)yb, idx_out, step_dev,
        seed, (uint32_t)n, k, F, yw, h, vec);
  HIP_CHECK_LAUNCH();
  return hipSuccess;
}
