// Shared device-side helpers for the sparktorch_amd CDNA4 (gfx950) kernels.
// Pure HIP: no torch headers here — launchers take raw pointers + hipStream_t.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "launchers.h"  // bf16raw

#define WAVE 64

__device__ __forceinline__ float bf16_to_f32(bf16raw h) {
  union {
    uint32_t u;
    float f;
  } c;
  c.u = ((uint32_t)h) << 16;
  return c.f;
}

// round-to-nearest-even f32 -> bf16
__device__ __forceinline__ bf16raw f32_to_bf16(float f) {
  union {
    float f;
    uint32_t u;
  } c;
  c.f = f;
  uint32_t u = c.u;
  uint32_t rounding = 0x7fff + ((u >> 16) & 1);
  u += rounding;
  return (bf16raw)(u >> 16);
}

// f32 -> bf16 of USER data (the cast kernels, mlp_predict.hip's fp32 rows):
// it may carry NaNs with any payload, and the rounding add of f32_to_bf16
// carries a low-payload NaN into Inf (0x7F800001) or across the sign into zero
// (0x7FFFFFFF).  A NaN becomes a quiet NaN of the same sign here; everything
// else rounds as there, which is what torch's cast stores.  The test is on the
// bits: the build's -ffast-math folds x != x away.  (Arithmetic NaNs are
// canonical 0x7FC00000 and survive f32_to_bf16, which the hot kernels keep.)
__device__ __forceinline__ bf16raw cast_f32_to_bf16(float f) {
  union {
    float f;
    uint32_t u;
  } c;
  c.f = f;
  const uint32_t nan = (c.u >> 16) | 0x0040u;
  const uint32_t rne = (c.u + 0x7fffu + ((c.u >> 16) & 1u)) >> 16;  // f32_to_bf16
  return (bf16raw)((c.u & 0x7fffffffu) > 0x7f800000u ? nan : rne);
}

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef short shortx8 __attribute__((ext_vector_type(8)));
typedef short shortx4 __attribute__((ext_vector_type(4)));

__host__ __device__ __forceinline__ int64_t ceil_div_i64(int64_t a, int64_t b) {
  return (a + b - 1) / b;
}

// Counter-based hash (murmur3 finalizer over a * golden + seed): dropout masks
// (conv.hip) and minibatch selection (sample_gather.hip; the same rule in
// Python is sparktorch_amd/utils/sampling.py).
__host__ __device__ __forceinline__ uint32_t hash_u32(uint32_t a, uint32_t seed) {
  uint32_t h = a * 0x9E3779B9u + seed;
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// Cross-entropy over C < 128 classes sums a row's exponentials by a lane
// butterfly up to this batch (ce_fused_wave_kernel) and class-ascending above
// it (ce_fused_kernel); head_bwd.hip's head_ce_kernel follows the same rule.
#define CE_WAVE_MAX_B 2048

#define HIP_CHECK_LAUNCH()                                        \
  do {                                                             \
    hipError_t err_ = hipGetLastError();                           \
    if (err_ != hipSuccess) return err_;                           \
  } while (0)
