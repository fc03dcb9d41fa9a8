// Microbench: full-N streaming Linear forward / dgrad+mask (linear_stream.hip)
// against gemm_kernel's 128x128-tile route (gemm.hip) at the flagship shapes.
// hipcc --offload-arch=gfx950 -O3 -ffast-math tools/linear_stream_bench.hip -o tools/linear_stream_bench
// usage: linear_stream_bench [M ...]      (default 2097152)
// Prints us and TB/s of NEEDED bytes (A once + C once (+ mask once)), and
// whether the two routes' outputs are bit-identical.
#include "../sparktorch_amd/ops/csrc/gemm.hip"
#include "../sparktorch_amd/ops/csrc/linear_stream.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CKB(x) do { hipError_t e=(x); if(e!=hipSuccess){printf("err %s %d\n",hipGetErrorString(e),__LINE__);return 1;} } while(0)

__global__ void fill_kernel(bf16raw* p, int64_t n, uint32_t seed, int relu, float scale) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = (uint32_t)i * 2654435761u ^ (uint32_t)(i >> 32) * 40503u ^ seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    float v = ((int)(h & 255) - 128) / 128.f * scale;
    if (relu && v < 0.f) v = 0.f;
    p[i] = f32_to_bf16(v);
  }
}

int main(int argc, char** argv) {
  std::vector<int64_t> ms;
  for (int i = 1; i < argc; ++i) ms.push_back(atoll(argv[i]));
  if (ms.empty()) ms.push_back(2097152);
  // fwd: C[M,N] = A[M,K] W[N,K]^T + b, relu;  dgrad: C[M,N] = A[M,K] W[K,N], masked
  struct S { const char* name; int K, N, dgrad; } shapes[] = {
      {"fwd   784->256", 784, 256, 0}, {"fwd   256->256", 256, 256, 0},
      {"dgrad 256->256", 256, 256, 1}};
  const int WARM = 2, REPS = 10;
  for (int64_t M : ms)
    for (auto& s : shapes) {
      bf16raw *a, *w, *mask, *c[3]; float* bias;
      CKB(hipMalloc(&a, M * s.K * 2));
      CKB(hipMalloc(&w, (size_t)s.K * s.N * 2));
      CKB(hipMalloc(&mask, M * s.N * 2));
      CKB(hipMalloc(&bias, s.N * 4));
      for (int v = 0; v < 3; ++v) CKB(hipMalloc(&c[v], M * s.N * 2));
      fill_kernel<<<2048, 256>>>(a, M * s.K, 1u, !s.dgrad, 1.f);
      fill_kernel<<<64, 256>>>(w, (int64_t)s.K * s.N, 2u, 0, 0.0625f);
      fill_kernel<<<2048, 256>>>(mask, M * s.N, 3u, 1, 1.f);
      CKB(hipMemset(bias, 0, s.N * 4));
      CKB(hipDeviceSynchronize());
      hipEvent_t e0, e1; CKB(hipEventCreate(&e0)); CKB(hipEventCreate(&e1));
      float us[3];
      const char* names[3] = {"gemm 128x128", "stream BK=32", "stream BK=64"};
      for (int v = 0; v < 3; ++v) {
        for (int it = 0; it < WARM + REPS; ++it) {
          if (it == WARM) CKB(hipEventRecord(e0));
          if (v == 0) {
            if (s.dgrad)
              CKB(launch_gemm_bf16_mask(a, w, 0, nullptr, c[0], nullptr, (int)M, s.N, s.K, s.K, 1,
                                        s.N, 1, EPI_BF16_MASK, 1, nullptr, -1, mask, 0));
            else
              CKB(launch_gemm_bf16(a, w, 0, nullptr, c[0], bias, (int)M, s.N, s.K, s.K, 1, 1, s.K,
                                   EPI_BIAS_RELU, 1, nullptr, -1, 0));
          } else {
            CKB(launch_linear_stream(a, w, c[v], s.dgrad ? nullptr : bias,
                                     s.dgrad ? mask : nullptr, M, s.N, s.K,
                                     s.dgrad ? EPI_BF16_MASK : EPI_BIAS_RELU, s.dgrad,
                                     v == 1 ? 32 : 64, 0));
          }
        }
        CKB(hipEventRecord(e1)); CKB(hipEventSynchronize(e1));
        float t; CKB(hipEventElapsedTime(&t, e0, e1));
        us[v] = t * 1000.f / REPS;
      }
      // bit comparison on a prefix and a suffix (the whole C at small M)
      const size_t total = (size_t)M * s.N, chunk = total < (1u << 22) ? total : (1u << 22);
      bool same[3] = {true, true, true};
      std::vector<bf16raw> h0(chunk), h1(chunk);
      for (int v = 1; v < 3; ++v)
        for (int part = 0; part < 2; ++part) {
          const size_t off = part ? total - chunk : 0;
          CKB(hipMemcpy(h0.data(), c[0] + off, chunk * 2, hipMemcpyDeviceToHost));
          CKB(hipMemcpy(h1.data(), c[v] + off, chunk * 2, hipMemcpyDeviceToHost));
          if (memcmp(h0.data(), h1.data(), chunk * 2) != 0) same[v] = false;
        }
      const double bytes = (double)M * (s.K + s.N * (s.dgrad ? 2 : 1)) * 2;
      for (int v = 0; v < 3; ++v)
        printf("M=%8ld %s %-12s: %8.1f us  %5.2f TB/s needed  %6.1f TF/s%s\n", (long)M, s.name,
               names[v], us[v], bytes / us[v] / 1e6, 2.0 * M * s.K * s.N / us[v] / 1e6,
               v == 0 ? "" : (same[v] ? "  bits==gemm" : "  BITS DIFFER"));
      hipFree(a); hipFree(w); hipFree(mask); hipFree(bias);
      for (int v = 0; v < 3; ++v) hipFree(c[v]);
    }
  return 0;
}
