// Microbench: batch-streaming Linear wgrad+db (linear_wgrad.hip) against the
// split-K gemm_kernel route with the virtual ones column (gemm.hip).
// hipcc --offload-arch=gfx950 -O3 -ffast-math tools/linear_wgrad_bench.hip -o tools/linear_wgrad_bench
// usage: linear_wgrad_bench [B ...]      (default 2097152)
#include "../sparktorch_amd/ops/csrc/gemm.hip"
#include "../sparktorch_amd/ops/csrc/linear_wgrad.hip"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CKB(x) do { hipError_t e=(x); if(e!=hipSuccess){printf("err %s %d\n",hipGetErrorString(e),__LINE__);return 1;} } while(0)

__global__ void fill_kernel(bf16raw* p, int64_t n, uint32_t seed, int relu) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = (uint32_t)i * 2654435761u ^ (uint32_t)(i >> 32) * 40503u ^ seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    float v = ((int)(h & 255) - 128) / 128.f;  // exact in bf16
    if (relu && v < 0.f) v = 0.f;
    p[i] = f32_to_bf16(v);
  }
}

static int choose_splitk(int64_t batch, int n_out, int k_in) {
  int base = ((n_out + 127) / 128) * ((k_in + 127) / 128);
  int64_t want = 2048 / base; if (want < 1) want = 1;
  int64_t rows = batch / 512; if (rows < 1) rows = 1;
  int64_t s = want < rows ? want : rows;
  return (int)(s < 512 ? s : 512);
}

int main(int argc, char** argv) {
  std::vector<int64_t> batches;
  for (int i = 1; i < argc; ++i) batches.push_back(atoll(argv[i]));
  if (batches.empty()) batches.push_back(2097152);
  int cus = 256;
  CKB(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  struct S { int No, Ki; } shapes[] = {{256, 784}, {256, 256}};
  const int WARM = 3, REPS = 20;
  for (int64_t B : batches)
    for (auto& s : shapes) {
      bf16raw *dz, *x; float *dw[2], *db[2];
      CKB(hipMalloc(&dz, B * s.No * 2));
      CKB(hipMalloc(&x, B * s.Ki * 2));
      for (int v = 0; v < 2; ++v) {
        CKB(hipMalloc(&dw[v], s.No * s.Ki * 4));
        CKB(hipMalloc(&db[v], s.No * 4));
      }
      fill_kernel<<<2048, 256>>>(dz, B * s.No, 1u, 0);
      fill_kernel<<<2048, 256>>>(x, B * s.Ki, 2u, 1);
      CKB(hipDeviceSynchronize());
      const int sk = choose_splitk(B, s.No, s.Ki);
      hipEvent_t e0, e1; CKB(hipEventCreate(&e0)); CKB(hipEventCreate(&e1));
      float us[2];
      for (int v = 0; v < 2; ++v) {
        for (int it = 0; it < WARM + REPS; ++it) {
          if (it == WARM) CKB(hipEventRecord(e0));
          if (it == WARM + REPS - 1) {  // last call's result is the one compared
            CKB(hipMemsetAsync(dw[v], 0, s.No * s.Ki * 4));
            CKB(hipMemsetAsync(db[v], 0, s.No * 4));
          }
          if (v == 0)
            CKB(launch_gemm_bf16(dz, x, 0, dw[0], nullptr, nullptr, s.No, s.Ki + 1, (int)B, 1, s.No,
                                 s.Ki, 1, 0, -sk, db[0], s.Ki, 0));
          else
            CKB(launch_linear_wgrad_stream(dz, x, dw[1], db[1], B, s.No, s.Ki, 0, cus, 0));
        }
        CKB(hipEventRecord(e1)); CKB(hipEventSynchronize(e1));
        float ms; CKB(hipEventElapsedTime(&ms, e0, e1));
        us[v] = ms * 1000.f / REPS;
      }
      std::vector<float> h0(s.No * s.Ki), h1(s.No * s.Ki), b0(s.No), b1(s.No);
      CKB(hipMemcpy(h0.data(), dw[0], h0.size() * 4, hipMemcpyDeviceToHost));
      CKB(hipMemcpy(h1.data(), dw[1], h1.size() * 4, hipMemcpyDeviceToHost));
      CKB(hipMemcpy(b0.data(), db[0], b0.size() * 4, hipMemcpyDeviceToHost));
      CKB(hipMemcpy(b1.data(), db[1], b1.size() * 4, hipMemcpyDeviceToHost));
      double dmax = 0, rmax = 0, bd = 0, br = 0;
      for (size_t i = 0; i < h0.size(); ++i) { dmax = fmax(dmax, fabs(h0[i] - h1[i])); rmax = fmax(rmax, fabs(h0[i])); }
      for (size_t i = 0; i < b0.size(); ++i) { bd = fmax(bd, fabs(b0[i] - b1[i])); br = fmax(br, fabs(b0[i])); }
      const double bytes = (double)B * (s.No + s.Ki) * 2, flop = 2.0 * B * s.No * s.Ki;
      for (int v = 0; v < 2; ++v)
        printf("B=%8ld No=%3d Ki=%3d %-9s: %8.1f us  %5.2f TB/s  %6.1f TF/s\n", (long)B, s.No, s.Ki,
               v ? "stream" : "split-K", us[v], bytes / us[v] / 1e6, flop / us[v] / 1e6);
      printf("   max|dw_new-dw_old|/max|dw_old| = %.3g   db: %.3g\n", dmax / rmax, bd / br);
      hipFree(dz); hipFree(x);
      for (int v = 0; v < 2; ++v) { hipFree(dw[v]); hipFree(db[v]); }
    }
  return 0;
}
