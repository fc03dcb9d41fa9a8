// Microbench: wide-layer streaming Linear wgrad+db (linear_wgrad_wide.hip)
// against the split-K gemm_kernel route with the virtual ones column
// (gemm.hip).  The two routes alternate inside every run; three runs per
// batch and shape.
// hipcc --offload-arch=gfx950 -O3 -ffast-math tools/linear_wgrad_wide_bench.hip -o tools/linear_wgrad_wide_bench
// usage: linear_wgrad_wide_bench No Ki [B ...]      (default 784 256 131072)
#include "../sparktorch_amd/ops/csrc/gemm.hip"
#include "../sparktorch_amd/ops/csrc/linear_wgrad_wide.hip"
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

__global__ void zero_kernel(float* p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0.f;
}

static int choose_splitk(int64_t batch, int n_out, int k_in) {
  int base = ((n_out + 127) / 128) * ((k_in + 127) / 128);
  int64_t want = 2048 / base; if (want < 1) want = 1;
  int64_t rows = batch / 512; if (rows < 1) rows = 1;
  int64_t s = want < rows ? want : rows;
  return (int)(s < 512 ? s : 512);
}

int main(int argc, char** argv) {
  const int No = argc > 1 ? atoi(argv[1]) : 784, Ki = argc > 2 ? atoi(argv[2]) : 256;
  std::vector<int64_t> batches;
  for (int i = 3; i < argc; ++i) batches.push_back(atoll(argv[i]));
  if (batches.empty()) batches.push_back(131072);
  if (!linear_wgrad_wide_can_run(No, Ki, 1)) { printf("unsupported (No, Ki)\n"); return 1; }
  int cus = 256;
  CKB(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  const int WARM = 3, REPS = 10, RUNS = 3, ROUNDS = 2;
  hipEvent_t e0, e1; CKB(hipEventCreate(&e0)); CKB(hipEventCreate(&e1));
  for (int64_t B : batches) {
    bf16raw *dz, *x; float *dw[2], *db[2];
    CKB(hipMalloc(&dz, B * No * 2));
    CKB(hipMalloc(&x, B * Ki * 2));
    for (int v = 0; v < 2; ++v) {
      CKB(hipMalloc(&dw[v], No * Ki * 4));
      CKB(hipMalloc(&db[v], No * 4));
    }
    fill_kernel<<<2048, 256>>>(dz, B * No, 1u, 0);
    fill_kernel<<<2048, 256>>>(x, B * Ki, 2u, 1);
    CKB(hipDeviceSynchronize());
    const int sk = choose_splitk(B, No, Ki);
    auto launch = [&](int v) -> hipError_t {
      if (v == 0)
        return launch_gemm_bf16(dz, x, 0, dw[0], nullptr, nullptr, No, Ki + 1, (int)B, 1, No, Ki,
                                1, 0, -sk, db[0], Ki, 0);
      return launch_linear_wgrad_wide(dz, x, dw[1], db[1], B, No, Ki, 0, cus, 0);
    };
    const double bytes = (double)B * (No + Ki) * 2;
    for (int run = 0; run < RUNS; ++run) {
      // split-K, wide, split-K, wide: each route's time is the mean of its
      // ROUNDS timed groups of REPS launches
      float us[2] = {0.f, 0.f};
      for (int round = 0; round < ROUNDS; ++round)
        for (int v = 0; v < 2; ++v) {
          for (int it = 0; it < WARM; ++it) CKB(launch(v));
          CKB(hipEventRecord(e0));
          for (int it = 0; it < REPS; ++it) CKB(launch(v));
          CKB(hipEventRecord(e1)); CKB(hipEventSynchronize(e1));
          float ms; CKB(hipEventElapsedTime(&ms, e0, e1));
          us[v] += ms * 1000.f / REPS / ROUNDS;
        }
      printf("B=%8ld No=%4d Ki=%3d run %d: split-K %8.1f us %5.2f TB/s | wide %8.1f us %5.2f TB/s | x%.2f\n",
             (long)B, No, Ki, run, us[0], bytes / us[0] / 1e6, us[1], bytes / us[1] / 1e6,
             us[0] / us[1]);
    }
    // one clean call each: the results compared
    for (int v = 0; v < 2; ++v) {
      zero_kernel<<<(No * Ki + 255) / 256, 256>>>(dw[v], No * Ki);
      zero_kernel<<<(No + 255) / 256, 256>>>(db[v], No);
      CKB(launch(v));
    }
    CKB(hipDeviceSynchronize());
    std::vector<float> h0(No * Ki), h1(No * Ki), b0(No), b1(No);
    CKB(hipMemcpy(h0.data(), dw[0], h0.size() * 4, hipMemcpyDeviceToHost));
    CKB(hipMemcpy(h1.data(), dw[1], h1.size() * 4, hipMemcpyDeviceToHost));
    CKB(hipMemcpy(b0.data(), db[0], b0.size() * 4, hipMemcpyDeviceToHost));
    CKB(hipMemcpy(b1.data(), db[1], b1.size() * 4, hipMemcpyDeviceToHost));
    double dmax = 0, rmax = 0, bd = 0, br = 0;
    for (size_t i = 0; i < h0.size(); ++i) { dmax = fmax(dmax, fabs(h0[i] - h1[i])); rmax = fmax(rmax, fabs(h0[i])); }
    for (size_t i = 0; i < b0.size(); ++i) { bd = fmax(bd, fabs(b0[i] - b1[i])); br = fmax(br, fabs(b0[i])); }
    printf("   max|dw_new-dw_old|/max|dw_old| = %.3g   db: %.3g\n", dmax / rmax, bd / br);
    CKB(hipFree(dz)); CKB(hipFree(x));
    for (int v = 0; v < 2; ++v) { CKB(hipFree(dw[v])); CKB(hipFree(db[v])); }
  }
  return 0;
}
