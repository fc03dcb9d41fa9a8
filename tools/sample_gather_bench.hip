// Microbench: minibatch draw + row gather (sample_gather.hip) against a plain
// device-to-device copy of as many bytes.
// hipcc --offload-arch=gfx950 -O3 tools/sample_gather_bench.hip -o tools/sample_gather_bench
// usage: sample_gather_bench [n [k ...]]     (default 2097152, k = 256 131072)
//
// Every timed launch reads its own step counter, so every launch draws other
// rows: the gather's reads come from HBM, not from a cache warmed by the
// launch before.  bytes/s counts each row once read and once written.
#include "../sparktorch_amd/ops/csrc/sample_gather.hip"
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CKB(x) do { hipError_t e=(x); if(e!=hipSuccess){printf("err %s %d\n",hipGetErrorString(e),__LINE__);return 1;} } while(0)

__global__ void fill_kernel(uint32_t* p, int64_t nwords, uint32_t seed) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nwords;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = hash_u32((uint32_t)i, seed ^ (uint32_t)(i >> 32));
}

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 2097152;
  std::vector<int> ks;
  for (int i = 2; i < argc; ++i) ks.push_back(atoi(argv[i]));
  if (ks.empty()) ks = {256, 131072};
  const int F = 784, L = 1, WARM = 5, REPS = 50;
  int cus = 256;
  CKB(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  bf16raw* x; float* y; int* steps;
  CKB(hipMalloc(&x, n * F * 2));
  CKB(hipMalloc(&y, n * L * 4));
  CKB(hipMalloc(&steps, (WARM + REPS) * sizeof(int)));
  fill_kernel<<<2048, 256>>>((uint32_t*)x, n * F / 2, 1u);
  fill_kernel<<<2048, 256>>>((uint32_t*)y, n * L, 2u);
  std::vector<int> hs(WARM + REPS);
  for (int i = 0; i < WARM + REPS; ++i) hs[i] = i;
  CKB(hipMemcpy(steps, hs.data(), hs.size() * sizeof(int), hipMemcpyHostToDevice));
  CKB(hipDeviceSynchronize());
  hipEvent_t e0, e1; CKB(hipEventCreate(&e0)); CKB(hipEventCreate(&e1));
  for (int k : ks) {
    if (k < 1 || k > n) { printf("k=%d out of range\n", k); return 1; }
    bf16raw* xb; float* yb; int* idx;
    const size_t row_bytes = (size_t)F * 2, bytes = (size_t)k * row_bytes;
    CKB(hipMalloc(&xb, bytes));
    CKB(hipMalloc(&yb, (size_t)k * L * 4));
    CKB(hipMalloc(&idx, (size_t)k * 4));
    float ms_g, ms_c;
    for (int it = 0; it < WARM + REPS; ++it) {
      if (it == WARM) CKB(hipEventRecord(e0));
      CKB(launch_sample_gather(x, 2, y, 4, xb, yb, nullptr, steps + it, 12345u, n, k, F, L, cus, 0));
    }
    CKB(hipEventRecord(e1)); CKB(hipEventSynchronize(e1));
    CKB(hipEventElapsedTime(&ms_g, e0, e1));
    // plain copy of the same number of bytes from a moving window of x
    for (int it = 0; it < WARM + REPS; ++it) {
      if (it == WARM) CKB(hipEventRecord(e0));
      const size_t off = ((size_t)it * bytes) % ((size_t)n * row_bytes - bytes + 1) / 16 * 16;
      CKB(hipMemcpyAsync(xb, (const char*)x + off, bytes, hipMemcpyDeviceToDevice, 0));
    }
    CKB(hipEventRecord(e1)); CKB(hipEventSynchronize(e1));
    CKB(hipEventElapsedTime(&ms_c, e0, e1));
    // spot check: the last launch's rows against the host rule
    CKB(launch_sample_gather(x, 2, y, 4, xb, yb, idx, steps + 1, 12345u, n, k, F, L, cus, 0));
    std::vector<int> hidx(k);
    CKB(hipMemcpy(hidx.data(), idx, (size_t)k * 4, hipMemcpyDeviceToHost));
    const sg_keys K = sg_make_keys(1u, 12345u, sample_gather_half_bits(n));
    int bad = 0;
    for (int j = 0; j < k; ++j) {
      uint32_t v = (uint32_t)j;
      do v = sg_network(v, K); while (v >= (uint32_t)n);
      bad += (int)v != hidx[j];
    }
    const double ug = ms_g * 1e3 / REPS, uc = ms_c * 1e3 / REPS;
    printf("n=%ld k=%6d F=%d bf16: gather %8.2f us %7.3f TB/s | copy %8.2f us %7.3f TB/s | idx %s\n",
           (long)n, k, F, ug, 2.0 * bytes / ug * 1e-6, uc, 2.0 * bytes / uc * 1e-6,
           bad ? "MISMATCH" : "ok");
    CKB(hipFree(xb)); CKB(hipFree(yb)); CKB(hipFree(idx));
    if (bad) return 1;
  }
  return 0;
}
