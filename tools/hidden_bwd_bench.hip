// Microbench: one-pass hidden-layer backward (hidden_bwd.hip) against the two
// launches it replaces: linear_stream.hip's masked dgrad and linear_wgrad.hip's
// dW+db, at (No, Ki) = (256, 256).
// hipcc --offload-arch=gfx950 -O3 -ffast-math -Xclang -target-feature -Xclang -packed-fp32-ops \
//   tools/hidden_bwd_bench.hip -o tools/hidden_bwd_bench
// usage: hidden_bwd_bench [B ...]      (default 2097152)
// Prints us per launch and TB/s of NEEDED bytes (dz + x_in in, dz_in out),
// whether dz_in is bit-identical to the pair's and the largest dW / db
// difference relative to the largest entry.
#include "../sparktorch_amd/ops/csrc/linear_stream.hip"
#include "../sparktorch_amd/ops/csrc/linear_wgrad.hip"
#include "../sparktorch_amd/ops/csrc/hidden_bwd.hip"
#include <cmath>
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

static double rel_diff(const std::vector<float>& a, const std::vector<float>& b) {
  double d = 0, m = 0;
  for (size_t i = 0; i < a.size(); ++i) {
    d = fmax(d, fabs((double)a[i] - b[i]));
    m = fmax(m, fabs((double)a[i]));
  }
  return d / (m + 1e-300);
}

int main(int argc, char** argv) {
  std::vector<int64_t> bs;
  for (int i = 1; i < argc; ++i) bs.push_back(atoll(argv[i]));
  if (bs.empty()) bs.push_back(2097152);
  const int No = 256, Ki = 256, WARM = 2, REPS = 10;
  int dev = 0, cus = 256;
  CKB(hipGetDevice(&dev));
  CKB(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  for (int64_t B : bs) {
    bf16raw *dz, *x, *w, *o[2]; float *dw[2], *db[2];
    CKB(hipMalloc(&dz, B * No * 2));
    CKB(hipMalloc(&x, B * Ki * 2));
    CKB(hipMalloc(&w, (size_t)No * Ki * 2));
    for (int v = 0; v < 2; ++v) {
      CKB(hipMalloc(&o[v], B * Ki * 2));
      CKB(hipMalloc(&dw[v], (size_t)No * Ki * 4));
      CKB(hipMalloc(&db[v], No * 4));
    }
    fill_kernel<<<2048, 256>>>(dz, B * No, 1u, 0, 1.f);
    fill_kernel<<<2048, 256>>>(x, B * Ki, 3u, 1, 1.f);
    fill_kernel<<<64, 256>>>(w, (int64_t)No * Ki, 2u, 0, 0.0625f);
    CKB(hipDeviceSynchronize());
    hipEvent_t e0, e1; CKB(hipEventCreate(&e0)); CKB(hipEventCreate(&e1));
    // v = 0: the pair; v = 1: fused.  The last launch of each starts from
    // zeroed dW / db so the results can be compared.
    float us[3] = {0, 0, 0};  // dgrad, wgrad, fused
    for (int v = 0; v < 3; ++v) {
      const int r = v == 2 ? 1 : 0;
      for (int it = 0; it < WARM + REPS + 1; ++it) {
        if (it == WARM) CKB(hipEventRecord(e0));
        if (it == WARM + REPS) {
          CKB(hipEventRecord(e1)); CKB(hipEventSynchronize(e1));
          float t; CKB(hipEventElapsedTime(&t, e0, e1));
          us[v] = t * 1000.f / REPS;
          CKB(hipMemset(dw[r], 0, (size_t)No * Ki * 4));
          CKB(hipMemset(db[r], 0, No * 4));
        }
        if (v == 0)
          CKB(launch_linear_stream(dz, w, o[0], nullptr, x, B, Ki, No, EPI_BF16_MASK, 1, 0, 0, 0));
        else if (v == 1)
          CKB(launch_linear_wgrad_stream(dz, x, dw[0], db[0], B, No, Ki, 0, cus, 0));
        else
          CKB(launch_hidden_bwd(dz, x, w, o[1], dw[1], db[1], B, No, Ki, 0, cus, 0));
      }
      CKB(hipDeviceSynchronize());
    }
    // dz_in bit comparison on a prefix and a suffix (the whole at small B)
    const size_t total = (size_t)B * Ki, chunk = total < (1u << 22) ? total : (1u << 22);
    bool same = true;
    std::vector<bf16raw> h0(chunk), h1(chunk);
    for (int part = 0; part < 2; ++part) {
      const size_t off = part ? total - chunk : 0;
      CKB(hipMemcpy(h0.data(), o[0] + off, chunk * 2, hipMemcpyDeviceToHost));
      CKB(hipMemcpy(h1.data(), o[1] + off, chunk * 2, hipMemcpyDeviceToHost));
      if (memcmp(h0.data(), h1.data(), chunk * 2) != 0) same = false;
    }
    std::vector<float> w0((size_t)No * Ki), w1((size_t)No * Ki), b0(No), b1(No);
    CKB(hipMemcpy(w0.data(), dw[0], w0.size() * 4, hipMemcpyDeviceToHost));
    CKB(hipMemcpy(w1.data(), dw[1], w1.size() * 4, hipMemcpyDeviceToHost));
    CKB(hipMemcpy(b0.data(), db[0], No * 4, hipMemcpyDeviceToHost));
    CKB(hipMemcpy(b1.data(), db[1], No * 4, hipMemcpyDeviceToHost));
    const double bytes = (double)B * (No + 2 * Ki) * 2;
    printf("B=%8ld dgrad+mask %8.1f us + wgrad %8.1f us = %8.1f us | fused %8.1f us  %5.2f TB/s "
           "needed  %s  dW diff %.1e  db diff %.1e\n",
           (long)B, us[0], us[1], us[0] + us[1], us[2], bytes / us[2] / 1e6,
           same ? "dz_in bits==pair" : "DZ_IN BITS DIFFER", rel_diff(w0, w1), rel_diff(b0, b1));
    hipFree(dz); hipFree(x); hipFree(w);
    for (int v = 0; v < 2; ++v) { hipFree(o[v]); hipFree(dw[v]); hipFree(db[v]); }
  }
  return 0;
}
