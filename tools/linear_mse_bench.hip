// Microbench: one-pass wide-layer forward + mean squared error (linear_mse.hip)
// against the two launches it replaces: the layer's forward (gemm_kernel,
// EPI_BIAS, both operands by DMA) and mse_fused.  (The train step's third
// launch, torch's dpred * 1.0, has no counterpart here.)
// hipcc --offload-arch=gfx950 -O3 -ffast-math -Xclang -target-feature -Xclang -packed-fp32-ops
//   tools/linear_mse_bench.hip -o tools/linear_mse_bench
// usage: linear_mse_bench [N [H [B ...]]]   (default N = 784, H = 256, B = 2097152)
// Runs the two routes alternately, RUNS times each, and prints us per launch
// of every run, TB/s of NEEDED bytes (h once + target once + dpred once),
// whether pred and dpred are bit-identical and the loss difference.
#include "../sparktorch_amd/ops/csrc/gemm.hip"
#include "../sparktorch_amd/ops/csrc/loss.hip"
#include "../sparktorch_amd/ops/csrc/linear_mse.hip"
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

static bool same_bits(const bf16raw* a, const bf16raw* b, size_t n, bool* ok) {
  const size_t chunk = 1u << 24;
  std::vector<bf16raw> ha(chunk), hb(chunk);
  for (size_t off = 0; off < n; off += chunk) {
    const size_t m = n - off < chunk ? n - off : chunk;
    if (hipMemcpy(ha.data(), a + off, m * 2, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(hb.data(), b + off, m * 2, hipMemcpyDeviceToHost) != hipSuccess) {
      *ok = false;
      return false;
    }
    if (memcmp(ha.data(), hb.data(), m * 2) != 0) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  const int WARM = 2, REPS = 10, RUNS = 3;
  const int N = argc > 1 ? atoi(argv[1]) : 784;
  const int H = argc > 2 ? atoi(argv[2]) : 256;
  if (!linear_mse_supported(N, H)) { printf("unsupported (N, H)\n"); return 1; }
  std::vector<int64_t> bs;
  for (int i = 3; i < argc; ++i) bs.push_back(atoll(argv[i]));
  if (bs.empty()) bs.push_back(2097152);
  int cus = 256;
  CKB(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  for (int64_t B : bs) {
    if (B < 1 || B >= (1LL << 31)) { printf("bad B\n"); return 1; }
    bf16raw *y, *w, *tgt, *pred[2], *dpred[2];
    float *bias, *loss[2];
    CKB(hipMalloc(&y, B * H * 2));
    CKB(hipMalloc(&w, (size_t)N * H * 2));
    CKB(hipMalloc(&bias, N * 4));
    CKB(hipMalloc(&tgt, B * N * 2));
    for (int v = 0; v < 2; ++v) {
      CKB(hipMalloc(&pred[v], B * N * 2));
      CKB(hipMalloc(&dpred[v], B * N * 2));
      CKB(hipMalloc(&loss[v], 4));
    }
    fill_kernel<<<2048, 256>>>(y, B * H, 1u, 1, 1.f);
    fill_kernel<<<256, 256>>>(w, (int64_t)N * H, 2u, 0, 0.0625f);
    fill_kernel<<<2048, 256>>>(tgt, B * N, 3u, 0, 1.f);
    fill_kernel<<<4, 256>>>((bf16raw*)bias, (int64_t)N * 2, 4u, 0, 0.f);  // zeros
    CKB(hipDeviceSynchronize());
    hipEvent_t e0, e1; CKB(hipEventCreate(&e0)); CKB(hipEventCreate(&e1));
    // stage 0, 1: the replaced launches; 2: the fused kernel (with the launch
    // that zeroes its loss); 3: the fused kernel also writing pred
    const char* names[4] = {"fwd gemm_kernel", "mse_fused", "linear_mse_kernel",
                            "linear_mse_kernel+pred"};
    const double needed = (double)B * (2.0 * H + 4.0 * N);
    for (int run = 0; run < RUNS; ++run) {
      float us[4];
      for (int s = 0; s < 4; ++s) {
        for (int it = 0; it < WARM + REPS; ++it) {
          if (it == WARM) CKB(hipEventRecord(e0));
          if (s == 0)
            CKB(launch_gemm_bf16(y, w, 0, nullptr, pred[0], bias, (int)B, N, H, H, 1, 1, H,
                                 EPI_BIAS, 1, nullptr, -1, 0));
          else if (s == 1)
            CKB(launch_mse_fused(pred[0], tgt, loss[0], dpred[0], B * N, 0));
          else
            CKB(launch_linear_mse(y, w, bias, tgt, dpred[1], s == 3 ? pred[1] : nullptr, loss[1],
                                  (int)B, N, H, 0, cus, 0));
        }
        CKB(hipEventRecord(e1)); CKB(hipEventSynchronize(e1));
        float t; CKB(hipEventElapsedTime(&t, e0, e1));
        us[s] = t * 1000.f / REPS;
      }
      for (int s = 0; s < 4; ++s)
        printf("run %d B=%8ld H=%d N=%d %-24s: %8.1f us\n", run, (long)B, H, N, names[s], us[s]);
      printf("run %d B=%8ld replaced launches: %8.1f us   fused: %8.1f us  %5.2f TB/s needed\n",
             run, (long)B, us[0] + us[1], us[2], needed / us[2] / 1e6);
    }
    // one clean pass of each route for the comparison
    CKB(hipMemset(loss[0], 0, 4));
    CKB(launch_gemm_bf16(y, w, 0, nullptr, pred[0], bias, (int)B, N, H, H, 1, 1, H, EPI_BIAS, 1,
                         nullptr, -1, 0));
    CKB(launch_mse_fused(pred[0], tgt, loss[0], dpred[0], B * N, 0));
    CKB(launch_linear_mse(y, w, bias, tgt, dpred[1], pred[1], loss[1], (int)B, N, H, 0, cus, 0));
    CKB(hipDeviceSynchronize());
    bool ok = true;
    const bool pr_same = same_bits(pred[0], pred[1], (size_t)B * N, &ok);
    const bool dp_same = same_bits(dpred[0], dpred[1], (size_t)B * N, &ok);
    if (!ok) { printf("copy failed\n"); return 1; }
    float hl[2];
    for (int v = 0; v < 2; ++v) CKB(hipMemcpy(&hl[v], loss[v], 4, hipMemcpyDeviceToHost));
    printf("B=%8ld N=%d pred %s  dpred %s  loss %.7g vs %.7g (rel %.1e)\n", (long)B, N,
           pr_same ? "bits==" : "BITS DIFFER", dp_same ? "bits==" : "BITS DIFFER", hl[1], hl[0],
           fabs(hl[1] - hl[0]) / fabs(hl[0]));
    hipFree(y); hipFree(w); hipFree(bias); hipFree(tgt);
    for (int v = 0; v < 2; ++v) { hipFree(pred[v]); hipFree(dpred[v]); hipFree(loss[v]); }
  }
  return 0;
}
