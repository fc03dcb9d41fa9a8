// Microbench: one-pass head forward + cross-entropy + head backward
// (head_bwd.hip, head_ce_kernel) against the launches it replaces: the fc3
// forward (gemm_kernel, EPI_BIAS), ce_fused and head_bwd_kernel.  (The train
// step's fourth launch, torch's dlogits * 1.0, has no counterpart here.)
// hipcc --offload-arch=gfx950 -O3 -ffast-math tools/head_ce_bench.hip -o tools/head_ce_bench
// usage: head_ce_bench [B ...]      (default 2097152; H = 256, C = 10)
// Prints us per launch, TB/s of NEEDED bytes (y_in once + dz_in once +
// targets), whether dz_in and the logits are bit-identical, and the loss /
// dw / db differences (fp32 atomics: equal to rounding only).
#include "../sparktorch_amd/ops/csrc/gemm.hip"
#include "../sparktorch_amd/ops/csrc/loss.hip"
#include "../sparktorch_amd/ops/csrc/head_bwd.hip"
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

__global__ void fill_targets(int64_t* p, int64_t n, int C) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    p[i] = (int64_t)(hash_u32((uint32_t)i, 7u) % (uint32_t)C);
}

static bool same_bits(const bf16raw* a, const bf16raw* b, size_t n, bool* ok) {
  const size_t chunk = 1u << 22;
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
  std::vector<int64_t> bs;
  for (int i = 1; i < argc; ++i) bs.push_back(atoll(argv[i]));
  if (bs.empty()) bs.push_back(2097152);
  const int H = 256, C = 10, WARM = 2, REPS = 10;
  int cus = 256;
  CKB(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  for (int64_t B : bs) {
    bf16raw *y, *w, *logits[2], *dlogits, *dz[2];
    float *bias, *dw[2], *db[2], *loss[2];
    int64_t* tgt;
    CKB(hipMalloc(&y, B * H * 2));
    CKB(hipMalloc(&w, C * H * 2));
    CKB(hipMalloc(&bias, C * 4));
    CKB(hipMalloc(&tgt, B * 8));
    CKB(hipMalloc(&dlogits, B * C * 2));
    for (int v = 0; v < 2; ++v) {
      CKB(hipMalloc(&logits[v], B * C * 2));
      CKB(hipMalloc(&dz[v], B * H * 2));
      CKB(hipMalloc(&dw[v], C * H * 4));
      CKB(hipMalloc(&db[v], C * 4));
      CKB(hipMalloc(&loss[v], 4));
    }
    fill_kernel<<<2048, 256>>>(y, B * H, 1u, 1, 1.f);
    fill_kernel<<<16, 256>>>(w, (int64_t)C * H, 2u, 0, 0.0625f);
    fill_targets<<<2048, 256>>>(tgt, B, C);
    CKB(hipMemset(bias, 0, C * 4));
    CKB(hipDeviceSynchronize());
    hipEvent_t e0, e1; CKB(hipEventCreate(&e0)); CKB(hipEventCreate(&e1));
    // stage 0..2: the replaced launches one by one; 3: the fused kernel
    // (with its loss memset); 4: the fused kernel also writing the logits
    const char* names[5] = {"fc3 fwd gemm_kernel", "ce_fused", "head_bwd_kernel",
                            "head_ce_kernel", "head_ce_kernel+logits"};
    float us[5];
    for (int s = 0; s < 5; ++s) {
      for (int it = 0; it < WARM + REPS; ++it) {
        if (it == WARM) CKB(hipEventRecord(e0));
        if (s == 0)
          CKB(launch_gemm_bf16(y, w, 0, nullptr, logits[0], bias, (int)B, C, H, H, 1, 1, H,
                               EPI_BIAS, 1, nullptr, -1, 0));
        else if (s == 1)
          CKB(launch_ce_fused(logits[0], tgt, loss[0], dlogits, (int)B, C, 0));
        else if (s == 2)
          CKB(launch_head_bwd(dlogits, w, y, dz[0], dw[0], db[0], (int)B, C, H, 0, cus, 0));
        else
          CKB(launch_head_ce(w, bias, y, tgt, dz[1], dw[1], db[1], loss[1],
                             s == 4 ? logits[1] : nullptr, (int)B, C, H, 0, cus, 0));
      }
      CKB(hipEventRecord(e1)); CKB(hipEventSynchronize(e1));
      float t; CKB(hipEventElapsedTime(&t, e0, e1));
      us[s] = t * 1000.f / REPS;
    }
    // one clean pass of each route for the comparison
    CKB(hipMemset(loss[0], 0, 4));
    for (int v = 0; v < 2; ++v) { CKB(hipMemset(dw[v], 0, C * H * 4)); CKB(hipMemset(db[v], 0, C * 4)); }
    CKB(launch_gemm_bf16(y, w, 0, nullptr, logits[0], bias, (int)B, C, H, H, 1, 1, H, EPI_BIAS, 1,
                         nullptr, -1, 0));
    CKB(launch_ce_fused(logits[0], tgt, loss[0], dlogits, (int)B, C, 0));
    CKB(launch_head_bwd(dlogits, w, y, dz[0], dw[0], db[0], (int)B, C, H, 0, cus, 0));
    CKB(launch_head_ce(w, bias, y, tgt, dz[1], dw[1], db[1], loss[1], logits[1], (int)B, C, H, 0,
                       cus, 0));
    CKB(hipDeviceSynchronize());
    bool ok = true;
    const bool dz_same = same_bits(dz[0], dz[1], (size_t)B * H, &ok);
    const bool lg_same = same_bits(logits[0], logits[1], (size_t)B * C, &ok);
    if (!ok) { printf("copy failed\n"); return 1; }
    float hl[2], hw[2][C * H], hb[2][C];
    for (int v = 0; v < 2; ++v) {
      CKB(hipMemcpy(&hl[v], loss[v], 4, hipMemcpyDeviceToHost));
      CKB(hipMemcpy(hw[v], dw[v], C * H * 4, hipMemcpyDeviceToHost));
      CKB(hipMemcpy(hb[v], db[v], C * 4, hipMemcpyDeviceToHost));
    }
    float wmax = 0.f, wdiff = 0.f, bmax = 0.f, bdiff = 0.f;
    for (int i = 0; i < C * H; ++i) {
      wmax = fmaxf(wmax, fabsf(hw[0][i]));
      wdiff = fmaxf(wdiff, fabsf(hw[0][i] - hw[1][i]));
    }
    for (int i = 0; i < C; ++i) {
      bmax = fmaxf(bmax, fabsf(hb[0][i]));
      bdiff = fmaxf(bdiff, fabsf(hb[0][i] - hb[1][i]));
    }
    const double needed = (double)B * (2.0 * H * 2 + 8);
    for (int s = 0; s < 5; ++s)
      printf("B=%8ld H=%d C=%d %-22s: %8.1f us\n", (long)B, H, C, names[s], us[s]);
    printf("B=%8ld replaced launches: %8.1f us   fused: %8.1f us  %5.2f TB/s needed\n", (long)B,
           us[0] + us[1] + us[2], us[3], needed / us[3] / 1e6);
    printf("B=%8ld dz_in %s  logits %s  loss %.7g vs %.7g (rel %.1e)  dw rel %.1e  db rel %.1e\n",
           (long)B, dz_same ? "bits==" : "BITS DIFFER", lg_same ? "bits==" : "BITS DIFFER", hl[1],
           hl[0], fabs(hl[1] - hl[0]) / fabs(hl[0]), wdiff / (wmax + 1e-30f),
           bdiff / (bmax + 1e-30f));
    hipFree(y); hipFree(w); hipFree(bias); hipFree(tgt); hipFree(dlogits);
    for (int v = 0; v < 2; ++v) {
      hipFree(logits[v]); hipFree(dz[v]); hipFree(dw[v]); hipFree(db[v]); hipFree(loss[v]);
    }
  }
  return 0;
}
