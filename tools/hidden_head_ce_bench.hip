// Microbench: the last hidden layer's forward fused into the head's loss pass
// (hidden_head_ce.hip) against the two launches it replaces: the hidden
// layer's forward (linear_stream_kernel, EPI_BIAS_RELU) and head_ce_kernel.
// (Below linear_fwd_stream_min_rows() the library's linear_fwd takes
// gemm_kernel instead; this tool times linear_stream_kernel at every B.)
// hipcc --offload-arch=gfx950 -O3 -ffast-math tools/hidden_head_ce_bench.hip -o tools/hidden_head_ce_bench
// usage: hidden_head_ce_bench [--k=K_in] [--h=H] [B ...]
//        (default B = 2097152, K_in = 256, H = 256; C = 10)
// Both routes run on the same buffers, 10 timed launches after 2 warm-up.
// Prints us per launch, TB/s of NEEDED bytes (x once + dz2 once + targets),
// whether dz2, h2 and the logits are bit-identical, and the loss / dw3 / db3
// differences (fp32 atomics: equal to rounding only).
#include "../sparktorch_amd/ops/csrc/linear_stream.hip"
#include "../sparktorch_amd/ops/csrc/head_bwd.hip"
#include "../sparktorch_amd/ops/csrc/hidden_head_ce.hip"
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

__global__ void fill_f32(float* p, int n, uint32_t seed, float scale) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    p[i] = ((int)(hash_u32((uint32_t)i, seed) & 255) - 128) / 128.f * scale;
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
  int K = 256, H = 256;
  for (int i = 1; i < argc; ++i) {
    if (!strncmp(argv[i], "--k=", 4)) K = atoi(argv[i] + 4);
    else if (!strncmp(argv[i], "--h=", 4)) H = atoi(argv[i] + 4);
    else bs.push_back(atoll(argv[i]));
  }
  if (bs.empty()) bs.push_back(2097152);
  const int C = 10, WARM = 2, REPS = 10;
  if (!hidden_head_ce_supported(K, H, C)) { printf("unsupported (K_in, H)\n"); return 1; }
  int cus = 256;
  CKB(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  for (int64_t B : bs) {
    if (!linear_fwd_stream_supported(H, K, B)) { printf("unsupported B\n"); return 1; }
    bf16raw *x, *w2, *w3, *h2[2], *logits[2], *dz[2];
    float *b2, *b3, *dw[2], *db[2], *loss[2];
    int64_t* tgt;
    CKB(hipMalloc(&x, B * K * 2));
    CKB(hipMalloc(&w2, H * K * 2));
    CKB(hipMalloc(&w3, C * H * 2));
    CKB(hipMalloc(&b2, H * 4));
    CKB(hipMalloc(&b3, C * 4));
    CKB(hipMalloc(&tgt, B * 8));
    for (int v = 0; v < 2; ++v) {
      CKB(hipMalloc(&h2[v], B * H * 2));
      CKB(hipMalloc(&logits[v], B * C * 2));
      CKB(hipMalloc(&dz[v], B * H * 2));
      CKB(hipMalloc(&dw[v], C * H * 4));
      CKB(hipMalloc(&db[v], C * 4));
      CKB(hipMalloc(&loss[v], 4));
    }
    fill_kernel<<<2048, 256>>>(x, B * K, 1u, 1, 1.f);
    fill_kernel<<<64, 256>>>(w2, (int64_t)H * K, 3u, 0, 0.0625f);
    fill_kernel<<<16, 256>>>(w3, (int64_t)C * H, 2u, 0, 0.0625f);
    fill_f32<<<1, 256>>>(b2, H, 5u, 0.5f);
    fill_f32<<<1, 64>>>(b3, C, 6u, 0.5f);
    fill_targets<<<2048, 256>>>(tgt, B, C);
    CKB(hipDeviceSynchronize());
    hipEvent_t e0, e1; CKB(hipEventCreate(&e0)); CKB(hipEventCreate(&e1));
    // stage 0, 1: the replaced launches one by one; 2: the fused kernel (with
    // its loss-zeroing launch); 3: the fused kernel also writing h2 and logits
    const char* names[4] = {"hidden fwd linear_stream", "head_ce_kernel", "hidden_head_ce_kernel",
                            "hidden_head_ce+h2+logits"};
    float us[4];
    for (int s = 0; s < 4; ++s) {
      for (int it = 0; it < WARM + REPS; ++it) {
        if (it == WARM) CKB(hipEventRecord(e0));
        if (s == 0)
          CKB(launch_linear_stream(x, w2, h2[0], b2, nullptr, B, H, K, EPI_BIAS_RELU, 0, 0,
                                   LS_PATH_TILE128, 0));
        else if (s == 1)
          CKB(launch_head_ce(w3, b3, h2[0], tgt, dz[0], dw[0], db[0], loss[0], nullptr, (int)B, C,
                             H, 0, cus, 0));
        else
          CKB(launch_hidden_head_ce(x, w2, b2, w3, b3, tgt, dz[1], dw[1], db[1], loss[1],
                                    s == 3 ? logits[1] : nullptr, s == 3 ? h2[1] : nullptr,
                                    (int)B, K, H, C, 0, cus, 0));
      }
      CKB(hipEventRecord(e1)); CKB(hipEventSynchronize(e1));
      float t; CKB(hipEventElapsedTime(&t, e0, e1));
      us[s] = t * 1000.f / REPS;
    }
    // one clean pass of each route for the comparison
    for (int v = 0; v < 2; ++v) { CKB(hipMemset(dw[v], 0, C * H * 4)); CKB(hipMemset(db[v], 0, C * 4)); }
    CKB(launch_linear_stream(x, w2, h2[0], b2, nullptr, B, H, K, EPI_BIAS_RELU, 0, 0,
                             LS_PATH_TILE128, 0));
    CKB(launch_head_ce(w3, b3, h2[0], tgt, dz[0], dw[0], db[0], loss[0], logits[0], (int)B, C, H,
                       0, cus, 0));
    CKB(launch_hidden_head_ce(x, w2, b2, w3, b3, tgt, dz[1], dw[1], db[1], loss[1], logits[1],
                              h2[1], (int)B, K, H, C, 0, cus, 0));
    CKB(hipDeviceSynchronize());
    bool ok = true;
    const bool dz_same = same_bits(dz[0], dz[1], (size_t)B * H, &ok);
    const bool h2_same = same_bits(h2[0], h2[1], (size_t)B * H, &ok);
    const bool lg_same = same_bits(logits[0], logits[1], (size_t)B * C, &ok);
    if (!ok) { printf("copy failed\n"); return 1; }
    float hl[2];
    std::vector<float> hw[2], hb[2];
    for (int v = 0; v < 2; ++v) {
      hw[v].resize(C * H); hb[v].resize(C);
      CKB(hipMemcpy(&hl[v], loss[v], 4, hipMemcpyDeviceToHost));
      CKB(hipMemcpy(hw[v].data(), dw[v], C * H * 4, hipMemcpyDeviceToHost));
      CKB(hipMemcpy(hb[v].data(), db[v], C * 4, hipMemcpyDeviceToHost));
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
    const double needed = (double)B * ((K + H) * 2.0 + 8);
    for (int s = 0; s < 4; ++s)
      printf("B=%8ld K=%d H=%d C=%d %-26s: %8.1f us\n", (long)B, K, H, C, names[s], us[s]);
    printf("B=%8ld replaced launches: %8.1f us   fused: %8.1f us  %5.2f TB/s needed\n", (long)B,
           us[0] + us[1], us[2], needed / us[2] / 1e6);
    printf("B=%8ld dz2 %s  h2 %s  logits %s  loss %.7g vs %.7g (rel %.1e)  dw rel %.1e  db rel %.1e\n",
           (long)B, dz_same ? "bits==" : "BITS DIFFER", h2_same ? "bits==" : "BITS DIFFER",
           lg_same ? "bits==" : "BITS DIFFER", hl[1], hl[0], fabs(hl[1] - hl[0]) / fabs(hl[0]),
           wdiff / (wmax + 1e-30f), bdiff / (bmax + 1e-30f));
    hipFree(x); hipFree(w2); hipFree(w3); hipFree(b2); hipFree(b3); hipFree(tgt);
    for (int v = 0; v < 2; ++v) {
      hipFree(h2[v]); hipFree(logits[v]); hipFree(dz[v]); hipFree(dw[v]); hipFree(db[v]);
      hipFree(loss[v]);
    }
  }
  return 0;
}
