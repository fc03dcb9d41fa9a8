// Microbench: one-launch MLP inference (mlp_predict.hip) against the per-layer
// launches it replaces on the same buffers: linear_stream.hip where linear_fwd
// routes a layer there (N in (128, 256], M >= its row threshold), else
// gemm.hip's tiles.
// hipcc --offload-arch=gfx950 -O3 -ffast-math tools/mlp_predict_bench.hip -o tools/mlp_predict_bench
// usage: mlp_predict_bench [--dims K0,w1[,w2..],C] [M ...]   (default 784,256,256,10 at 2097152)
// Prints us per launch (fused; the per-layer launches and their sum), TB/s of
// NEEDED bytes (x once + 4 B of class id a row), and whether the logits are
// bit-identical and the class ids the argmax of the per-layer logits.
#include "../sparktorch_amd/ops/csrc/gemm.hip"
#include "../sparktorch_amd/ops/csrc/linear_stream.hip"
#include "../sparktorch_amd/ops/csrc/mlp_predict.hip"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CKB(x) do { hipError_t e=(x); if(e!=hipSuccess){printf("err %s %d\n",hipGetErrorString(e),__LINE__);return 1;} } while(0)

__global__ void fill_kernel(bf16raw* p, int64_t n, uint32_t seed, float scale) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = (uint32_t)i * 2654435761u ^ (uint32_t)(i >> 32) * 40503u ^ seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    p[i] = f32_to_bf16(((int)(h & 255) - 128) / 128.f * scale);
  }
}

__global__ void fill_f32_kernel(float* p, int n, uint32_t seed) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    uint32_t h = (uint32_t)i * 2654435761u ^ seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    p[i] = ((int)(h & 255) - 128) / 512.f;
  }
}

static float bf16_host(bf16raw h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

int main(int argc, char** argv) {
  std::vector<int64_t> ms;
  std::vector<int> dims = {784, 256, 256, 10};
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--dims") && i + 1 < argc) {
      dims.clear();
      for (char* tok = strtok(argv[++i], ","); tok; tok = strtok(nullptr, ",")) dims.push_back(atoi(tok));
    } else {
      ms.push_back(atoll(argv[i]));
    }
  }
  if (ms.empty()) ms.push_back(2097152);
  const int NL = (int)dims.size() - 1;  // layers, the head included
  if (NL < 2 || NL > MP_MAX_HIDDEN + 1) { printf("need K0, 1-4 hidden widths and C\n"); return 1; }
  const int L = NL - 1, K0 = dims[0], C = dims[NL];
  int num_cus = 0;
  CKB(hipDeviceGetAttribute(&num_cus, hipDeviceAttributeMultiprocessorCount, 0));
  const int WARM = 2, REPS = 10;
  for (int64_t M : ms) {
    if (!mlp_predict_supported(K0, &dims[1], L, C, M)) { printf("unsupported chain\n"); return 1; }
    bf16raw *x, *w[MP_MAX_HIDDEN + 1], *act[MP_MAX_HIDDEN + 1], *logits;
    float* b[MP_MAX_HIDDEN + 1];
    int* classes;
    CKB(hipMalloc(&x, M * K0 * 2));
    fill_kernel<<<2048, 256>>>(x, M * K0, 1u, 1.f);
    for (int l = 0; l < NL; ++l) {
      const int K = dims[l], N = dims[l + 1];
      CKB(hipMalloc(&w[l], (size_t)K * N * 2));
      CKB(hipMalloc(&b[l], ((N * 4 + 15) / 16) * 16));
      CKB(hipMalloc(&act[l], M * N * 2));
      fill_kernel<<<64, 256>>>(w[l], (int64_t)K * N, 2u + l, 2.f / sqrtf((float)K));
      fill_f32_kernel<<<1, 256>>>(b[l], N, 9u + l);
    }
    CKB(hipMalloc(&logits, M * C * 2));
    CKB(hipMalloc(&classes, M * 4));
    CKB(hipDeviceSynchronize());
    hipEvent_t e0, e1; CKB(hipEventCreate(&e0)); CKB(hipEventCreate(&e1));

    // v = 0: fused with logits, 1: fused, class ids only, 2 + l: layer l alone
    std::vector<float> us(2 + NL);
    for (int v = 0; v < 2 + NL; ++v) {
      for (int it = 0; it < WARM + REPS; ++it) {
        if (it == WARM) CKB(hipEventRecord(e0));
        if (v < 2) {
          CKB(launch_mlp_predict(x, w, b, &dims[1], L, K0, C, M, classes, v == 0 ? logits : nullptr,
                                 0, num_cus, 0));
        } else {
          const int l = v - 2, K = dims[l], N = dims[l + 1];
          const bf16raw* in = l == 0 ? x : act[l - 1];
          const int epi = l < L ? EPI_BIAS_RELU : EPI_BIAS;
          if (linear_fwd_stream_supported(N, K, M) && M >= LS_MIN_ROWS)
            CKB(launch_linear_stream(in, w[l], act[l], b[l], nullptr, M, N, K, epi, 0, 0, 0));
          else
            CKB(launch_gemm_bf16(in, w[l], 0, nullptr, act[l], b[l], (int)M, N, K, K, 1, 1, K, epi, 1,
                                 nullptr, -1, 0));
        }
      }
      CKB(hipEventRecord(e1)); CKB(hipEventSynchronize(e1));
      float t; CKB(hipEventElapsedTime(&t, e0, e1));
      us[v] = t * 1000.f / REPS;
    }

    // logits bit for bit, class ids against the host argmax of the per-layer
    // logits (lowest index on ties), on a prefix and a suffix of the rows
    const int64_t rows = M < (1 << 18) ? M : (1 << 18);
    std::vector<bf16raw> h0(rows * C), h1(rows * C);
    std::vector<int> hc(rows);
    bool same = true, ids_ok = true;
    for (int part = 0; part < 2; ++part) {
      const int64_t r0 = part ? M - rows : 0;
      CKB(hipMemcpy(h0.data(), act[L] + r0 * C, rows * C * 2, hipMemcpyDeviceToHost));
      CKB(hipMemcpy(h1.data(), logits + r0 * C, rows * C * 2, hipMemcpyDeviceToHost));
      CKB(hipMemcpy(hc.data(), classes + r0, rows * 4, hipMemcpyDeviceToHost));
      if (memcmp(h0.data(), h1.data(), rows * C * 2) != 0) same = false;
      for (int64_t r = 0; r < rows; ++r) {
        int best = 0;
        for (int c = 1; c < C; ++c)
          if (bf16_host(h0[r * C + c]) > bf16_host(h0[r * C + best])) best = c;
        if (hc[r] != best) ids_ok = false;
      }
    }
    float sum = 0.f;
    for (int l = 0; l < NL; ++l) sum += us[2 + l];
    const double bytes = (double)M * (K0 * 2 + 4);
    printf("M=%8ld fused+logits %8.1f us | fused ids %8.1f us  %5.2f TB/s needed | per-layer", (long)M,
           us[0], us[1], bytes / us[1] / 1e6);
    for (int l = 0; l < NL; ++l) printf(" %s%.1f", l ? "+ " : "", us[2 + l]);
    printf(" = %8.1f us  %s %s\n", sum, same ? "bits==per-layer" : "BITS DIFFER",
           ids_ok ? "ids==argmax" : "IDS DIFFER");
    (void)hipFree(x); (void)hipFree(logits); (void)hipFree(classes);
    for (int l = 0; l < NL; ++l) { (void)hipFree(w[l]); (void)hipFree(b[l]); (void)hipFree(act[l]); }
  }
  return 0;
}
