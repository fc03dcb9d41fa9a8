// The host-visible interface of the gfx950 kernels: every function a csrc
// .hip file defines with C linkage, the bf16 carrier type and the codes that
// cross the interface.  Host-safe (no device code, no vector types): g++
// compiles it for bindings.cpp, hipcc for every .hip, and since each .hip
// includes it the compiler holds each definition to its declaration here — a
// reordered or widened argument is "conflicting types", not a wrong answer.
//
// A new kernel file declares its launchers and predicates here and includes
// this header; nothing else declares them.
//
// Launchers take raw pointers and a stream, enqueue, and return the launch
// error.  num_cus is the device's compute-unit count (it sizes persistent
// grids); max_blocks > 0 caps a grid, 0 = the launcher's own choice.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

// bf16 carried as raw uint16 bits; conversions are explicit bit ops so we do
// not depend on hip_bf16 operator overloads inside hot loops.
typedef uint16_t bf16raw;

// Epilogue codes of gemm_kernel and linear_stream_kernel
#define EPI_F32 0        // fp32 store (atomicAdd when SPLITK)
#define EPI_BF16 1       // bf16 store
#define EPI_BIAS 2       // bf16 store, + bias[n]
#define EPI_BIAS_RELU 3  // bf16 store, + bias[n], relu
#define EPI_RELU 4       // bf16 store, relu (no bias)
#define EPI_F32_SLAB 5   // fp32 per-slice slab store (split-K without atomics;
                         // a separate reduce kernel combines the slabs —
                         // guide §5 "splitk-seam": slab reducer beats an
                         // fp32-atomicAdd accumulator)
#define EPI_BF16_MASK 6  // bf16 store, zeroed where mask[m][n] <= 0 (mask: bf16
                         // [M][N], same layout as C) — dgrad with the upstream
                         // ReLU backward folded in

// launch_linear_stream's fwd_path
#define LS_PATH_AUTO 0     // by the measured row threshold
#define LS_PATH_TILE128 1  // linear_stream_kernel
#define LS_PATH_DEEP 2     // linear_stream_deep_kernel

extern "C" {

// ---- elementwise.hip ----

hipError_t launch_increment_i32(int* x, hipStream_t stream);

// step_dev: device step counter for the bias corrections, or null to use
// bc1 / bc2 as given.
hipError_t launch_fused_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                             float b1, float b2, float eps, float wd, float bc1, float bc2,
                             float gscale, int adamw, const int* step_dev, hipStream_t stream);

hipError_t launch_fused_sgd(float* p, const float* g, float* buf, int64_t n, float lr,
                            float momentum, float wd, float dampening, float gscale, int nesterov,
                            int first, int has_momentum, hipStream_t stream);

hipError_t launch_relu_bwd(const bf16raw* dy, const bf16raw* y, bf16raw* dz, int64_t n,
                           hipStream_t stream);

// db is accumulated into.  scratch: S * N floats for the small-N path, or
// null (S = 0) for the atomic one.
hipError_t launch_bias_grad(const bf16raw* dz, float* db, int M, int N, float* scratch, int S,
                            hipStream_t stream);

// dw is accumulated into; scratch holds S * CO * K floats.
hipError_t launch_small_wgrad(const bf16raw* dz, const bf16raw* col, float* dw, float* scratch,
                              int S, int64_t M, int CO, int K, hipStream_t stream);

hipError_t launch_cast_f64_f32(const double* src, float* dst, int64_t n, hipStream_t stream);
hipError_t launch_cast_f64_bf16(const double* src, bf16raw* dst, int64_t n, hipStream_t stream);
hipError_t launch_cast_f32_bf16(const float* src, bf16raw* dst, int64_t n, hipStream_t stream);

// ---- loss.hip ----

// loss_out is accumulated into: the caller zeroes it.
hipError_t launch_ce_fused(const bf16raw* logits, const int64_t* tgt, float* loss_out,
                           bf16raw* dlogits, int B, int C, hipStream_t stream);
hipError_t launch_mse_fused(const bf16raw* pred, const bf16raw* target, float* loss_out,
                            bf16raw* dpred, int64_t n, hipStream_t stream);

// ---- gemm.hip ----

// C[M,N] = A B over K with element strides (sam, sak) and (sbk, sbn); A is
// bf16, B bf16 or fp32 (b_is_f32).  epi: EPI_*; Cf receives the fp32 forms, Cb
// the bf16 ones.  splitk > 1 atomically adds into a zeroed Cf, splitk < 0
// always adds (|splitk| slices).  ones_row >= 0: that column of the extended B
// is a virtual ones column whose output lands in Db (the fused bias grad);
// -1 = none.
hipError_t launch_gemm_bf16(const void* A, const void* B, int b_is_f32, float* Cf, bf16raw* Cb,
                            const float* bias, int M, int N, int K, int64_t sam, int64_t sak,
                            int64_t sbk, int64_t sbn, int epi, int splitk, float* Db, int ones_row,
                            hipStream_t stream);

// mask is read only by EPI_BF16_MASK (bf16 [M][N], same layout as Cb).
hipError_t launch_gemm_bf16_mask(const void* A, const void* B, int b_is_f32, float* Cf,
                                 bf16raw* Cb, const float* bias, int M, int N, int K, int64_t sam,
                                 int64_t sak, int64_t sbk, int64_t sbn, int epi, int splitk,
                                 float* Db, int ones_row, const bf16raw* mask, hipStream_t stream);

// Number of K slices the slab path will use for (K, splitk): callers size the
// workspace as that many M * N floats.  (tools/wgrad_ab.hip only.)
int wgrad_slab_slices(int K, int splitk);

// Split-K wgrad without atomics: per-slice slab stores into ws + one reduce
// launch that writes dw.  transpose != 0: the caller swapped operands to
// compute dW^T; ones_row must be -1 with it.  (tools/wgrad_ab.hip only.)
hipError_t launch_wgrad_slab(const void* A, const void* B, int b_is_f32, float* dw, float* db,
                             int M, int N, int K, int64_t sam, int64_t sak, int64_t sbk,
                             int64_t sbn, int splitk, int ones_row, float* ws, int transpose,
                             hipStream_t stream);

// ---- linear_stream.hip ----

// 1 when the kernel can compute C[M,N] = A[M,K] B for this shape
int linear_fwd_stream_supported(int N, int K, int64_t M);
// 1 when the deep-K forward serves this shape
int linear_fwd_stream_deep_supported(int N, int K, int64_t M);
// Measured rows from which the bindings route a supported shape here, and
// from which a K > 256 forward takes the deep-K kernel.
int64_t linear_fwd_stream_min_rows();
int64_t linear_fwd_stream_deep_min_rows();

// epi: EPI_BF16 / BIAS / BIAS_RELU / RELU for the forward (b_kn = 0,
// B = W[N][K]); EPI_BF16 / EPI_BF16_MASK for the dgrad (b_kn = 1, B = W[K][N]).
// bias and mask may be null where epi does not read them.  bk: k-slab depth of
// linear_stream_kernel, 32 or 64, 0 = the measured default.  fwd_path:
// LS_PATH_*; the dgrad has one.  All pointers 16-byte aligned.
hipError_t launch_linear_stream(const bf16raw* A, const bf16raw* B, bf16raw* C, const float* bias,
                                const bf16raw* mask, int64_t M, int N, int K, int epi, int b_kn,
                                int bk, int fwd_path, hipStream_t stream);

// ---- head_bwd.hip ----

// 1 when (C, H) is served by the fused kernels
int head_bwd_supported(int C, int H);

// dz_in = (dz_out @ w) * (y_in > 0) is written; dw / db are accumulated into
// (the caller zeroes), db may be null.  max_blocks > 0 caps the grid.
hipError_t launch_head_bwd(const bf16raw* dz_out, const bf16raw* w, const bf16raw* y_in,
                           bf16raw* dz_in, float* dw, float* db, int B, int C, int H,
                           int max_blocks, int num_cus, hipStream_t stream);

// Same shape range and grid rule.  loss is defined, not accumulated: it is
// zeroed on the stream first.  bias, db and logits_out may be null.
hipError_t launch_head_ce(const bf16raw* w, const float* bias, const bf16raw* y_in,
                          const int64_t* tgt, bf16raw* dz_in, float* dw, float* db, float* loss,
                          bf16raw* logits_out, int B, int C, int H, int max_blocks, int num_cus,
                          hipStream_t stream);

// The same against a bf16 [B, C] target; bias, db and pred_out may be null.
hipError_t launch_head_mse(const bf16raw* w, const float* bias, const bf16raw* y_in,
                           const bf16raw* target, bf16raw* dz_in, float* dw, float* db,
                           float* loss, bf16raw* pred_out, int B, int C, int H, int max_blocks,
                           int num_cus, hipStream_t stream);

// ---- hidden_head_ce.hip ----

// 1 when a hidden layer K_in -> H under a head of C classes is served
int hidden_head_ce_supported(int K_in, int H, int C);
// rows from which functional._mlp_chain_step takes the kernel (measured)
int64_t hidden_head_ce_min_rows();

// loss is defined (zeroed on the stream first); dw / db are accumulated into.
// b2, b3, db, logits_out and h2_out may be null.  max_blocks > 0 caps the
// grid.  x, w2, w3, dz_in and h2_out 16-byte aligned.
hipError_t launch_hidden_head_ce(const bf16raw* x, const bf16raw* w2, const float* b2,
                                 const bf16raw* w3, const float* b3, const int64_t* tgt,
                                 bf16raw* dz_in, float* dw, float* db, float* loss,
                                 bf16raw* logits_out, bf16raw* h2_out, int B, int K_in, int H,
                                 int C, int max_blocks, int num_cus, hipStream_t stream);

// ---- linear_mse.hip ----

// 1 when the kernel serves an H -> N layer
int linear_mse_supported(int N, int H);
// rows from which functional.linear_mse takes the kernel (measured)
int64_t linear_mse_min_rows();
// columns of one W chunk at width H: a row's last chunk is narrower when N is
// no multiple of it
int linear_mse_chunk_cols(int H);

// h [B,H], w [N,H], target / dpred / pred [B,N] bf16, 16-byte aligned; bias
// fp32 [N] or null; pred null unless wanted.  loss is defined (zeroed on the
// stream first).  max_blocks > 0 caps the grid.
hipError_t launch_linear_mse(const bf16raw* h, const bf16raw* w, const float* bias,
                             const bf16raw* target, bf16raw* dpred, bf16raw* pred, float* loss,
                             int B, int N, int H, int max_blocks, int num_cus,
                             hipStream_t stream);

// ---- mlp_predict.hip ----

// 1 when the kernel serves x[M,K0] -> widths[0..L-1] -> C classes
int mlp_predict_supported(int K0, const int* widths, int L, int C, int64_t M);
// rows from which MnistMLPFused.forward takes the kernel (measured)
int64_t mlp_predict_min_rows();

// w / b: L hidden layers then the head (b entries may be null); logits may be
// null.  max_blocks > 0 caps the persistent grid.  All pointers 16-byte
// aligned.
hipError_t launch_mlp_predict(const bf16raw* x, const bf16raw* const* w, const float* const* b,
                              const int* widths, int L, int K0, int C, int64_t M, int* classes,
                              bf16raw* logits, int max_blocks, int num_cus, hipStream_t stream);
// the same from fp32 rows x[M][K0], rounded to bf16 as torch's cast rounds them
hipError_t launch_mlp_predict_f32(const float* x, const bf16raw* const* w, const float* const* b,
                                  const int* widths, int L, int K0, int C, int64_t M, int* classes,
                                  bf16raw* logits, int max_blocks, int num_cus,
                                  hipStream_t stream);

// ---- linear_wgrad.hip, linear_wgrad_wide.hip, hidden_bwd.hip ----
// One contract: dw [No][Ki] and db [No] (or null) are accumulated into, the
// caller zeroes.  *_can_run: 1 when the kernel can compute (No, Ki, B) at
// all; *_supported: 1 when the router sends (No, Ki, B) there (shape set and
// measured batch threshold).  The launchers serve any B >= 1 that *_can_run
// accepts.  max_blocks > 0 caps the blocks per column tile, i.e. the row
// groups.  dz, x (and dzin) 16-byte aligned.

int linear_wgrad_stream_can_run(int No, int Ki, int64_t B);
int linear_wgrad_stream_supported(int No, int Ki, int64_t B);
hipError_t launch_linear_wgrad_stream(const bf16raw* dz, const bf16raw* x, float* dw, float* db,
                                      int64_t B, int No, int Ki, int max_blocks, int num_cus,
                                      hipStream_t stream);

// layers linear_wgrad.hip cannot hold (No > 256) on a 64/128/256-wide input
int linear_wgrad_wide_can_run(int No, int Ki, int64_t B);
int linear_wgrad_wide_supported(int No, int Ki, int64_t B);
hipError_t launch_linear_wgrad_wide(const bf16raw* dz, const bf16raw* x, float* dw, float* db,
                                    int64_t B, int No, int Ki, int max_blocks, int num_cus,
                                    hipStream_t stream);

// w is the bf16 weight [No][Ki]; dzin receives (dz @ w) * (x > 0), [B][Ki].
int hidden_bwd_can_run(int No, int Ki, int64_t B);
int hidden_bwd_supported(int No, int Ki, int64_t B);
hipError_t launch_hidden_bwd(const bf16raw* dz, const bf16raw* x, const bf16raw* w, bf16raw* dzin,
                             float* dw, float* db, int64_t B, int No, int Ki, int max_blocks,
                             int num_cus, hipStream_t stream);

// ---- sample_gather.hip ----

// half the bit width of the Feistel domain: the smallest h >= 1 with 4^h >= n
int sample_gather_half_bits(int64_t n);

// xb[j] = x[idx[j]], yb[j] = y[idx[j]] for minibatch *step_dev under seed.
// x_es: element size of x (2 or 4); y_es: of y (4 or 8); y / yb and idx_out
// may be null.  Does not advance step_dev.
hipError_t launch_sample_gather(const void* x, int x_es, const void* y, int y_es, void* xb,
                                void* yb, int* idx_out, const int* step_dev, uint32_t seed,
                                int64_t n, int k, int F, int L, int num_cus, hipStream_t stream);

// ---- conv_implicit.hip ----

hipError_t launch_pad_nhwc(const bf16raw* x, bf16raw* xP, int B, int H, int W, int CI, int P,
                           hipStream_t stream);
hipError_t launch_s2d_stem(const bf16raw* x, bf16raw* out, int B, int H, int W, int P,
                           hipStream_t stream);
hipError_t launch_flip_w2d(const bf16raw* w2d, bf16raw* wf, int CO, int CI, int KHW,
                           hipStream_t stream);

// xP is the ring-padded input; wmat [N][Kpad], K padded to x64; bias may be
// null.  (OHo, OWo) <= the GEMM's output dims: the compact output written.
hipError_t launch_conv_implicit_fwd(const bf16raw* xP, const bf16raw* wmat, const float* bias,
                                    bf16raw* y, int B, int Hp, int Wp, int CI, int KH, int KW,
                                    int SH, int SW, int N, int Kpad, int relu, int OHo, int OWo,
                                    hipStream_t stream);

// ws null: atomic combine into a zeroed dw.  ws given: it holds
// conv_implicit_wgrad_slices(B * OH * OW, splitk) slabs of CO * KH*KW*CI
// floats and the reduce writes dw.
hipError_t launch_conv_implicit_wgrad(const bf16raw* dz, const bf16raw* xP, float* dw, int CO,
                                      int B, int Hp, int Wp, int CI, int KH, int KW, int SH,
                                      int SW, int splitk, float* ws, int OHo, int OWo,
                                      hipStream_t stream);
int conv_implicit_wgrad_slices(int K, int splitk);

// ---- conv.hip (NCHW) ----

hipError_t launch_im2col(const bf16raw* x, bf16raw* col, int B, int CI, int H, int W, int KH,
                         int KW, int HO, int WO, int sh, int sw, int ph, int pw,
                         hipStream_t stream);
hipError_t launch_col2im(const bf16raw* dcol, bf16raw* dx, int B, int CI, int H, int W, int KH,
                         int KW, int HO, int WO, int sh, int sw, int ph, int pw,
                         hipStream_t stream);
// kernel == stride; arg: the window slot of each maximum
hipError_t launch_maxpool_fwd(const bf16raw* x, bf16raw* y, uint8_t* arg, int BC, int H, int W,
                              int KS, int HO, int WO, hipStream_t stream);
hipError_t launch_maxpool_bwd(const bf16raw* dy, const uint8_t* arg, bf16raw* dx, int BC, int H,
                              int W, int KS, int HO, int WO, hipStream_t stream);
hipError_t launch_dropout(const bf16raw* in, bf16raw* out, int64_t n, int64_t units_div,
                          int64_t cmod, float p, uint32_t seed, hipStream_t stream);

// ---- conv_nhwc.hip ----

// Kp: the col matrix's row stride (K padded to x8); im2col zeroes the pad
hipError_t launch_im2col_nhwc(const bf16raw* x, bf16raw* col, int B, int CI, int H, int W, int KH,
                              int KW, int HO, int WO, int sh, int sw, int ph, int pw, int Kp,
                              hipStream_t stream);
hipError_t launch_col2im_nhwc(const bf16raw* dcol, bf16raw* dx, int B, int CI, int H, int W,
                              int KH, int KW, int HO, int WO, int sh, int sw, int ph, int pw,
                              int Kp, hipStream_t stream);
hipError_t launch_maxpool_nhwc_fwd(const bf16raw* x, bf16raw* y, uint8_t* arg, int B, int C, int H,
                                   int W, int HO, int WO, int KS, int S, int P,
                                   hipStream_t stream);
hipError_t launch_maxpool_nhwc_bwd(const bf16raw* dy, const uint8_t* arg, bf16raw* dx, int B,
                                   int C, int H, int W, int HO, int WO, int KS, int S, int P,
                                   hipStream_t stream);
hipError_t launch_gap_nhwc_fwd(const bf16raw* x, bf16raw* y, int B, int C, int64_t HW,
                               hipStream_t stream);
hipError_t launch_gap_nhwc_bwd(const bf16raw* dy, bf16raw* dx, int B, int C, int64_t HW,
                               hipStream_t stream);

// ---- norm.hip ----

// sum / sumsq are zeroed by the caller; running_mean / running_var may be
// null (both or neither).
hipError_t launch_bn_stats(const bf16raw* x, float* sum, float* sumsq, float* mean, float* invstd,
                           float* running_mean, float* running_var, int B, int C, int64_t HW,
                           float momentum, float eps, int nsplit, hipStream_t stream);
// res may be null
hipError_t launch_bn_apply(const bf16raw* x, const bf16raw* res, bf16raw* y, const float* mean,
                           const float* invstd, const float* gamma, const float* beta, int C,
                           int64_t HW, int64_t total, int do_relu, hipStream_t stream);
// dbeta / dgamma are accumulated into; yrelu (the ReLU output, for its mask)
// may be null
hipError_t launch_bn_bwd_reduce(const bf16raw* dy, const bf16raw* yrelu, const bf16raw* x,
                                const float* mean, const float* invstd, float* dbeta,
                                float* dgamma, int B, int C, int64_t HW, int nsplit,
                                hipStream_t stream);
hipError_t launch_bn_bwd_dx(const bf16raw* dy, const bf16raw* yrelu, const bf16raw* x,
                            const float* mean, const float* invstd, const float* gamma,
                            const float* dbeta, const float* dgamma, bf16raw* dx, int C,
                            int64_t HW, int64_t total, float inv_count, int train_stats,
                            hipStream_t stream);

// The NHWC forms over M = B*H*W rows.  scratch: 2 * S * C floats for the
// vector reduction path, or null (S = 0) for the atomic one.
hipError_t launch_bn_stats_nhwc(const bf16raw* x, float* sum, float* sumsq, float* mean,
                                float* invstd, float* running_mean, float* running_var, int64_t M,
                                int C, float momentum, float eps, int nsplit, float* scratch,
                                int S, hipStream_t stream);
hipError_t launch_bn_apply_nhwc(const bf16raw* x, const bf16raw* res, bf16raw* y,
                                const float* mean, const float* invstd, const float* gamma,
                                const float* beta, int C, int64_t total, int do_relu,
                                hipStream_t stream);
hipError_t launch_bn_bwd_reduce_nhwc(const bf16raw* dy, const bf16raw* yrelu, const bf16raw* x,
                                     const float* mean, const float* invstd, const float* gamma,
                                     const float* beta, float* dbeta, float* dgamma, int64_t M,
                                     int C, int nsplit, float* scratch, int S,
                                     hipStream_t stream);
hipError_t launch_bn_bwd_dx_nhwc(const bf16raw* dy, const bf16raw* yrelu, const bf16raw* x,
                                 const float* mean, const float* invstd, const float* gamma,
                                 const float* beta, const float* dbeta, const float* dgamma,
                                 bf16raw* dx, int C, int64_t total, float inv_count,
                                 int train_stats, hipStream_t stream);

hipError_t launch_add_relu(const bf16raw* a, const bf16raw* b, bf16raw* out, int64_t n,
                           hipStream_t stream);
// arg: the window slot of each maximum (KS <= 15)
hipError_t launch_maxpool_gen_fwd(const bf16raw* x, bf16raw* y, uint8_t* arg, int64_t BC, int H,
                                  int W, int HO, int WO, int KS, int S, int P, hipStream_t stream);
hipError_t launch_maxpool_gen_bwd(const bf16raw* dy, const uint8_t* arg, bf16raw* dx, int64_t BC,
                                  int H, int W, int HO, int WO, int KS, int S, int P,
                                  hipStream_t stream);
hipError_t launch_gap_fwd(const bf16raw* x, bf16raw* y, int64_t BC, int64_t HW,
                          hipStream_t stream);
hipError_t launch_gap_bwd(const bf16raw* dy, bf16raw* dx, int64_t HW, int64_t total,
                          hipStream_t stream);

}  // extern "C"
