// The host-side interface of the HIP extension, declared ONCE: the argument structs that cross a
// translation unit (and go on into kernels by value) and one prototype per dtf_* launcher / setter.
// bindings.cpp and every .hip / .cpp that defines or calls one of these include this header before
// their own definitions, so a signature or a struct field changed on one side only no longer
// compiles.  A new launcher is declared here, under the file that defines it.
#pragma once
#include <string>
#include <vector>

#include "common.h"

#define DTF_MAX_TAPS 64

// conv.hip: forward / data-gradient tap table (kernel argument, read with wave-uniform indices)
struct TapTable {
  int n;
  int dh[DTF_MAX_TAPS];
  int dw[DTF_MAX_TAPS];
};

// conv_wgrad.hip: the weight gradient's tap table (a distinct type: the kernels take it by value)
struct TapTableW {
  int n;
  int dh[DTF_MAX_TAPS];
  int dw[DTF_MAX_TAPS];
};

struct ConvGeom {
  int N, H, W, C;        // input
  int P, Q;              // output grid of this launch
  int sh, sw;            // input stride
  int Kout;              // output channels (GEMM N)
  int Kpad;              // filter row stride (T*C rounded up to BK)
  int Ho, Wo;            // output tensor spatial dims
  int osh, osw, oh0, ow0;// output placement
  int acc;               // 1: Y += result (dgrad accumulating onto a residual gradient)
                         // 2: Y = result + acc_src * relu_mask (see acc_add8)
  const bf16_t* acc_src; // acc 2: the residual BN's incoming dy, [N, Ho, Wo, Kout] like Y
  const uint8_t* acc_mask;  // acc 2: that BN's forward ReLU bit mask (1 byte per 8 channels)
  const float* bias;        // fused epilogue (register kernel only): Y = act(conv + bias[k])
  int relu;                 //   tf.layers.conv2d(activation=tf.nn.relu) -- MNIST K3/K5
  int nt;                   // non-temporal output stores (set by dtf_conv_igemm)
  // BN + ReLU on load (halo kernels, forward): X is a BatchNorm INPUT; the kernel normalises its
  // patch in LDS with y = bf16(max(x * lsc[c] + lsh[c], 0)) -- the apply pass's arithmetic -- and
  // writes the rows it owns to ly (the weight gradient's operand), so the apply pass never runs
  const float* lsc;
  const float* lsh;
  bf16_t* ly;
};

// Fused BatchNorm-backward statistics in the DATA-GRADIENT epilogue (conv.hip): when this launch
// produces dy of a training-mode BN's output (the BN sits right before this conv in the forward
// pass), the epilogue also accumulates, per channel, sum(dz) and sum(dz * (x - mean) * invstd) with
// dz = dy * relu_mask(x) -- exactly bn_reduce_kernel<1>'s sums, from the bf16-ROUNDED final dy
// (after a fused residual accumulation) -- into row `row0 + tile` of a [rows][2][Kout] slab the
// BN's finalize combines.  Saves the backward reduce pass its full re-read of dy.
struct BnBwdEpi {
  const bf16_t* x;          // BN input, same [N, Ho, Wo, Kout] layout as Y
  const float* mean;
  const float* invstd;
  const float* fsc;         // forward scale / shift (mask recomputed from x, mkind 2)
  const float* fsh;
  const uint8_t* mask;      // ReLU bit mask (mkind 1)
  float* part;              // null: off
  int mkind;                // 0 no ReLU, 1 bit mask, 2 from x
  int row0;
};

// conv.hip: the jobs of one batched filter-transpose launch
constexpr int kWtMaxJobs = 48;
struct WtJobs {
  const bf16_t* src[kWtMaxJobs];
  bf16_t* dst[kWtMaxJobs];
  int K[kWtMaxJobs], T[kWtMaxJobs], C[kWtMaxJobs];
  int tile_end[kWtMaxJobs];     // exclusive prefix sum of T * ceil(K/64) * ceil(C/64)
  int n;
};

struct WgradGeom {
  int N, H, W, C;   // input X
  int P, Q;         // dY spatial
  int sh, sw;
  int Kout;
  int ldw;          // dW row stride (>= T*C)
  long m_per_split; // reduction pixels per split (multiple of BKM)
  long slab;        // floats per split slab (Kout * ldw)
};

// ---- batchnorm.hip
void dtf_relu_mask_apply(const bf16_t* dy, const uint8_t* mask, bf16_t* out, long n,
                         hipStream_t st);
int dtf_bn_partial_blocks(long M, int C);
void dtf_bn_fwd_stats(const bf16_t* x, long M, int C, float* partial, hipStream_t st);
void dtf_bn_fwd_finalize_g(const float* partial, int G, long M, int C, const float* gamma,
                           const float* beta, float* run_mean, float* run_var, float momentum,
                           float eps, float* mean, float* invstd, float* scale, float* shift,
                           hipStream_t st);
void dtf_bn_fwd_finalize(const float* partial, long M, int C, const float* gamma, const float* beta,
                         float* run_mean, float* run_var, float momentum, float eps, float* mean,
                         float* invstd, float* scale, float* shift, hipStream_t st);
long dtf_bn_workspace_floats_g(int G, int C);
long dtf_bn_workspace_floats(long M, int C);
void dtf_bn_infer_finalize(int C, const float* gamma, const float* beta, const float* run_mean,
                           const float* run_var, float eps, float* mean, float* invstd,
                           float* scale, float* shift, hipStream_t st);
void dtf_bn_apply(const bf16_t* x, const bf16_t* res, bf16_t* y, uint8_t* mask, const float* scale,
                  const float* shift, long M, int C, int relu, hipStream_t st);
void dtf_bn_apply_dual(const bf16_t* x, const bf16_t* xp, bf16_t* y, uint8_t* mask,
                       const float* scale, const float* shift, const float* pscale,
                       const float* pshift, long M, int C, int relu, hipStream_t st);
void dtf_bn_set_nt(int v);
void dtf_bn_set_grid_cap(int v);
void dtf_bn_set_stats_blocks(int v);
void dtf_bn_bwd_reduce(const bf16_t* dy, const bf16_t* y, const uint8_t* mask, const bf16_t* x,
                       const float* mean, const float* invstd, long M, int C, int relu,
                       float* partial, const float* fsc, const float* fsh, hipStream_t st);
void dtf_bn_bwd_finalize_g(const float* partial, int G, long M, int C, const float* gamma,
                           const float* mean, const float* invstd, float* dgamma, float* dbeta,
                           float* coefA, float* coefB, float* coefC, int accumulate,
                           hipStream_t st);
void dtf_bn_bwd_finalize(const float* partial, long M, int C, const float* gamma, const float* mean,
                         const float* invstd, float* dgamma, float* dbeta, float* coefA,
                         float* coefB, float* coefC, int accumulate, hipStream_t st);
void dtf_bn_bwd_apply(const bf16_t* dy, const bf16_t* y, const uint8_t* mask, const bf16_t* x,
                      const float* cA, const float* cB, const float* cC, bf16_t* dx, bf16_t* dres,
                      long M, int C, int relu, const float* fsc, const float* fsh, hipStream_t st);
void dtf_bn_bwd_reduce_dual(const bf16_t* dy, const uint8_t* mask, const bf16_t* x,
                            const float* mean, const float* invstd, const bf16_t* xp,
                            const float* meanp, const float* invstdp, long M, int C, float* partial,
                            float* partialp, hipStream_t st);
void dtf_bn_bwd_apply_dual(const bf16_t* dy, const uint8_t* mask, const bf16_t* x, const float* cA,
                           const float* cB, const float* cC, bf16_t* dx, const bf16_t* xp,
                           const float* cAp, const float* cBp, const float* cCp, bf16_t* dxp,
                           long M, int C, hipStream_t st);

// ---- conv.hip
void dtf_conv_set_small_k(int mode);
void dtf_conv_set_dma_mode(int mode);
void dtf_conv_set_halo(int on);
void dtf_conv_set_halo_strips(int v);
void dtf_conv_set_halo_freg(int v);
void dtf_conv_set_halo_stages(int v);
void dtf_conv_set_bnl_probe(int v);
void dtf_conv_set_stem_halo(int v);
void dtf_conv_set_halo_bnb(int v);
int dtf_conv_stats_rows(long M, int Kout, int C, int taps, int W);
void dtf_conv_set_gemm(int v);
int dtf_conv_tile_rows(const ConvGeom& g, const TapTable& taps, int bnb);
// the short name of the kernel dtf_conv_igemm launches for these arguments ("halo1", "dma",
// "reg32_wide", "gather8_narrow", "gemm", "stem", ...): the dispatcher branches on the same function
std::string dtf_conv_route(const ConvGeom& g, const TapTable& taps, int bk, bool stats,
                           const BnBwdEpi& bnb);
void dtf_conv_set_nt(int v);
bool dtf_conv_bnl_ok(const ConvGeom& g, const TapTable& taps);
void dtf_conv_igemm(const bf16_t* X, const bf16_t* Wt, bf16_t* Y, const ConvGeom& g_in,
                    const TapTable& taps, int bk, float* stats, const BnBwdEpi& bnb,
                    hipStream_t st);
bool dtf_conv_igemm_grouped(const bf16_t* X, bf16_t* Y, const ConvGeom& g0, int ncls,
                            const bf16_t* const* wts, const int* oh0, const int* ow0,
                            const int* kpad, const std::vector<std::vector<int>>& dh,
                            const std::vector<std::vector<int>>& dw, const BnBwdEpi& bnb,
                            const int* row0, hipStream_t st);
void dtf_filter_transpose(const WtJobs& jobs, hipStream_t st);

// ---- conv_wgrad.hip
void dtf_wgrad_set_dma_mode(int mode);
void dtf_wgrad_set_pp(int v);
void dtf_wgrad_set_dense(int v);
void dtf_wgrad_set_deep(int v);
void dtf_wgrad_set_direct(int v);
void dtf_wgrad_set_pipe(int p);
int dtf_wgrad_get_pipe();
void dtf_wgrad_set_halo(int v);
void dtf_wgrad_set_stem(int v);
int dtf_conv_wgrad_halo_splits(int N, int H, int W, int C, int P, int Q, int Kout, int sh, int sw,
                               const TapTableW& taps);
int dtf_conv_wgrad_splits(long M, int Kout, int TC, long ws_cap, int taps);
void dtf_conv_wgrad(const bf16_t* X, const bf16_t* dY, float* dW, float* ws, WgradGeom g,
                    const TapTableW& taps, int splits, int tr_mode, int accumulate, hipStream_t st);
// the short name of the kernel dtf_conv_wgrad launches for these arguments ("halo", "stem", "pp1",
// "dma_narrow_pipe3", "reg", "generic", ...): the dispatcher branches on the same function
std::string dtf_conv_wgrad_route(WgradGeom g, const TapTableW& taps, int splits, int tr_mode);
void dtf_slab_reduce(const float* ws, float* out, long n, int nsplit, int accumulate,
                     hipStream_t st);
int dtf_wgrad_stem_dz_splits(int N);
void dtf_conv_wgrad_stem_dz(const bf16_t* X, const bf16_t* dp, const uint8_t* arg,
                            const bf16_t* xbn, const float* ca, const float* cb, const float* cc,
                            const float* fsc, const float* fsh, float* dW, float* ws, int N,
                            int accumulate, hipStream_t st);

// ---- conv1x1_bwd.hip
bool dtf_conv1x1_bwd_ok(int M, int C, int K);
int dtf_conv1x1_bwd_blocks(int M, int C);
void dtf_conv1x1_bwd_set_grid(int n);
void dtf_conv1x1_bwd_set_w16(int v);
void dtf_conv1x1_bwd(const bf16_t* dout, const bf16_t* wt, const bf16_t* y, const bf16_t* x,
                     const float* mean, const float* inv, const float* sc, const float* sh,
                     bf16_t* dy, float* wpart, float* bpart, int M, int C, int K, hipStream_t st);
bool dtf_conv1x1_bwd_lazy_ok(int M, int C, int K);
int dtf_conv1x1_bwd_lazy_blocks(int M, int C);
void dtf_conv1x1_bwd_lazy(const bf16_t* dy3, const bf16_t* x3, const uint8_t* mask, const float* cA,
                          const float* cB, const float* cC, const bf16_t* wt, const bf16_t* y,
                          const bf16_t* x, const float* mean, const float* inv, const float* sc,
                          const float* sh, bf16_t* dy, float* wpart, float* bpart, int M, int C,
                          int K, const bf16_t* w, hipStream_t st);

// ---- gemm.hip
void dtf_gemm_set_variant(int v);
void dtf_gemm_set_stream(int v);
void dtf_gemm_set_pp2(int v);
void dtf_gemm_set_pp2_strided(int v);
int dtf_gemm_get_pp2();
void dtf_gemm_set_nt(int v);
void dtf_gemm_set_dbg(int v);
void dtf_gemm_set_group(int gm);
int dtf_gemm_conv_part_images(int N, int H, int W, int C, int P, int Q);
void dtf_gemm_conv(const bf16_t* X, const bf16_t* Wt, bf16_t* Y, int N, int H, int W, int C, int P,
                   int Q, int sh, int sw, int Kout, int ntaps, const int* dh, const int* dw, int Ho,
                   int Wo, int osh, int osw, int oh0, int ow0, float* stats, const bf16_t* Cin,
                   const bf16_t* acc_src, const uint8_t* acc_mask, hipStream_t st);
void dtf_gemm_nt_gelu_bwd(const bf16_t* A, const bf16_t* B, bf16_t* C, int M, int N, int K, int lda,
                          int ldb, const bf16_t* gelu_a, const float* gelu_b, float* colsum,
                          hipStream_t st);
void dtf_gemm_nt_bias_gelu(const bf16_t* A, const bf16_t* B, bf16_t* Z, bf16_t* H, int M, int N,
                           int K, int lda, int ldb, const float* bias, hipStream_t st);
bool dtf_gemm_pp2_ok(int M, int N, int K, int lda, int ldb);
int dtf_gemm_tile_rows(int M);
void dtf_gemm_nt(const bf16_t* A, const bf16_t* B, bf16_t* C, int M, int N, int K, int lda, int ldb,
                 int ldc, const float* bias, const bf16_t* Cin, int relu, float* stats,
                 hipStream_t st, const bf16_t* acc_src, const uint8_t* acc_mask);

// ---- gemm_stream.hip
bool dtf_gemm_stream_ok(int M, int N, int K, int lda, int ldb, int ldc);
void dtf_gemm_stream(const bf16_t* A, const bf16_t* B, bf16_t* C, int M, int N, int K, int lda,
                     int ldb, int ldc, const bf16_t* Cin, float* stats, const bf16_t* acc_src,
                     const uint8_t* acc_mask, int nt, hipStream_t st);
void dtf_gemm_stream_bnb(const bf16_t* A, const bf16_t* B, bf16_t* C, int M, int N, int K, int lda,
                         int ldb, int ldc, const bf16_t* Cin, const bf16_t* acc_src,
                         const uint8_t* acc_mask, const bf16_t* bx, const float* bmean,
                         const float* binv, const float* bsc, const float* bsh,
                         const uint8_t* bmask, int kind, float* part, int nt, hipStream_t st,
                         const bf16_t* y2, const bf16_t* w3, int k3);
void dtf_gemm_stream_bnb_dual(const bf16_t* A, const bf16_t* B, bf16_t* C, int M, int N, int K,
                              int lda, int ldb, int ldc, const bf16_t* Cin, const bf16_t* acc_src,
                              const uint8_t* acc_mask, const bf16_t* bx, const float* bmean,
                              const float* binv, const uint8_t* bmask, float* part,
                              const bf16_t* bxp, const float* bmeanp, const float* binvp,
                              float* part_p, hipStream_t st);
void dtf_gemm_stream_pre(const bf16_t* X, const bf16_t* B, bf16_t* C, int M, int N, int K,
                         const float* pre_sc, const float* pre_sh, bf16_t* y, float* stats,
                         hipStream_t st, int nostore);
void dtf_gemm_stream_apply(const bf16_t* A, const bf16_t* W, bf16_t* Y, int M, int N, int K,
                           const bf16_t* res, const float* sc, const float* sh, uint8_t* mask,
                           hipStream_t st);
void dtf_gemm_stream_set_bnb_probe(int v);
void dtf_gemm_stream_probe(const bf16_t* A, const bf16_t* B, bf16_t* C, int M, int N, int probe,
                           hipStream_t st);

// ---- pool.hip
void dtf_maxpool_fwd(const bf16_t* x, bf16_t* y, uint8_t* arg, int N, int H, int W, int C, int P,
                     int Q, int kh, int kw, int sh, int sw, int ph, int pw, hipStream_t st);
void dtf_pool_set_blocked(int v);
void dtf_maxpool_bwd(const bf16_t* dy, const uint8_t* arg, bf16_t* dx, int N, int H, int W, int C,
                     int P, int Q, int kh, int kw, int sh, int sw, int ph, int pw, hipStream_t st);
void dtf_gap_fwd(const bf16_t* x, bf16_t* y, int N, int HW, int C, hipStream_t st);
void dtf_gap_bwd(const bf16_t* dy, bf16_t* dx, int N, int HW, int C, hipStream_t st);
void dtf_s2d_set_rows(int v);
void dtf_s2d_input(const bf16_t* x, bf16_t* xs, int N, int H, int W, int C, int Ho, int Wo, int s,
                   int cp, int pad, hipStream_t st);
void dtf_bn_relu_maxpool_fwd(const bf16_t* x, const float* scale, const float* shift, bf16_t* y,
                             uint8_t* arg, int N, int H, int W, int C, int P, int Q, int kh, int kw,
                             int sh, int sw, int ph, int pw, hipStream_t st);
void dtf_pool_bn_bwd_set_caps(int reduce_cap, int apply_cap);
int dtf_pool_bn_bwd_blocks(int N, int H, int W, int C);
void dtf_pool_bn_bwd_reduce(const bf16_t* dy, const uint8_t* arg, const bf16_t* x,
                            const float* mean, const float* invstd, const float* fsc,
                            const float* fsh, float* partial, int N, int H, int W, int C, int P,
                            int Q, hipStream_t st);
void dtf_pool_bn_bwd_apply(const bf16_t* dy, const uint8_t* arg, const bf16_t* x, const float* cA,
                           const float* cB, const float* cC, const float* fsc, const float* fsh,
                           bf16_t* dx, int N, int H, int W, int C, int P, int Q, hipStream_t st);

// ---- dense.hip
int dtf_bias_relu_bwd_ws_floats(int N);
void dtf_bias_relu_bwd(const bf16_t* dy, const bf16_t* y, bf16_t* dz, int T, int N, float* ws,
                       float* db, int accumulate, int relu, hipStream_t st);
void dtf_gather_u8_scale(const uint8_t* images, const int64_t* idx, void* out, int B, int D,
                         float scale, int out_bf16, hipStream_t st);

// ---- augment.hip
void dtf_augment_images(const uint8_t* images, const int64_t* idx, const int* boxes,
                        const uint8_t* flip, const void* lut, void* out, long N, int B, int Hs,
                        int Ws, int C, int Ho, int Wo, int fill, int out_bf16, int max_blocks,
                        hipStream_t st);
// the same, row b mixed with row partner[b] of the batch (Mixup weight lam_q / 65536, CutMix box
// cut[b] = (oy0, ox0, h, w) in output pixels)
void dtf_augment_mix_images(const uint8_t* images, const int64_t* idx, const int* boxes,
                            const uint8_t* flip, const void* lut, const int* partner,
                            const int* lam_q, const int* cut, void* out, long N, int B, int Hs,
                            int Ws, int C, int Ho, int Wo, int fill, int out_bf16, int max_blocks,
                            hipStream_t st);
// the same with RandAugment: row b's output -> input affine map aff[b] = (a, b, c, d, e, f) in
// Q16 and its L <= 4 pointwise ops (pops[b], ppar[b]); Ho, Wo <= 1024; partner / lam_q / cut all
// null: unmixed
void dtf_augment_rand_images(const uint8_t* images, const int64_t* idx, const int* boxes,
                             const uint8_t* flip, const void* lut, const int* aff,
                             const int* pops, const int* ppar, int L, const int* partner,
                             const int* lam_q, const int* cut, void* out, long N, int B, int Hs,
                             int Ws, int C, int Ho, int Wo, int fill, int ra_fill, int out_bf16,
                             int max_blocks, hipStream_t st);

// ---- mlm_mask.hip
// the masking settings (data.TokenMasking), a kernel argument by value
struct MlmMaskRule {
  uint32_t vocab_size, pad_id, cls_id, sep_id, mask_id;
  uint32_t random_low;      // random replacements are drawn from [random_low, vocab_size)
  uint32_t prob_q16;        // round(prob * 65536)
};
void dtf_mlm_mask_tokens(const void* tokens, int token_bytes, const int64_t* idx,
                         int64_t* input_ids, int64_t* segment_ids, int64_t* input_mask,
                         int64_t* positions, int64_t* ids, float* weights, long N, int B, int S,
                         int P, uint32_t seed, long ex_stride, long ex_offset,
                         const MlmMaskRule& rule, int max_blocks, hipStream_t st);
// the same with whole-word masking: continuation[v] = 1 marks id v of the vocabulary as a
// continuation piece, and a word's pieces are selected together
void dtf_mlm_mask_words(const void* tokens, int token_bytes, const int64_t* idx,
                        const uint8_t* continuation, int64_t* input_ids, int64_t* segment_ids,
                        int64_t* input_mask, int64_t* positions, int64_t* ids, float* weights,
                        long N, int B, int S, int P, uint32_t seed, long ex_stride, long ex_offset,
                        const MlmMaskRule& rule, int max_blocks, hipStream_t st);

// ---- loss.hip
void dtf_softmax_xent(const float* logits, const void* labels, int label_bytes, int B, int V,
                      float* loss_rows, float* grad, float grad_scale, hipStream_t st);
void dtf_softmax_xent_smooth(const float* logits, const void* labels, int label_bytes, int B, int V,
                             float* loss_rows, float* grad, float grad_scale, float smoothing,
                             hipStream_t st);
// two labels per row, weighted lam[b] and 1 - lam[b] (Mixup / CutMix); smoothing = 0 allowed
void dtf_softmax_xent_pair(const float* logits, const void* labels_a, const void* labels_b,
                           int label_bytes, const float* lam, int B, int V, float* loss_rows,
                           float* grad, float grad_scale, float smoothing, hipStream_t st);

// ---- metrics.hip
void dtf_eval_rows(uintptr_t logits, int elem_bytes, const void* labels, int label_bytes, int N,
                   int V, int ld, float* loss_rows, int* rank, hipStream_t st);
void dtf_metrics_accumulate(const float* loss_rows, const int* rank, const float* weights, int N,
                            int k, double* state, hipStream_t st);

// ---- optim.hip
void dtf_sgd_momentum(float* p, const float* g, float* a, bf16_t* shadow, long n,
                      const float* lr_ptr, float momentum, float wd, float gscale, int nesterov,
                      int* nonfinite, const float* gmul, hipStream_t st);
void dtf_adam(float* p, const float* g, float* m, float* v, bf16_t* shadow, long n,
              const float* lr_t_ptr, float b1, float b2, float eps, float wd, float gscale,
              int* nonfinite, const float* gmul, hipStream_t st);
void dtf_adagrad(float* p, const float* g, float* acc, bf16_t* shadow, long n, const float* lr_ptr,
                 float gscale, int* nonfinite, const float* gmul, hipStream_t st);
void dtf_lamb(float* p, float* g, float* m, float* v, bf16_t* shadow, const void* chunks,
              int nchunks, const float* hyper, const float* lr_ptr, float b1, float b2, float eps,
              const float* wd_seg, float gscale, float* norms, float* partial, int* nonfinite,
              const float* gmul, hipStream_t st);
int dtf_lamb_chunk_bytes();
void dtf_lars(float* p, const float* g, float* a, bf16_t* shadow, const void* chunks, int nchunks,
              const void* segs, const float* lr_ptr, float momentum, float wd, float eeta,
              float eps, float gscale, int nesterov, float* partial, int* nonfinite,
              const float* gmul, hipStream_t st);
void dtf_sumsq(const float* x, long n, float* out, hipStream_t st);
// Deterministic global gradient norm.  The partial pass stores one fp64 sum of squares per
// dtf_grad_norm_chunk()-element chunk of g into partial[]; the finish pass adds partial[0..nchunks)
// and extra[0..nextra) (other ranks' sums; may be null) in a fixed order and writes
// GradNormRecord{S, norm = gscale sqrt(S), gmul = gscale clip / max(norm, clip)}.  gmul (when
// non-null above) replaces gscale in the update kernels.  max_blocks: grid cap, 0 = default.
struct GradNormRecord { double S; float norm; float gmul; };
int dtf_grad_norm_chunk();
void dtf_grad_norm_partial(const float* g, long n, double* partial, int max_blocks, hipStream_t st);
void dtf_grad_norm_finish(const double* partial, long nchunks, const double* extra, int nextra,
                          float gscale, float clip, GradNormRecord* rec, hipStream_t st);
void dtf_grad_norm(const float* g, long n, double* partial, int max_blocks, const double* extra,
                   int nextra, float gscale, float clip, GradNormRecord* rec, hipStream_t st);
void dtf_cast_f32_bf16(const float* x, bf16_t* y, long n, hipStream_t st);
// tf.train.ExponentialMovingAverage: avg[i] -= a * (avg[i] - var[i]) over [0, n), a = *a_ptr on the
// device.  avg / var may start at any element offset.  max_blocks: grid cap, 0 = default.
void dtf_ema_update(float* avg, const float* var, long n, const float* a_ptr, int max_blocks,
                    hipStream_t st);
// Gradient accumulation over micro-batches: mode 0 dst[i] = src[i], mode 1 dst[i] = dst[i] + src[i]
// over [0, n), one fp32 add per element.  dst / src may start at any element offset and must not
// overlap.  max_blocks: grid cap, 0 = default.
void dtf_grad_accumulate(float* dst, const float* src, long n, int mode, int max_blocks,
                         hipStream_t st);

// ---- nlp.hip
int dtf_bf16_col_sum_ws_floats(int N);
void dtf_bf16_col_sum(const bf16_t* x, int T, int N, float* ws, float* out, int accumulate,
                      hipStream_t st);
void dtf_ln_set_wide(int v);
void dtf_ln_fwd(const bf16_t* a, const float* bias, const bf16_t* res, const float* gamma,
                const float* beta, bf16_t* y, bf16_t* s, float* mean, float* rstd, int M, int H,
                float eps, float p_pre, uint32_t seed_pre, float p_post, uint32_t seed_post,
                const int64_t* ids, const int64_t* tt, const bf16_t* word, const bf16_t* pos,
                const bf16_t* type, int S, hipStream_t st);
int dtf_ln_bwd_blocks(int M);
void dtf_ln_bwd(const bf16_t* dy, const bf16_t* s, const float* mean, const float* rstd,
                const float* gamma, bf16_t* ds, bf16_t* da, float* part, float* dgamma,
                float* dbeta, float* dbias, int M, int H, float p_pre, uint32_t seed_pre,
                float p_post, uint32_t seed_post, hipStream_t st, int accumulate);
void dtf_bias_gelu_fwd(const bf16_t* a, const float* bias, bf16_t* y, long M, int N,
                       hipStream_t st);
int dtf_bias_gelu_bwd_blocks(int M);
void dtf_bias_gelu_bwd(const bf16_t* dy, const bf16_t* a, const float* bias, bf16_t* da,
                       float* part, float* dbias, int M, int N, hipStream_t st, int accumulate);
void dtf_attn_set_wide(int v);
void dtf_attn_set_keep(int v);
long dtf_attn_keep_words(int B, int S, int H, float p);
void dtf_attn_fwd(const bf16_t* qkv, const float* mask, bf16_t* out, float* lse, int B, int S,
                  int H, float scale, float p, uint32_t seed, hipStream_t st, uint32_t* keep,
                  int causal);
void dtf_attn_set_fused(int v);
int dtf_attn_bwd_fused(int S);
void dtf_attn_bwd(const bf16_t* qkv, const float* mask, const bf16_t* out, const bf16_t* dout,
                  const float* lse, float* delta, bf16_t* dqkv, int B, int S, int H, float scale,
                  float p, uint32_t seed, hipStream_t st, float* colpart, const uint32_t* keep,
                  int causal);
int dtf_pos_type_grad_ws_floats(int S, int H, int NT);
void dtf_pos_type_grad(const bf16_t* ds, const int64_t* tt, int B, int S, int H, int NT,
                       float* dpos, float* dtyp, float* ws, hipStream_t st);
void dtf_segment_sum(const int64_t* sorted_ids, const int64_t* perm, const bf16_t* src, float* out,
                     int T, int H, hipStream_t st);
void dtf_mlm_xent(const bf16_t* logits, const int64_t* labels, const float* weights,
                  const float* denom, int N, int V, int ld, float* loss_rows, bf16_t* grad,
                  hipStream_t st);

// ---- f32.hip
int dtf_gemm_f32_splits(int M, int N, int K);
void dtf_gemm_f32(const float* A, const float* B, float* C, const float* bias, int M, int N, int K,
                  long sam, long sak, long sbn, long sbk, long scm, long scn, float alpha, int relu,
                  int accumulate, float* ws, hipStream_t st);
void dtf_im2col_f32(const float* x, float* cols, int N, int H, int W, int C, int P, int Q, int sh,
                    int sw, int R, int S, int pt, int pl, hipStream_t st);
void dtf_col2im_f32(const float* dcols, float* dx, int N, int H, int W, int C, int P, int Q, int sh,
                    int sw, int R, int S, int pt, int pl, hipStream_t st);
void dtf_maxpool_f32_fwd(const float* x, float* y, uint8_t* arg, int N, int H, int W, int C, int P,
                         int Q, int k, int s, hipStream_t st);
void dtf_maxpool_f32_bwd(const float* dy, const uint8_t* arg, float* dx, int N, int H, int W, int C,
                         int P, int Q, int k, int s, hipStream_t st);
int dtf_bias_relu_bwd_f32_ws_floats(int N);
void dtf_bias_relu_bwd_f32(const float* dy, const float* y, float* dz, int T, int N, float* ws,
                           float* db, int accumulate, int relu, hipStream_t st);
void dtf_clipped_xent(const float* z, const float* t, int B, int V, float* row_loss, float* dz,
                      float scale, hipStream_t st);

// ---- probe.hip
void dtf_lds_probe(int bytes, int blocks, int* errors, int spin, hipStream_t st);
int dtf_max_dynamic_lds(int dev);

// ---- ipc.cpp
uintptr_t dtf_ipc_alloc(size_t bytes, int device);
std::string dtf_ipc_handle(uintptr_t ptr, int device);
uintptr_t dtf_ipc_open(const std::string& handle, int device);
void dtf_ipc_close(uintptr_t ptr, int device);
void dtf_ipc_free(uintptr_t ptr, int device);

// ---- rccl_comm.cpp
int dtf_rccl_load(const std::string& path);
std::string dtf_rccl_unique_id();
long dtf_rccl_comm_init(const std::string& uid, int nranks, int rank, int device);
void dtf_rccl_comm_destroy(long comm, int abort);
int dtf_rccl_async_error(long comm);
void dtf_rccl_all_reduce(long comm, long send, long recv, long count, int dtype, int op,
                         long stream);
void dtf_rccl_reduce_scatter(long comm, long send, long recv, long recvcount, int dtype, int op,
                             long stream);
void dtf_rccl_all_gather(long comm, long send, long recv, long sendcount, int dtype, long stream);
void dtf_rccl_broadcast(long comm, long send, long recv, long count, int dtype, int root,
                        long stream);
void dtf_rccl_reduce(long comm, long send, long recv, long count, int dtype, int op, int root,
                     long stream);
void dtf_rccl_group(int start);
