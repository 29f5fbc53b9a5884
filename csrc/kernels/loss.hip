// Fused sparse softmax cross-entropy forward+backward.
// TF semantics (run_mnist_distributed.py:113): loss = mean_b(-log softmax(logits_b)[label_b]);
// the gradient (softmax - onehot) / B is produced in the same pass (one wave per row; the
// row max / sum use 64-lane shuffles) and cached for the backward.
//
// Label smoothing (tf.losses.softmax_cross_entropy(label_smoothing=e), the same definition as
// torch's): the target row is (1-e) onehot + e/V, so
//   loss_b   = lse - (1-e) x[label] - (e/V) sum_i x_i
//   grad_b,i = (p_i - (1-e) [i = label] - e/V) / B
// It is the SMOOTH instantiation of the same kernel (sum_i x_i rides the first sweep); e = 0
// launches the plain instantiation, whose code and results are unchanged.
//
// Two labels per row (Mixup / CutMix): the target row is lam onehot(a) + (1 - lam) onehot(b),
// smoothed as above, so with mu = 1 - lam
//   loss_b   = lse - (1-e) (lam x[a] + mu x[b]) - (e/V) sum_i x_i
//   grad_b,i = (p_i - (1-e) (lam [i = a] + mu [i = b]) - e/V) / B
// (a = b puts both terms on one class).  It is the PAIR instantiation, still one wave per row and
// one read of the logits; the other two are what they were.
#include "launch.h"

namespace {
template <typename LT, bool SMOOTH, bool PAIR = false>
__global__ void __launch_bounds__(256)
xent_kernel(const float* __restrict__ logits, const LT* __restrict__ labels, int B, int V,
            float* __restrict__ loss_rows, float* __restrict__ grad, float grad_scale,
            float smoothing, const LT* __restrict__ labels_b = nullptr,
            const float* __restrict__ lam = nullptr) {
  const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= B) return;
  const float* row = logits + (long)wave * V;
  float mx = -INFINITY, sx = 0.f;
  for (int i = lane; i < V; i += 64) {
    mx = fmaxf(mx, row[i]);
    if (SMOOTH) sx += row[i];
  }
  mx = wave_max(mx);
  if (SMOOTH) sx = wave_sum(sx);
  float s = 0.f;
  for (int i = lane; i < V; i += 64) s += __expf(row[i] - mx);
  s = wave_sum(s);
  const float lse = mx + __logf(s);
  const int lab = (int)labels[wave];
  const float on = SMOOTH ? 1.f - smoothing : 1.f;     // weight of the true class
  const float off = SMOOTH ? smoothing / V : 0.f;      // weight spread over every class
  int lab_b = lab;
  float la = 1.f, mu = 0.f;                            // weights of the two labels
  if (PAIR) {
    lab_b = (int)labels_b[wave];
    la = lam[wave];
    mu = 1.f - la;
    if (lane == 0) loss_rows[wave] = lse - on * (la * row[lab] + mu * row[lab_b]) - off * sx;
  } else if (lane == 0) {
    loss_rows[wave] = SMOOTH ? lse - on * row[lab] - off * sx : lse - row[lab];
  }
  if (grad) {
    const float inv = 1.f / s;
    float* g = grad + (long)wave * V;
    for (int i = lane; i < V; i += 64) {
      float p = __expf(row[i] - mx) * inv;
      if (PAIR)
        g[i] = (p - on * ((i == lab ? la : 0.f) + (i == lab_b ? mu : 0.f)) - off) * grad_scale;
      else if (SMOOTH)
        g[i] = (p - (i == lab ? on : 0.f) - off) * grad_scale;
      else
        g[i] = (p - (i == lab ? 1.f : 0.f)) * grad_scale;
    }
  }
}

template <bool SMOOTH>
void launch_xent(const float* logits, const void* labels, int label_bytes, int B, int V,
                 float* loss_rows, float* grad, float grad_scale, float smoothing,
                 hipStream_t st) {
  const int blocks = (B * 64 + 255) / 256;
  if (label_bytes == 8)
    hipLaunchKernelGGL((xent_kernel<int64_t, SMOOTH>), dim3(blocks), dim3(256), 0, st, logits,
                       (const int64_t*)labels, B, V, loss_rows, grad, grad_scale, smoothing);
  else
    hipLaunchKernelGGL((xent_kernel<int32_t, SMOOTH>), dim3(blocks), dim3(256), 0, st, logits,
                       (const int32_t*)labels, B, V, loss_rows, grad, grad_scale, smoothing);
}

void launch_xent_pair(const float* logits, const void* labels_a, const void* labels_b,
                      int label_bytes, const float* lam, int B, int V, float* loss_rows,
                      float* grad, float grad_scale, float smoothing, hipStream_t st) {
  const int blocks = (B * 64 + 255) / 256;
  if (label_bytes == 8)
    hipLaunchKernelGGL((xent_kernel<int64_t, true, true>), dim3(blocks), dim3(256), 0, st, logits,
                       (const int64_t*)labels_a, B, V, loss_rows, grad, grad_scale, smoothing,
                       (const int64_t*)labels_b, lam);
  else
    hipLaunchKernelGGL((xent_kernel<int32_t, true, true>), dim3(blocks), dim3(256), 0, st, logits,
                       (const int32_t*)labels_a, B, V, loss_rows, grad, grad_scale, smoothing,
                       (const int32_t*)labels_b, lam);
}
}  // namespace

void dtf_softmax_xent(const float* logits, const void* labels, int label_bytes, int B, int V,
                      float* loss_rows, float* grad, float grad_scale, hipStream_t st) {
  launch_xent<false>(logits, labels, label_bytes, B, V, loss_rows, grad, grad_scale, 0.f, st);
}

void dtf_softmax_xent_smooth(const float* logits, const void* labels, int label_bytes, int B,
                             int V, float* loss_rows, float* grad, float grad_scale,
                             float smoothing, hipStream_t st) {
  launch_xent<true>(logits, labels, label_bytes, B, V, loss_rows, grad, grad_scale, smoothing,
                    st);
}

void dtf_softmax_xent_pair(const float* logits, const void* labels_a, const void* labels_b,
                           int label_bytes, const float* lam, int B, int V, float* loss_rows,
                           float* grad, float grad_scale, float smoothing, hipStream_t st) {
  if (B <= 0) return;
  launch_xent_pair(logits, labels_a, labels_b, label_bytes, lam, B, V, loss_rows, grad,
                   grad_scale, smoothing, st);
}
