// Evaluation metrics: per-row loss + rank of the label in ONE sweep of the logits, and a
// deterministic accumulation of a batch into a device-resident fp64 state.
//
// eval_rows (one wave per row, like xent_kernel / mlm_xent_kernel):
//   loss_rows[i] = lse_i - x[label_i]                       (unsmoothed: evaluation loss is)
//   rank[i]      = #{j : x_j > x_label} + #{j < label : x_j == x_label}
// the stable descending rank of the label: the label is in the top k iff rank < k, fully defined
// under ties (bf16 logits over 30k classes tie constantly); for k = 1 it is torch.argmax's rule
// (the first maximal index wins).  Stricter than TF's in_top_k, which counts strictly greater
// logits only and so lets every member of a tie at the k boundary in.
//   * x[label] is read first, then the row is read exactly once: an online (max, sum) with one
//     rescale per 16-B chunk (taken only when the chunk raises the lane's maximum) and the two
//     counters.  No gradient, no second pass.
//   * rows are `ld` elements apart (ld >= V); columns V .. ld-1 are not classes: they are left
//     out of the softmax and of the rank whatever they hold (the tied BERT decoder emits
//     ld = 30528 for V = 30522).
//   * rows need no alignment (bf16 V = ld = 30522, fp32 V = ld = 1003, a view at an odd offset):
//     like mlm_xent_kernel the row is swept in 16-B chunks from the 16-B-aligned address below
//     its start with range-checked raw buffer loads, elements outside the row masked.  The
//     buffer starts at the 16-B-aligned address at or below the tensor (inside its allocation)
//     and ends at the last class of the last row: nothing outside it is ever touched.
//   * a label outside [0, V) marks an ignored row: rank = -1, loss = 0 (weight 0 downstream).
//   * a NaN label logit is a miss: rank = V.
//
// metrics_accumulate (ONE 256-thread block): state[0..3] += [sum w, sum w loss, sum w [rank<1],
// sum w [rank<k]] over the batch, w = the optional fp32 row weight (1 without), 0 for ignored
// rows; rows of weight 0 are dropped whatever their loss holds.  Fixed order -- thread t adds
// rows t, t+256, ... in fp64, a fixed LDS tree, thread 0 adds to the state -- and no atomics:
// two runs give a bit-identical state, and with 0/1 weights the hit counts are exact integers.
#include "launch.h"

#include <stdexcept>
#include <string>

namespace {

template <typename T> struct Elem;
template <> struct Elem<bf16_t> {
  static constexpr int kPer = 8;       // elements per 16-B chunk
  static DTF_DEV void unpack(const uint4& v, float* f) { unpack8(v, f); }
  static DTF_DEV float one(const bf16_t* p) { return bf2f(*p); }
};
template <> struct Elem<float> {
  static constexpr int kPer = 4;
  static DTF_DEV void unpack(const uint4& v, float* f) {
    f[0] = __builtin_bit_cast(float, v.x);
    f[1] = __builtin_bit_cast(float, v.y);
    f[2] = __builtin_bit_cast(float, v.z);
    f[3] = __builtin_bit_cast(float, v.w);
  }
  static DTF_DEV float one(const float* p) { return *p; }
};

DTF_DEV int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One 16-B chunk whose first element is class `e0` (negative / past V at a row's two ends) into the
// lane's online (max, sum) and its two counters.  EDGE: some element may lie outside [0, V) and
// is masked; interior chunks skip the per-element range checks.
template <typename T, bool EDGE>
DTF_DEV void sweep_chunk(const uint4& raw, int e0, int V, int lab, float xl, float& mx, float& s,
                         int& gt, int& eq) {
  constexpr int P = Elem<T>::kPer;
  float f[P];
  Elem<T>::unpack(raw, f);
  const int lim = lab - e0;                      // elements k < lim lie before the label
  float mc = -INFINITY;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    if (EDGE) {
      const int j = e0 + k;
      const bool in = j >= 0 && j < V;
      gt += (in && f[k] > xl) ? 1 : 0;
      eq += (in && k < lim && f[k] == xl) ? 1 : 0;
      if (!in) f[k] = -INFINITY;
    } else {
      gt += f[k] > xl ? 1 : 0;
      eq += (k < lim && f[k] == xl) ? 1 : 0;
    }
    mc = fmaxf(mc, f[k]);
  }
  const float nm = fmaxf(mx, mc);
  if (nm == -INFINITY) return;                   // nothing finite yet: exp(-inf - -inf) is NaN
  if (nm != mx) {                                // rare after the first chunks: full-precision exp
    s *= expf(mx - nm);                          // mx = -inf: s = 0 stays 0
    mx = nm;
  }
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < P; ++k) acc += __expf(f[k] - nm);     // exp(-inf) = 0 for masked slots
  s += acc;
}

// `base` = the 16-B-aligned address at or below the tensor, `off0` = the tensor's first element
// counted from it (0 .. kPer-1), `bytes` = the buffer's extent from `base`.
template <typename T, typename LT>
__global__ void __launch_bounds__(256)
eval_rows_kernel(const T* __restrict__ base, int off0, uint32_t bytes,
                 const LT* __restrict__ labels, int N, int V, int ld,
                 float* __restrict__ loss_rows, int* __restrict__ rank) {
  constexpr int P = Elem<T>::kPer;
  constexpr uint32_t ES = sizeof(T);
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= N) return;
  const LT lab_raw = labels[row];
  if (lab_raw < 0 || lab_raw >= (LT)V) {          // ignored row (wave-uniform)
    if (lane == 0) {
      loss_rows[row] = 0.f;
      rank[row] = -1;
    }
    return;
  }
  const int lab = (int)lab_raw;
  const float xl = Elem<T>::one(base + off0 + (long)row * ld + lab);
  const auto rl = buffer_rsrc(base, bytes);
  const uint32_t b0 = ((uint32_t)off0 + (uint32_t)row * (uint32_t)ld) * ES;
  const uint32_t a0 = b0 & ~15u;
  const int head = (int)((b0 - a0) / ES);
  const int nch = (head + V + P - 1) / P;
  float mx = -INFINITY, s = 0.f;
  int gt = 0, eq = 0;
  // two chunks per trip: both loads are issued before either is consumed.  A chunk at or past
  // `nch` holds no class (every element masked); past the buffer it reads zeros.
  for (int c = lane; c < nch; c += 128) {
    uint4 raw[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
      raw[u] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                             rl, a0 + (uint32_t)(c + u * 64) * 16u, 0, 0));
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e0 = (c + u * 64) * P - head;
      if (e0 >= 0 && e0 + P <= V)
        sweep_chunk<T, false>(raw[u], e0, V, lab, xl, mx, s, gt, eq);
      else
        sweep_chunk<T, true>(raw[u], e0, V, lab, xl, mx, s, gt, eq);
    }
  }
  // combine the lanes: the row maximum is exact, every lane rescales its sum ONCE (full-precision
  // exp), and the 64 partial sums and the final lse - x[label] are formed in fp64 -- one fp32
  // rounding of the loss in all
  const float M = wave_max(mx);
  double ds = mx == -INFINITY ? 0.0 : (double)s * (double)expf(mx - M);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ds += __shfl_xor(ds, o, 64);
  gt = wave_sum_i(gt);
  eq = wave_sum_i(eq);
  if (lane == 0) {
    loss_rows[row] = (float)(((double)M - (double)xl) + log(ds));
    rank[row] = xl != xl ? V : gt + eq;
  }
}

__global__ void __launch_bounds__(256)
metrics_accumulate_kernel(const float* __restrict__ loss_rows, const int* __restrict__ rank,
                          const float* __restrict__ weights, int N, int k,
                          double* __restrict__ state) {
  __shared__ double sm[4][256];
  const int t = threadIdx.x;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = t; i < N; i += 256) {
    const int r = rank[i];
    const double w = r < 0 ? 0.0 : (weights ? (double)weights[i] : 1.0);
    if (w == 0.0) continue;
    a[0] += w;
    a[1] += w * (double)loss_rows[i];
    a[2] += r < 1 ? w : 0.0;
    a[3] += r < k ? w : 0.0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) sm[j][t] = a[j];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) {
#pragma unroll
      for (int j = 0; j < 4; ++j) sm[j][t] += sm[j][t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) state[j] += sm[j][0];
  }
}

template <typename T>
void launch_eval_rows(uintptr_t logits, const void* labels, int label_bytes, int N, int V, int ld,
                      float* loss_rows, int* rank, hipStream_t st) {
  const uintptr_t mis = logits & 15u;
  if (mis % sizeof(T)) throw std::runtime_error("eval_rows: logits not aligned to their element");
  const double extent = (double)mis + ((double)(N - 1) * ld + V) * sizeof(T);
  if (extent >= 2147483647.0) throw std::runtime_error("eval_rows: logits too large");
  const T* base = reinterpret_cast<const T*>(logits - mis);
  const int off0 = (int)(mis / sizeof(T));
  // whole dwords: the range check is per dword, and the aligned dword that holds the last class
  // lies inside the tensor's allocation
  const uint32_t bytes = ((uint32_t)extent + 3u) & ~3u;
  const dim3 grid((unsigned)(((long)N + 3) / 4)), block(256);
  if (label_bytes == 8)
    hipLaunchKernelGGL((eval_rows_kernel<T, int64_t>), grid, block, 0, st, base, off0,
                       bytes, (const int64_t*)labels, N, V, ld, loss_rows, rank);
  else
    hipLaunchKernelGGL((eval_rows_kernel<T, int32_t>), grid, block, 0, st, base, off0,
                       bytes, (const int32_t*)labels, N, V, ld, loss_rows, rank);
}

}  // namespace

// elem_bytes: 2 = bf16, 4 = fp32; label_bytes: 4 = int32, 8 = int64
void dtf_eval_rows(uintptr_t logits, int elem_bytes, const void* labels, int label_bytes, int N,
                   int V, int ld, float* loss_rows, int* rank, hipStream_t st) {
  if (N < 0) throw std::runtime_error("eval_rows: negative row count");
  if (V < 1 || ld < V) throw std::runtime_error("eval_rows: row stride below the class count");
  if (label_bytes != 4 && label_bytes != 8)
    throw std::runtime_error("eval_rows: labels must be int32 or int64");
  if (N == 0) return;
  if (elem_bytes == 2)
    launch_eval_rows<bf16_t>(logits, labels, label_bytes, N, V, ld, loss_rows, rank, st);
  else if (elem_bytes == 4)
    launch_eval_rows<float>(logits, labels, label_bytes, N, V, ld, loss_rows, rank, st);
  else
    throw std::runtime_error("eval_rows: logits must be bf16 or fp32");
}

void dtf_metrics_accumulate(const float* loss_rows, const int* rank, const float* weights, int N,
                            int k, double* state, hipStream_t st) {
  if (N < 0) throw std::runtime_error("metrics_accumulate: negative row count");
  if (k < 1) throw std::runtime_error("metrics_accumulate: k must be at least 1");
  if (N == 0) return;
  hipLaunchKernelGGL(metrics_accumulate_kernel, dim3(1), dim3(256), 0, st, loss_rows, rank,
                     weights, N, k, state);
}
