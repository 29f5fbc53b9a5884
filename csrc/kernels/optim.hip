// Fused optimizer updates over FLAT fp32 buffers (all parameters of a strategy live in one
// contiguous master buffer, so one launch updates the whole model — no multi-tensor lists).
//
// TF-exact update math:
//   Momentum (tf.train.MomentumOptimizer):  a = mu*a + g;  p -= lr*a   (nesterov: p -= lr*(g + mu*a))
//   Adam     (tf.train.AdamOptimizer):      lr_t = lr*sqrt(1-b2^t)/(1-b1^t)
//                                           m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2
//                                           p -= lr_t * m / (sqrt(v) + eps)   <- eps OUTSIDE the
//                                           bias correction, unlike torch.optim.Adam
//   Adagrad  (tf.train.AdagradOptimizer):   acc += g^2; p -= lr * g * rsqrt(acc)   (acc0 = 0.1)
//   LAMB     (per-tensor trust ratio):      u = m_hat/(sqrt(v_hat)+eps) + wd*p;
//                                           p -= lr * (|p|/|u|) * u
//   LARS     (tf.contrib.opt.LARSOptimizer): decayed tensors: g2 = g + wd*p,
//                                           s = lr * eeta*|p| / (|g| + wd*|p| + eps);
//                                           others: g2 = g, s = lr;
//                                           a = mu*a + s*g2;  p -= a
//                                           (nesterov: p -= s*g2 + mu*a)
//            Its norms and LAMB's are slab-reduced in a fixed order (bitwise reproducible).
// Every kernel optionally writes the bf16 compute shadow of p in the same pass (saves the
// separate cast of the fp32 master every step) and flags non-finite gradients.
// Hyper-parameters that change per step (lr, lr_t) are read from DEVICE memory so a captured
// hipGraph replays correctly.
// Global-norm clip (tf.clip_by_global_norm, then the optimizer): every update kernel multiplies g
// by `gscale`, or -- when `gmul` is non-null -- by the multiplier the grad_norm pass below left on
// the device, in the same single fp32 multiply.
#include "launch.h"

namespace {
constexpr int kT = 256;

DTF_DEV void flag_nonfinite(int* flag, float g) {
  if (flag && !isfinite(g)) atomicOr(flag, 1);
}

__global__ void __launch_bounds__(kT)
sgd_momentum_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ a,
                    bf16_t* __restrict__ shadow, long n, const float* __restrict__ lr_ptr,
                    float momentum, float wd, float gscale_v, const float* __restrict__ gmul,
                    int nesterov, int* nonfinite) {
  const float lr = *lr_ptr;
  const float gscale = gmul ? *gmul : gscale_v;
  const long n4 = n >> 2;
  for (long i = (long)blockIdx.x * kT + threadIdx.x; i < n4; i += (long)gridDim.x * kT) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 av = reinterpret_cast<float4*>(a)[i];
    float pp[4] = {pv.x, pv.y, pv.z, pv.w};
    const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
    float aa[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      flag_nonfinite(nonfinite, gg[j]);
      const float gr = gg[j] * gscale + wd * pp[j];
      aa[j] = momentum * aa[j] + gr;
      pp[j] -= lr * (nesterov ? gr + momentum * aa[j] : aa[j]);
    }
    reinterpret_cast<float4*>(p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
    reinterpret_cast<float4*>(a)[i] = make_float4(aa[0], aa[1], aa[2], aa[3]);
    if (shadow) {
      uint2 s;
      s.x = pack2(pp[0], pp[1]);
      s.y = pack2(pp[2], pp[3]);
      reinterpret_cast<uint2*>(shadow)[i] = s;
    }
  }
  // scalar tail
  for (long i = n4 * 4 + (long)blockIdx.x * kT + threadIdx.x; i < n; i += (long)gridDim.x * kT) {
    flag_nonfinite(nonfinite, g[i]);
    const float gr = g[i] * gscale + wd * p[i];
    a[i] = momentum * a[i] + gr;
    p[i] -= lr * (nesterov ? gr + momentum * a[i] : a[i]);
    if (shadow) shadow[i] = f2bf(p[i]);
  }
}

__global__ void __launch_bounds__(kT)
adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
            float* __restrict__ v, bf16_t* __restrict__ shadow, long n,
            const float* __restrict__ lr_t_ptr, float b1, float b2, float eps, float wd,
            float gscale_v, const float* __restrict__ gmul, int* nonfinite) {
  const float lr_t = *lr_t_ptr;
  const float gscale = gmul ? *gmul : gscale_v;
  for (long i = (long)blockIdx.x * kT + threadIdx.x; i < n; i += (long)gridDim.x * kT) {
    const float gr0 = g[i];
    flag_nonfinite(nonfinite, gr0);
    const float gr = gr0 * gscale;
    const float mi = b1 * m[i] + (1.f - b1) * gr;
    const float vi = b2 * v[i] + (1.f - b2) * gr * gr;
    m[i] = mi;
    v[i] = vi;
    float pi = p[i];
    pi -= lr_t * mi / (sqrtf(vi) + eps) + (wd != 0.f ? lr_t * wd * pi : 0.f);
    p[i] = pi;
    if (shadow) shadow[i] = f2bf(pi);
  }
}

__global__ void __launch_bounds__(kT)
adagrad_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ acc,
               bf16_t* __restrict__ shadow, long n, const float* __restrict__ lr_ptr,
               float gscale_v, const float* __restrict__ gmul, int* nonfinite) {
  const float lr = *lr_ptr;
  const float gscale = gmul ? *gmul : gscale_v;
  for (long i = (long)blockIdx.x * kT + threadIdx.x; i < n; i += (long)gridDim.x * kT) {
    const float gr0 = g[i];
    flag_nonfinite(nonfinite, gr0);
    const float gr = gr0 * gscale;
    const float ai = acc[i] + gr * gr;
    acc[i] = ai;
    const float pi = p[i] - lr * gr * rsqrtf(ai);
    p[i] = pi;
    if (shadow) shadow[i] = f2bf(pi);
  }
}

// ---- LAMB: chunk table entries {segment, start, len}; norms[seg] = {sum p^2, sum u^2}.
// Phase 1 stores one partial {sum p^2, sum u^2} per chunk into a slab (plain stores); the norm
// pass gives each tensor -- a run of rows with one segment in the table -- to the block of its
// first row, which adds the rows in one fixed order; phase 2 reads the finished norms.  No float
// atomics: the trust ratio and with it the whole update are bitwise reproducible.
struct Chunk { int seg; int len; long start; };

__global__ void __launch_bounds__(kT)
lamb_phase1_kernel(const float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                   float* __restrict__ v, const Chunk* __restrict__ chunks,
                   const float* __restrict__ hyper, float b1, float b2, float eps,
                   const float* __restrict__ wd_seg, float gscale_v,
                   const float* __restrict__ gmul, float2* __restrict__ partial, int* nonfinite) {
  // hyper[0] = 1/(1-b1^t), hyper[1] = 1/(1-b2^t)
  __shared__ float red[2][kT / 64];
  const float gscale = gmul ? *gmul : gscale_v;
  const Chunk c = chunks[blockIdx.x];
  const float bc1 = hyper[0], bc2 = hyper[1];
  const float wd = wd_seg[c.seg];
  float sp = 0.f, su = 0.f;
  for (int j = threadIdx.x; j < c.len; j += kT) {
    const long i = c.start + j;
    const float gr0 = g[i];
    flag_nonfinite(nonfinite, gr0);
    const float gr = gr0 * gscale;
    const float mi = b1 * m[i] + (1.f - b1) * gr;
    const float vi = b2 * v[i] + (1.f - b2) * gr * gr;
    m[i] = mi;
    v[i] = vi;
    const float pi = p[i];
    const float u = (mi * bc1) / (sqrtf(vi * bc2) + eps) + wd * pi;
    g[i] = u;   // the gradient buffer is consumed: reuse it for the update direction
    sp += pi * pi;
    su += u * u;
  }
  sp = wave_sum(sp);
  su = wave_sum(su);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = sp; red[1][w] = su; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < kT / 64; ++k) { a += red[0][k]; b += red[1][k]; }
    partial[blockIdx.x] = make_float2(a, b);
  }
}

__global__ void __launch_bounds__(kT)
lamb_norm_kernel(const Chunk* __restrict__ chunks, int nchunks,
                 const float2* __restrict__ partial, float* __restrict__ norms) {
  __shared__ float red[2][kT / 64];
  const int r0 = blockIdx.x;
  const int seg = chunks[r0].seg;
  if (r0 > 0 && chunks[r0 - 1].seg == seg) return;   // block-uniform: not the tensor's first row
  // thread t adds rows r0 + t, r0 + t + kT, ... of the run in that order, then one wave / block
  // tree; a tensor's rows are contiguous in the table, so a thread stops at the first other one
  float sp = 0.f, su = 0.f;
  for (int r = r0 + threadIdx.x; r < nchunks && chunks[r].seg == seg; r += kT) {
    const float2 v = partial[r];
    sp += v.x;
    su += v.y;
  }
  sp = wave_sum(sp);
  su = wave_sum(su);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sp; red[1][threadIdx.x >> 6] = su; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < kT / 64; ++k) { a += red[0][k]; b += red[1][k]; }
    norms[2 * seg] = a;
    norms[2 * seg + 1] = b;
  }
}

__global__ void __launch_bounds__(kT)
lamb_phase2_kernel(float* __restrict__ p, const float* __restrict__ u,
                   bf16_t* __restrict__ shadow, const Chunk* __restrict__ chunks,
                   const float* __restrict__ lr_ptr, const float* __restrict__ norms) {
  const Chunk c = chunks[blockIdx.x];
  const float pn = sqrtf(norms[2 * c.seg]), un = sqrtf(norms[2 * c.seg + 1]);
  const float trust = (pn > 0.f && un > 0.f) ? pn / un : 1.f;
  const float step = *lr_ptr * trust;
  for (int j = threadIdx.x; j < c.len; j += kT) {
    const long i = c.start + j;
    const float pi = p[i] - step * u[i];
    p[i] = pi;
    if (shadow) shadow[i] = f2bf(pi);
  }
}

// ---- LARS: the LAMB chunk table, but the per-tensor norms go through a slab (one partial row
// per chunk, plain stores) that every update block of the tensor re-adds in the same fixed
// order -- no float atomics, so the trust ratio and the whole update are bitwise reproducible
// and every block of a tensor forms the bit-identical step size.
// segs[seg] = {first_row, row_count, decayed, 0}: the tensor's rows in THIS chunk table.
__global__ void __launch_bounds__(kT)
lars_norm_kernel(const float* __restrict__ p, const float* __restrict__ g,
                 const Chunk* __restrict__ chunks, const int4* __restrict__ segs, float gscale_v,
                 const float* __restrict__ gmul, float2* __restrict__ partial, int* nonfinite) {
  __shared__ float red[2][kT / 64];
  const float gscale = gmul ? *gmul : gscale_v;
  const Chunk c = chunks[blockIdx.x];
  if (!segs[c.seg].z) return;   // no trust ratio: the update pass flags this tensor's gradients
  const float* pw = p + c.start;
  const float* gw = g + c.start;
  const int n4 = c.len >> 2;
  float sw = 0.f, sg = 0.f;
  for (int j = threadIdx.x; j < n4; j += kT) {
    const float4 pv = reinterpret_cast<const float4*>(pw)[j];
    const float4 gv = reinterpret_cast<const float4*>(gw)[j];
    const float pp[4] = {pv.x, pv.y, pv.z, pv.w};
    const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      flag_nonfinite(nonfinite, gg[k]);
      const float gr = gg[k] * gscale;
      sw += pp[k] * pp[k];
      sg += gr * gr;
    }
  }
  // scalar tail
  for (int j = n4 * 4 + threadIdx.x; j < c.len; j += kT) {
    flag_nonfinite(nonfinite, gw[j]);
    const float gr = gw[j] * gscale;
    sw += pw[j] * pw[j];
    sg += gr * gr;
  }
  sw = wave_sum(sw);
  sg = wave_sum(sg);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sw; red[1][threadIdx.x >> 6] = sg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < kT / 64; ++k) { a += red[0][k]; b += red[1][k]; }
    partial[blockIdx.x] = make_float2(a, b);
  }
}

__global__ void __launch_bounds__(kT)
lars_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ a,
                   bf16_t* __restrict__ shadow, const Chunk* __restrict__ chunks,
                   const int4* __restrict__ segs, const float* __restrict__ lr_ptr,
                   const float2* __restrict__ partial, float momentum, float wd, float eeta,
                   float eps, float gscale_v, const float* __restrict__ gmul, int nesterov,
                   int* nonfinite) {
  __shared__ float red[2][kT / 64];
  const float gscale = gmul ? *gmul : gscale_v;
  const Chunk c = chunks[blockIdx.x];
  const int4 seg = segs[c.seg];
  const bool decayed = seg.z != 0;
  float s = *lr_ptr, wdv = 0.f;
  if (decayed) {   // block-uniform
    // thread t adds rows t, t + kT, ... in that order, then the same wave / block tree in every
    // block of the tensor
    float sw = 0.f, sg = 0.f;
    for (int r = threadIdx.x; r < seg.y; r += kT) {
      const float2 v = partial[seg.x + r];
      sw += v.x;
      sg += v.y;
    }
    sw = wave_sum(sw);
    sg = wave_sum(sg);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sw; red[1][threadIdx.x >> 6] = sg; }
    __syncthreads();
    float tw = 0.f, tg = 0.f;
    for (int k = 0; k < kT / 64; ++k) { tw += red[0][k]; tg += red[1][k]; }
    const float wn = sqrtf(tw), gn = sqrtf(tg);
    const float trust = (wn > 0.f && gn > 0.f) ? eeta * wn / (gn + wd * wn + eps) : 1.f;
    s *= trust;
    wdv = wd;
  }
  int* const flag = decayed ? nullptr : nonfinite;   // the norm pass saw the decayed tensors
  float* pw = p + c.start;
  const float* gw = g + c.start;
  float* aw = a + c.start;
  bf16_t* sh = shadow ? shadow + c.start : nullptr;
  const int n4 = c.len >> 2;
  for (int j = threadIdx.x; j < n4; j += kT) {
    const float4 pv = reinterpret_cast<float4*>(pw)[j];
    const float4 gv = reinterpret_cast<const float4*>(gw)[j];
    const float4 av = reinterpret_cast<float4*>(aw)[j];
    float pp[4] = {pv.x, pv.y, pv.z, pv.w};
    const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
    float aa[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      flag_nonfinite(flag, gg[k]);
      const float u = s * (gg[k] * gscale + wdv * pp[k]);
      aa[k] = momentum * aa[k] + u;
      pp[k] -= nesterov ? u + momentum * aa[k] : aa[k];
    }
    reinterpret_cast<float4*>(pw)[j] = make_float4(pp[0], pp[1], pp[2], pp[3]);
    reinterpret_cast<float4*>(aw)[j] = make_float4(aa[0], aa[1], aa[2], aa[3]);
    if (sh) {
      uint2 o;
      o.x = pack2(pp[0], pp[1]);
      o.y = pack2(pp[2], pp[3]);
      reinterpret_cast<uint2*>(sh)[j] = o;
    }
  }
  // scalar tail
  for (int j = n4 * 4 + threadIdx.x; j < c.len; j += kT) {
    flag_nonfinite(flag, gw[j]);
    const float u = s * (gw[j] * gscale + wdv * pw[j]);
    const float ai = momentum * aw[j] + u;
    aw[j] = ai;
    const float pi = pw[j] - (nesterov ? u + momentum * ai : ai);
    pw[j] = pi;
    if (sh) sh[j] = f2bf(pi);
  }
}

__global__ void __launch_bounds__(kT)
sumsq_kernel(const float* __restrict__ x, long n, float* __restrict__ out) {
  __shared__ float red[kT / 64];
  float s = 0.f;
  for (long i = (long)blockIdx.x * kT + threadIdx.x; i < n; i += (long)gridDim.x * kT) {
    const float v = x[i];
    s += v * v;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < kT / 64; ++k) t += red[k];
    atomicAdd(out, t);
  }
}

// ---- Deterministic global gradient norm (clip_by_global_norm inside the fused update).
// Partial pass: the buffer is cut into chunks of kNormChunk elements counted from g; chunk k is
// summed by exactly one block in an order that depends on nothing but the chunk's length, and its
// fp32 sum goes to partial[k] as fp64 with a plain store.  A block walks chunks b, b + G, ...:
// the grid size G decides who adds a chunk, never how.  Finish pass: one block adds the partials
// (and the caller's extra sums) in fp64 in a fixed order and forms the clip multiplier.  No
// atomics, no host read: bit-identical run to run.
//
// Longest chain of fp32 additions a square passes through inside a block, d = 20: 8 into its
// thread's per-component accumulator (kNormChunk / 4 / kT float4 per thread), 2 to combine the
// four accumulators, 1 for the scalar tail, 6 butterfly levels of wave_sum, 3 across the waves.
constexpr int kNormChunk = 8192;
constexpr int kNormBlocks = 2048;
static_assert(kNormChunk % (4 * kT) == 0, "a whole number of float4 per thread");

template <bool kAligned>
__global__ void __launch_bounds__(kT)
grad_norm_partial_kernel(const float* __restrict__ g, long n, long nchunks,
                         double* __restrict__ partial) {
  __shared__ float red[kT / 64];
  for (long k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const float* gc = g + k * kNormChunk;
    const long left = n - k * kNormChunk;
    const int len = left < kNormChunk ? (int)left : kNormChunk;
    const int n4 = len >> 2;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int u = 0; u < kNormChunk / 4 / kT; ++u) {
      const int j = u * kT + threadIdx.x;
      if (j < n4) {
        float4 v;
        if (kAligned) v = reinterpret_cast<const float4*>(gc)[j];
        else v = make_float4(gc[4 * j], gc[4 * j + 1], gc[4 * j + 2], gc[4 * j + 3]);
        s0 += v.x * v.x;
        s1 += v.y * v.y;
        s2 += v.z * v.z;
        s3 += v.w * v.w;
      }
    }
    float s = (s0 + s1) + (s2 + s3);
    // scalar tail: n % 4 != 0 or a short last chunk
    const int jt = n4 * 4 + threadIdx.x;
    if (jt < len) s += gc[jt] * gc[jt];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      float t = red[0];
      for (int w = 1; w < kT / 64; ++w) t += red[w];
      partial[k] = (double)t;
    }
    __syncthreads();   // red is rewritten on the next trip
  }
}

__global__ void __launch_bounds__(kT)
grad_norm_finish_kernel(const double* __restrict__ partial, long nchunks,
                        const double* __restrict__ extra, int nextra, float gscale, float clip,
                        GradNormRecord* __restrict__ rec) {
  __shared__ double red[kT];
  // thread t adds partials t, t + kT, ... in that order, then a fixed tree over the threads
  double s = 0.0;
  for (long k = threadIdx.x; k < nchunks; k += kT) s += partial[k];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kT / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double S = red[0];
    for (int r = 0; r < nextra; ++r) S += extra[r];   // rank order
    const double gs = gscale, c = clip;
    const double norm = gs * sqrt(S);
    // not clipped (and S == 0): gs * c / c == gs exactly -- gs * c is exact in fp64
    double gm = gs * c / (norm > c ? norm : c);
    if (!isfinite(S)) gm = __builtin_nan("");
    rec->S = S;
    rec->norm = (float)norm;
    rec->gmul = (float)gm;
  }
}

// ---- tf.train.ExponentialMovingAverage of the variables: avg -= a * (avg - var), a = 1 - decay
// read from DEVICE memory (a captured graph replays with each step's own decay).  In this form
// avg == var is a bit-exact fixed point.  avg and var sit at the same element offset of their
// flat buffers, so one scalar head of `head` elements brings both to 16-byte alignment; then
// float4, then a scalar tail.  Buffers misaligned differently get head = n: every element goes
// through the (grid-stride) scalar head.  Plain loads and stores, one writer per element.
DTF_DEV float ema_step(float e, float p, float a) { return e - a * (e - p); }

__global__ void __launch_bounds__(kT)
ema_update_kernel(float* __restrict__ avg, const float* __restrict__ var, long n, long head,
                  const float* __restrict__ a_ptr) {
  const float a = *a_ptr;
  const long t0 = (long)blockIdx.x * kT + threadIdx.x;
  const long stride = (long)gridDim.x * kT;
  // head <= 3, or n: all scalar
  for (long i = t0; i < head; i += stride) avg[i] = ema_step(avg[i], var[i], a);
  float4* a4 = reinterpret_cast<float4*>(avg + head);
  const float4* v4 = reinterpret_cast<const float4*>(var + head);
  const long n4 = (n - head) >> 2;
  for (long i = t0; i < n4; i += stride) {
    float4 e = a4[i];
    const float4 p = v4[i];
    e.x = ema_step(e.x, p.x, a);
    e.y = ema_step(e.y, p.y, a);
    e.z = ema_step(e.z, p.z, a);
    e.w = ema_step(e.w, p.w, a);
    a4[i] = e;
  }
  // scalar tail
  for (long i = head + n4 * 4 + t0; i < n; i += stride) avg[i] = ema_step(avg[i], var[i], a);
}

// ---- gradient accumulation over micro-batches: dst = src (ADD false) or dst = dst + src (ADD
// true) over flat fp32 buffers: the store and the add of a held micro-step, and the fold of the
// accumulator into a bucket's gradient range on the update step.  One IEEE add per element (no
// multiply next to it, so nothing to contract).  Same layout as the EMA pass: dst and src sit at
// the same element offset of their flat buffers, a scalar head of `head` elements brings both to
// 16-byte alignment, then float4, then a scalar tail; buffers misaligned differently get
// head = n.  Plain loads and stores, one writer per element.
template <bool ADD>
__global__ void __launch_bounds__(kT)
grad_accumulate_kernel(float* __restrict__ dst, const float* __restrict__ src, long n, long head) {
  const long t0 = (long)blockIdx.x * kT + threadIdx.x;
  const long stride = (long)gridDim.x * kT;
  // head <= 3, or n: all scalar
  for (long i = t0; i < head; i += stride) dst[i] = ADD ? dst[i] + src[i] : src[i];
  float4* d4 = reinterpret_cast<float4*>(dst + head);
  const float4* s4 = reinterpret_cast<const float4*>(src + head);
  const long n4 = (n - head) >> 2;
  for (long i = t0; i < n4; i += stride) {
    float4 s = s4[i];
    if (ADD) {
      const float4 d = d4[i];
      s.x = d.x + s.x;
      s.y = d.y + s.y;
      s.z = d.z + s.z;
      s.w = d.w + s.w;
    }
    d4[i] = s;
  }
  // scalar tail
  for (long i = head + n4 * 4 + t0; i < n; i += stride) dst[i] = ADD ? dst[i] + src[i] : src[i];
}

__global__ void __launch_bounds__(kT)
cast_f32_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * kT + threadIdx.x; i < n; i += (long)gridDim.x * kT)
    y[i] = f2bf(x[i]);
}

inline int grid_for(long n, int per_thread = 1) {
  long g = (n / per_thread + kT - 1) / kT;
  if (g > 2048) g = 2048;
  return (int)(g < 1 ? 1 : g);
}
}  // namespace

void dtf_sgd_momentum(float* p, const float* g, float* a, bf16_t* shadow, long n,
                      const float* lr_ptr, float momentum, float wd, float gscale, int nesterov,
                      int* nonfinite, const float* gmul, hipStream_t st) {
  hipLaunchKernelGGL(sgd_momentum_kernel, dim3(grid_for(n, 4)), dim3(kT), 0, st, p, g, a, shadow, n,
                     lr_ptr, momentum, wd, gscale, gmul, nesterov, nonfinite);
}

void dtf_adam(float* p, const float* g, float* m, float* v, bf16_t* shadow, long n,
              const float* lr_t_ptr, float b1, float b2, float eps, float wd, float gscale,
              int* nonfinite, const float* gmul, hipStream_t st) {
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(kT), 0, st, p, g, m, v, shadow, n,
                     lr_t_ptr, b1, b2, eps, wd, gscale, gmul, nonfinite);
}

void dtf_adagrad(float* p, const float* g, float* acc, bf16_t* shadow, long n,
                 const float* lr_ptr, float gscale, int* nonfinite, const float* gmul,
                 hipStream_t st) {
  hipLaunchKernelGGL(adagrad_kernel, dim3(grid_for(n)), dim3(kT), 0, st, p, g, acc, shadow, n,
                     lr_ptr, gscale, gmul, nonfinite);
}

void dtf_lamb(float* p, float* g, float* m, float* v, bf16_t* shadow, const void* chunks,
              int nchunks, const float* hyper, const float* lr_ptr, float b1, float b2,
              float eps, const float* wd_seg, float gscale, float* norms, float* partial,
              int* nonfinite, const float* gmul, hipStream_t st) {
  hipLaunchKernelGGL(lamb_phase1_kernel, dim3(nchunks), dim3(kT), 0, st, p, g, m, v,
                     (const Chunk*)chunks, hyper, b1, b2, eps, wd_seg, gscale, gmul,
                     (float2*)partial, nonfinite);
  hipLaunchKernelGGL(lamb_norm_kernel, dim3(nchunks), dim3(kT), 0, st, (const Chunk*)chunks,
                     nchunks, (const float2*)partial, norms);
  hipLaunchKernelGGL(lamb_phase2_kernel, dim3(nchunks), dim3(kT), 0, st, p, g, shadow,
                     (const Chunk*)chunks, lr_ptr, norms);
}

int dtf_lamb_chunk_bytes() { return (int)sizeof(Chunk); }

// chunks: the LAMB row layout; segs: int32 {first_row, row_count, decayed, 0} per tensor, indexing
// THIS table; partial: one float2 per row of the table.  g is left untouched.
void dtf_lars(float* p, const float* g, float* a, bf16_t* shadow, const void* chunks, int nchunks,
              const void* segs, const float* lr_ptr, float momentum, float wd, float eeta,
              float eps, float gscale, int nesterov, float* partial, int* nonfinite,
              const float* gmul, hipStream_t st) {
  hipLaunchKernelGGL(lars_norm_kernel, dim3(nchunks), dim3(kT), 0, st, p, g,
                     (const Chunk*)chunks, (const int4*)segs, gscale, gmul, (float2*)partial,
                     nonfinite);
  hipLaunchKernelGGL(lars_update_kernel, dim3(nchunks), dim3(kT), 0, st, p, g, a, shadow,
                     (const Chunk*)chunks, (const int4*)segs, lr_ptr, (const float2*)partial,
                     momentum, wd, eeta, eps, gscale, gmul, nesterov, nonfinite);
}

void dtf_sumsq(const float* x, long n, float* out, hipStream_t st) {
  hipLaunchKernelGGL(sumsq_kernel, dim3(grid_for(n)), dim3(kT), 0, st, x, n, out);
}

int dtf_grad_norm_chunk() { return kNormChunk; }

void dtf_grad_norm_partial(const float* g, long n, double* partial, int max_blocks,
                           hipStream_t st) {
  if (n <= 0) return;
  const long nchunks = (n + kNormChunk - 1) / kNormChunk;
  const long cap = max_blocks > 0 ? max_blocks : kNormBlocks;
  const dim3 grid((unsigned)(nchunks < cap ? nchunks : cap));
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0)
    hipLaunchKernelGGL(grad_norm_partial_kernel<true>, grid, dim3(kT), 0, st, g, n, nchunks,
                       partial);
  else   // same chunks, same order, 4-byte loads
    hipLaunchKernelGGL(grad_norm_partial_kernel<false>, grid, dim3(kT), 0, st, g, n, nchunks,
                       partial);
}

void dtf_grad_norm_finish(const double* partial, long nchunks, const double* extra, int nextra,
                          float gscale, float clip, GradNormRecord* rec, hipStream_t st) {
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(kT), 0, st, partial,
                     nchunks > 0 ? nchunks : 0, extra, nextra > 0 ? nextra : 0, gscale, clip, rec);
}

void dtf_grad_norm(const float* g, long n, double* partial, int max_blocks, const double* extra,
                   int nextra, float gscale, float clip, GradNormRecord* rec, hipStream_t st) {
  dtf_grad_norm_partial(g, n, partial, max_blocks, st);
  dtf_grad_norm_finish(partial, n > 0 ? (n + kNormChunk - 1) / kNormChunk : 0, extra, nextra,
                       gscale, clip, rec, st);
}

void dtf_cast_f32_bf16(const float* x, bf16_t* y, long n, hipStream_t st) {
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid_for(n)), dim3(kT), 0, st, x, y, n);
}

void dtf_ema_update(float* avg, const float* var, long n, const float* a_ptr, int max_blocks,
                    hipStream_t st) {
  if (n <= 0) return;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(avg), pv = reinterpret_cast<uintptr_t>(var);
  // elements up to the next 16-byte boundary; buffers misaligned differently (never the flat
  // buffers' case) take the scalar path for every element
  long head = (long)(((16 - (pa & 15)) & 15) >> 2);
  if ((pa & 15) != (pv & 15) || (pa & 3) || head > n) head = n;
  int grid = grid_for(n, 4);
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  hipLaunchKernelGGL(ema_update_kernel, dim3(grid), dim3(kT), 0, st, avg, var, n, head, a_ptr);
}

void dtf_grad_accumulate(float* dst, const float* src, long n, int mode, int max_blocks,
                         hipStream_t st) {
  if (n <= 0) return;
  const uintptr_t pd = reinterpret_cast<uintptr_t>(dst), ps = reinterpret_cast<uintptr_t>(src);
  // as dtf_ema_update: a bucket or owner range starts at any element of the flat buffers, at
  // the same one in both; buffers misaligned differently take the scalar path throughout
  long head = (long)(((16 - (pd & 15)) & 15) >> 2);
  if ((pd & 15) != (ps & 15) || (pd & 3) || head > n) head = n;
  int grid = grid_for(n, 4);
  if (max_blocks > 0 && grid > max_blocks) grid = max_blocks;
  if (mode)
    hipLaunchKernelGGL(grad_accumulate_kernel<true>, dim3(grid), dim3(kT), 0, st, dst, src, n,
                       head);
  else
    hipLaunchKernelGGL(grad_accumulate_kernel<false>, dim3(grid), dim3(kT), 0, st, dst, src, n,
                       head);
}
