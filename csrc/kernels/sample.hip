// Token sampling for generation: temperature, top-k, top-p (nucleus) and the draw, one kernel per
// decode step.  dtf_sample_tokens, per logits row b (see ``reference.sample_tokens``):
//   key_i  = 16-bit monotone key of the stored bf16 logit (negatives: all bits flipped; others:
//            sign bit set), columns >= V never candidates;
//   top-k  : keep key_i >= the k-th largest key (ties with the k-th kept);
//   top-p  : of those keep key_i >= t, t the largest key with
//            sum{m_i : key_i >= t} >= top_p * (kept mass), m_i = exp2((x_i - xmax) c),
//            c = log2(e) / temperature;
//   draw   : u = (fmix32(fmix32(b * 0x9E3779B1 + seed) + counter[b]) >> 8) * 2^-24; the token is
//            the lowest kept index whose inclusive running mass (ascending index) exceeds u Z;
//   logprob = ((x_tok - xmax) c - log2 Z) ln 2;   greedy: lowest index of the largest key, Z over
//            all V classes at temperature 1.
//
// Design.  One block of 1024 threads per row; the row (61 KB for BERT's 30528 columns) is read
// from HBM ONCE with 16-B loads, turned into keys on load (the >= V tail becomes the sentinel key
// 0, below every real key: -inf is key 0x007f) and kept in LDS, 2 B per column, for every later
// pass.  2 B per column is what lets a whole row stay resident (fp32 masses would not fit); a
// pass recomputes exp2 from the key instead.  No MFMA: every pass is a reduction with one
// transcendental per element at most.
//   * Reduction passes (maximum, histograms, masses) read LDS chunk-strided: thread t takes the
//     16-B chunks t, t + 1024, ...: neighbouring lanes read neighbouring 16 B, conflict-free.
//   * Top-k threshold: exact radix select on the keys.  A 256-bin count histogram of the high byte
//     (integer LDS atomics: their order cannot change a count), wave 0 finds the bin of the k-th
//     largest with a shuffle scan over 4 bins per lane, then the same over the low byte inside
//     that bin.
//   * Top-p threshold: bisection of the key range [top-k threshold, largest key], at most 16
//     rounds of block_sum(m_i over key_i >= mid).  Every thread ends a round with the same total,
//     so the search is block-uniform without a broadcast.  No floating-point atomics anywhere:
//     the same inputs give the same bits.
//   * Draw: thread t owns the CONTIGUOUS chunks [t per, (t + 1) per), per = ceil(chunks / 1024),
//     and sums its kept masses in index order; an exclusive scan (shuffles inside a wave, the 16
//     wave totals through LDS) gives its offset; the first thread whose offset + sum exceeds u Z
//     walks its range.  That thread's running mass ends at exactly the value that made it the
//     owner, so the walk always finds its index.
//   * SUMMATION ORDER (the tests' bound is derived from it).  block_sum: a thread adds its
//     elements in ascending index order (at most R = 8 ceil(chunks / 1024) terms), the wave adds
//     by xor-butterfly 32, 16, .. 1 (6 levels), every thread adds the 16 wave totals in wave order.
//     The draw's scan: the same R terms, 6 shuffle-up levels, the wave totals in wave order.  Every
//     sum is a chain of at most R + 22 fp32 additions.  The exponent (x_i - xmax) c carries three
//     roundings (the difference, c, the product) before v_exp_f32.
//   * Two instantiations, by LDS: 32000 keys (under 64 KB with the tables) and 65536 keys
//     (129 KB of the CU's 160 KB).
#include <stdexcept>
#include <string>

#include "launch.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kNW = kThreads / 64;           // waves per block
constexpr int kSmallKeys = 32000;
constexpr int kLargeKeys = 65536;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

DTF_DEV uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  return h ^ (h >> 16);
}
DTF_DEV uint32_t key_of(uint32_t bits) {
  return bits & 0x8000u ? ~bits & 0xffffu : bits | 0x8000u;
}
DTF_DEV float val_of(uint32_t key) {
  const uint32_t bits = key & 0x8000u ? key ^ 0x8000u : ~key & 0xffffu;
  return __builtin_bit_cast(float, bits << 16);
}
DTF_DEV uint32_t key_at(const uint4& v, int e) {
  const uint32_t w = e < 2 ? v.x : e < 4 ? v.y : e < 6 ? v.z : v.w;
  return e & 1 ? w >> 16 : w & 0xffffu;
}

struct Scratch {
  float f[2][kNW];                           // double-buffered: one barrier per reduction
  int i[2][kNW];
  int hist[256];
  int sel[2];                                // select_bin: the bin, the rank inside it
};

// every thread gets the same total; see SUMMATION ORDER
DTF_DEV float block_sum(float v, Scratch& sm, int& nf) {
  float* s = sm.f[nf++ & 1];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < kNW; ++i) t += s[i];
  return t;
}
template <bool MAX>
DTF_DEV int block_minmax(int v, Scratch& sm, int& ni) {
  int* s = sm.i[ni++ & 1];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int n = __shfl_xor(v, o, 64);
    v = MAX ? max(v, n) : min(v, n);
  }
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = s[0];
#pragma unroll
  for (int i = 1; i < kNW; ++i) t = MAX ? max(t, s[i]) : min(t, s[i]);
  return t;
}

// sum of m_i over key_i >= thr (thr >= 1 leaves the sentinel out)
DTF_DEV float mass_ge(const uint4* keys, int n8, uint32_t thr, float xmax, float c, Scratch& sm,
                      int& nf) {
  float s = 0.f;
  for (int ci = threadIdx.x; ci < n8; ci += kThreads) {
    const uint4 kv = keys[ci];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t k = key_at(kv, e);
      const float m = __builtin_amdgcn_exp2f((val_of(k) - xmax) * c);
      s += k >= thr ? m : 0.f;
    }
  }
  return block_sum(s, sm, nf);
}

// counts of byte (key >> shift) & 255 over the real keys whose bits above that byte equal `hi`
DTF_DEV void histogram(const uint4* keys, int n8, int shift, uint32_t hi, Scratch& sm) {
  if (threadIdx.x < 256) sm.hist[threadIdx.x] = 0;
  __syncthreads();
  for (int ci = threadIdx.x; ci < n8; ci += kThreads) {
    const uint4 kv = keys[ci];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t k = key_at(kv, e);
      if (k != 0 && (k >> shift) >> 8 == hi) atomicAdd(&sm.hist[(k >> shift) & 255], 1);
    }
  }
  __syncthreads();
}

// wave 0: the bin of the k-th largest entry of the count histogram (1 <= k <= total) and k's rank
// among that bin's entries -> sm.sel.  Lane l holds bins 255 - 4 l .. 252 - 4 l.
DTF_DEV void select_bin(int k, Scratch& sm) {
  const int lane = threadIdx.x;
  int cnt[4], tot = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    cnt[e] = sm.hist[255 - (4 * lane + e)];
    tot += cnt[e];
  }
  int incl = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(incl, o, 64);
    if (lane >= o) incl += n;
  }
  int r = incl - tot;
  if (r < k && k <= incl) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (r < k && k <= r + cnt[e]) {
        sm.sel[0] = 255 - (4 * lane + e);
        sm.sel[1] = k - r;
      }
      r += cnt[e];
    }
  }
}

template <int NKEYS>
__global__ void __launch_bounds__(kThreads) sample_kernel(const SampleArgs g) {
  __shared__ __attribute__((aligned(16))) uint16_t key_lds[NKEYS];
  __shared__ Scratch sm;
  uint4* keys = reinterpret_cast<uint4*>(key_lds);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int V = g.V, n8 = (V + 7) >> 3;            // chunks that hold a real column
  int nf = 0, ni = 0;

  // ---- the one HBM read: keys into LDS, the largest key on the way
  const uint4* row = reinterpret_cast<const uint4*>(g.logits + (long)b * g.ld);
  int kmax = 0;
  for (int ci = tid; ci < n8; ci += kThreads) {
    const uint4 v = row[ci];
    uint32_t k[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      k[e] = ci * 8 + e < V ? key_of(key_at(v, e)) : 0u;
      kmax = max(kmax, (int)k[e]);
    }
    keys[ci] = make_uint4(k[0] | k[1] << 16, k[2] | k[3] << 16, k[4] | k[5] << 16,
                          k[6] | k[7] << 16);
  }
  kmax = block_minmax<true>(kmax, sm, ni);         // its barrier also publishes the keys
  const float xmax = val_of(kmax);

  if (g.greedy) {
    int first = 0x7fffffff;
    for (int ci = tid; ci < n8; ci += kThreads) {
      const uint4 kv = keys[ci];
#pragma unroll
      for (int e = 7; e >= 0; --e)
        if ((int)key_at(kv, e) == kmax) first = min(first, ci * 8 + e);
    }
    first = block_minmax<false>(first, sm, ni);
    const float Z = mass_ge(keys, n8, 1u, xmax, g.c, sm, nf);
    if (tid == 0) {
      g.tokens[b] = first;
      g.logprob[b] = -__builtin_amdgcn_logf(Z) * kLn2;
    }
    return;
  }

  // ---- top-k: exact radix select of the k-th largest key
  uint32_t thr = 1u;
  if (g.top_k > 0 && g.top_k < V) {
    histogram(keys, n8, 8, 0u, sm);
    if (tid < 64) select_bin(g.top_k, sm);
    __syncthreads();
    const uint32_t hi = sm.sel[0];
    const int rank = sm.sel[1];
    __syncthreads();                                // sel is rewritten below
    histogram(keys, n8, 0, hi, sm);
    if (tid < 64) select_bin(rank, sm);
    __syncthreads();
    thr = hi << 8 | (uint32_t)sm.sel[0];
  }

  // ---- top-p: the largest key whose upper mass reaches top_p of the kept mass
  if (g.top_p < 1.f) {
    const float need = g.top_p * mass_ge(keys, n8, thr, xmax, g.c, sm, nf);
    uint32_t lo = thr, hi = kmax;                   // the predicate holds at lo
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (mass_ge(keys, n8, mid, xmax, g.c, sm, nf) >= need) lo = mid; else hi = mid - 1;
    }
    thr = lo;
  }

  // ---- draw: contiguous ranges, exclusive scan, the owner walks
  const uint32_t h = fmix32(fmix32((uint32_t)b * 0x9E3779B1u + g.seed) + (uint32_t)g.counter[b]);
  const float u = (float)(h >> 8) * 0x1p-24f;
  const int per = (n8 + kThreads - 1) / kThreads;
  const int c0 = min(tid * per, n8), c1 = min(c0 + per, n8);
  float s = 0.f;
  for (int ci = c0; ci < c1; ++ci) {
    const uint4 kv = keys[ci];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t k = key_at(kv, e);
      const float m = __builtin_amdgcn_exp2f((val_of(k) - xmax) * g.c);
      s += k >= thr ? m : 0.f;
    }
  }
  float incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float n = __shfl_up(incl, o, 64);
    if (lane >= o) incl += n;
  }
  float* tot = sm.f[nf++ & 1];
  if (lane == 63) tot[w] = incl;
  float excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = 0.f;
  __syncthreads();
  float Z = 0.f, base = 0.f;
#pragma unroll
  for (int i = 0; i < kNW; ++i) {
    if (i == w) base = Z;
    Z += tot[i];
  }
  excl += base;
  const float target = u * Z;
  // the first thread that holds mass and whose inclusive mass passes the target; should rounding
  // leave none, the last thread that holds mass
  const bool has = s > 0.f;
  const int pass = block_minmax<false>(has && excl + s > target ? tid : 0x7fffffff, sm, ni);
  const int last = block_minmax<true>(has ? tid : -1, sm, ni);
  const bool fallback = pass == 0x7fffffff;
  if (tid != (fallback ? last : pass)) return;
  float r = 0.f, xt = xmax;
  int tok = -1;
  for (int ci = c0; ci < c1; ++ci) {
    const uint4 kv = keys[ci];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t k = key_at(kv, e);
      const float x = val_of(k);
      const float m = __builtin_amdgcn_exp2f((x - xmax) * g.c);
      if (k >= thr && m > 0.f) {
        r += m;
        if (fallback || (tok < 0 && excl + r > target)) {
          tok = ci * 8 + e;
          xt = x;
        }
      }
    }
  }
  g.tokens[b] = tok;
  g.logprob[b] = ((xt - xmax) * g.c - __builtin_amdgcn_logf(Z)) * kLn2;
}

}  // namespace

// the widest row (columns that hold a class, rounded up to 8) of each instantiation
int dtf_sample_max_keys(bool large) { return large ? kLargeKeys : kSmallKeys; }

void dtf_sample_tokens(const bf16_t* logits, const int* counter, int64_t* tokens, float* logprob,
                       int B, int V, int ld, uint32_t seed, float temperature, int top_k,
                       float top_p, hipStream_t st) {
  if (!logits || !counter || !tokens || !logprob)
    throw std::runtime_error("sample_tokens: null pointer");
  if (B < 1 || V < 1 || V > ld) throw std::runtime_error("sample_tokens: B >= 1, 1 <= vocab <= ld");
  if (ld % 8 || ((uintptr_t)logits & 15))
    throw std::runtime_error("sample_tokens: rows must be 16-B aligned (ld % 8 == 0)");
  if (!(temperature >= 0.f) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f))
    throw std::runtime_error("sample_tokens: temperature >= 0, top_k >= 0, 0 < top_p <= 1");
  const int nkeys = (V + 7) / 8 * 8;
  if (nkeys > kLargeKeys)
    throw std::runtime_error("sample_tokens: vocab " + std::to_string(V) + " exceeds " +
                             std::to_string(kLargeKeys) + " keys");
  const bool greedy = temperature == 0.f;
  const SampleArgs g{logits, counter, tokens, logprob, V, ld, seed, top_k, top_p,
                     (float)(1.4426950408889634 / (greedy ? 1.0 : (double)temperature)), greedy};
  if (nkeys <= kSmallKeys)
    hipLaunchKernelGGL(sample_kernel<kSmallKeys>, dim3(B), dim3(kThreads), 0, st, g);
  else
    hipLaunchKernelGGL(sample_kernel<kLargeKeys>, dim3(B), dim3(kThreads), 0, st, g);
}
