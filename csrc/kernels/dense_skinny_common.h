// What the skinny-M dense kernels share (dense_skinny.hip: bf16 weights, dense_skinny_f8.hip: FP8
// weights): the block geometry, the wave-order merge, the epilogues, the row statistics of the
// deferred LayerNorm, and the host-side argument checks and combine launches, which live in
// dense_skinny.hip.  The design is described there.
#pragma once
#include "launch.h"

namespace dtf_skinny {

constexpr int kWaves = 4;        // waves per block
constexpr int kUnit = 64;        // k per unit: two MFMA steps
constexpr int kMp = 20;          // merge row pitch in floats: 80-B rows keep float4 alignment and
                                 // put the 4 k-groups' stores on distinct banks
constexpr int kMaxM = 64;
constexpr int kLnMaxWidth = 1024;
constexpr int kLnV = kLnMaxWidth / 512;      // 16-B loads a lane makes of one row

DTF_DEV f32x4_t mfma(const bf16x8_t& a, const bf16x8_t& b, const f32x4_t& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
DTF_DEV void mfma_fence() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// the epilogue on 4 consecutive columns n .. n + 3 of row m
DTF_DEV void store4(const DenseSkinnyArgs& g, int m, int n, float4 s) {
  if (g.epi) {
    const float4 b = *reinterpret_cast<const float4*>(g.bias + n);
    s.x += b.x; s.y += b.y; s.z += b.z; s.w += b.w;
    if (g.epi == 2) {
      s.x = gelu_f(s.x); s.y = gelu_f(s.y); s.z = gelu_f(s.z); s.w = gelu_f(s.w);
    }
  }
  *reinterpret_cast<uint2*>(g.y + (size_t)m * g.N + n) =
      make_uint2(pack2(s.x, s.y), pack2(s.z, s.w));
}

// The block's merge.  acc[t][r] is y[16 t + 4 gq + r][n0 + li] of wave w's k share: every wave
// leaves its accumulators in Ms [kWaves * MT * 16 * kMp], then thread -> (row, 4 columns) adds
// the waves' sums IN WAVE ORDER and hands the row's sum to emit(m, c, s), c the first of the 4
// columns within the tile.  Holds the block's one barrier after the main loop.
template <int MT, typename Emit>
DTF_DEV void merge_waves(float* Ms, const f32x4_t (&acc)[MT], int tid, int w, int M, Emit emit) {
  const int li = tid & 15, gq = (tid & 63) >> 4;
  float* mine = Ms + w * MT * 16 * kMp;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) mine[(16 * t + 4 * gq + r) * kMp + li] = acc[t][r];
  __syncthreads();

  if (tid >= MT * 64) return;
  const int m = tid >> 2, c = (tid & 3) * 4;
  if (m >= M) return;
  float4 s = *reinterpret_cast<const float4*>(Ms + m * kMp + c);
#pragma unroll
  for (int k = 1; k < kWaves; ++k) {
    const float4 p = *reinterpret_cast<const float4*>(Ms + (k * MT * 16 + m) * kMp + c);
    s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
  }
  emit(m, c, s);
}

// mean / rstd of rows m_lo + w, m_lo + w + 4, ... < m_hi (RW of them at most) of r -> st[row].
// Every load first, then two passes over the registers per row; rows past m_hi reduce zeros, so
// the RW reductions are straight-line code the scheduler can interleave.
template <int RW>
DTF_DEV void row_stats(const DenseSkinnyLnArgs& h, const bf16_t* r, int ld, int m_lo, int m_hi,
                       int w, int lane, float2* st) {
  const int pieces = h.ln_width / 8;
  const float inv = 1.f / (float)h.ln_width;
  uint4 v[RW][kLnV];
#pragma unroll
  for (int i = 0; i < RW; ++i)
#pragma unroll
    for (int j = 0; j < kLnV; ++j) {
      v[i][j] = make_uint4(0u, 0u, 0u, 0u);
      if (m_lo + w + kWaves * i < m_hi && lane + 64 * j < pieces)
        v[i][j] = *reinterpret_cast<const uint4*>(r + (size_t)(m_lo + w + kWaves * i) * ld +
                                                  8 * (lane + 64 * j));
    }
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    float f[kLnV][8], s = 0.f, sq = 0.f;
#pragma unroll
    for (int j = 0; j < kLnV; ++j) {
      unpack8(v[i][j], f[j]);
#pragma unroll
      for (int e = 0; e < 8; ++e) s += f[j][e];
    }
    const float mean = wave_sum(s) * inv;
#pragma unroll
    for (int j = 0; j < kLnV; ++j)
      if (lane + 64 * j < pieces) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = f[j][e] - mean;
          sq += d * d;
        }
      }
    const float rstd = rsqrtf(wave_sum(sq) * inv + h.ln_eps);
    const int m = m_lo + w + kWaves * i;
    if (lane == 0 && m < m_hi) st[m] = make_float2(mean, rstd);
  }
}

// lnb of 8 consecutive elements v with their gamma gm / beta bt, packed as one MFMA operand
DTF_DEV bf16x8_t lnb8(const uint4& v, float2 ms, const float (&gm)[8], const float (&bt)[8]) {
  float f[8];
  unpack8(v, f);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = ((f[e] - ms.x) * ms.y) * gm[e] + bt[e];
  return __builtin_bit_cast(bf16x8_t, pack8(f));
}

// store4 with the residual: (s + b[n]) + res, res read plain (RES 1) or as lnb(res) (RES 2)
template <int RES>
DTF_DEV void store4_res(const DenseSkinnyLnArgs& h, const float2* st, int m, int n, float4 s) {
  const DenseSkinnyArgs& g = h.d;
  if constexpr (RES == 0) {
    store4(g, m, n, s);
  } else {
    const float4 b = *reinterpret_cast<const float4*>(g.bias + n);
    const uint2 rv = *reinterpret_cast<const uint2*>(h.res + (size_t)m * h.ldres + n);
    float r[4] = {__builtin_bit_cast(float, rv.x << 16),
                  __builtin_bit_cast(float, rv.x & 0xffff0000u),
                  __builtin_bit_cast(float, rv.y << 16),
                  __builtin_bit_cast(float, rv.y & 0xffff0000u)};
    if constexpr (RES == 2) {
      const float2 ms = st[m];
      const float4 gm = *reinterpret_cast<const float4*>(h.ln_gamma + n);
      const float4 bt = *reinterpret_cast<const float4*>(h.ln_beta + n);
      r[0] = bf2f(f2bf(((r[0] - ms.x) * ms.y) * gm.x + bt.x));
      r[1] = bf2f(f2bf(((r[1] - ms.x) * ms.y) * gm.y + bt.y));
      r[2] = bf2f(f2bf(((r[2] - ms.x) * ms.y) * gm.z + bt.z));
      r[3] = bf2f(f2bf(((r[3] - ms.x) * ms.y) * gm.w + bt.w));
    }
    s.x = (s.x + b.x) + r[0]; s.y = (s.y + b.y) + r[1];
    s.z = (s.z + b.z) + r[2]; s.w = (s.w + b.w) + r[3];
    *reinterpret_cast<uint2*>(g.y + (size_t)m * g.N + n) =
        make_uint2(pack2(s.x, s.y), pack2(s.z, s.w));
  }
}

}  // namespace dtf_skinny

// ---- host side, defined in dense_skinny.hip
// The checks of a launch's shapes, pointers and epilogue (w: the weight bytes, 16-B aligned)
// -> its `splits`.
int dtf_dense_skinny_checked_splits(const bf16_t* x, const void* w, const float* bias,
                                    const bf16_t* y, const float* ws, int M, int N, int K, int ldx,
                                    int epi, int splits);
// ... and of the deferred-LayerNorm arguments (h.d already checked) -> RES: 0 none, 1 plain, 2 lnb
int dtf_dense_skinny_ln_checked_res(const DenseSkinnyLnArgs& h);
// The split-order combine of ws [splits, M, N] with the epilogue of `res` (h.d.splits > 1).
void dtf_dense_skinny_combine(const DenseSkinnyLnArgs& h, int res, hipStream_t st);
