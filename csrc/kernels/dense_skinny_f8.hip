// The skinny-M dense layer of dense_skinny.hip on FP8 (e4m3) weights:
//   y[M, N] = epi(x[M, K] @ Wq[N, K]^T + b[N]),   Wq[n][k] = float(q[n][k]) * scale[n][k / 64],
// 1 <= M <= 64, x / y bf16, q OCP e4m3 bytes, scale fp32 powers of two (the rule of kv_f8.h on
// every 64-k unit of a row), b fp32, fp32 accumulation, one rounding of the result.  Wq is exact
// in bf16, so this is the bf16 kernel on the dequantised matrix at half the streamed bytes; the
// split over N and K, the wave-order merge, the split-order combine, the epilogues and the
// deferred LayerNorm (PRE / RES) are those of dense_skinny.hip (dense_skinny_common.h).
//
// What differs.
//   * Weight load.  A lane's one 16-B load is 16 k of one row: lane (li, gq), li = lane % 16,
//     gq = lane / 16, holds bytes 64 u + 16 gq ..+16 of row n0 + li for unit u -- one load per
//     lane and unit, 64 contiguous bytes per row -- and uses bytes 8 j ..+8 of them as the B
//     operand of MFMA step j (j = 0, 1).  Element e of k-group gq in step j of unit u is therefore
//         k = 64 u + 16 gq + 8 j + e          (the bf16 kernel: 64 u + 32 j + 8 gq + e),
//     and the A operand of that step is x[m][64 u + 16 gq + 8 j ..+8]: the lane's two 16-B loads
//     of x are one contiguous 32 B.  A dot product does not care in which order its k arrive as
//     long as A and B agree.  The LayerNorm-on-load path indexes gamma and beta with the same k.
//   * Dequantisation in registers, just before the MFMA: v_cvt_scalef32_pk_bf16_fp8 makes two
//     bf16 from two bytes and the unit's scale, four of them one B operand.  The scale of
//     (row, unit) is one fp32 per lane and unit, loaded with the unit's bytes (the 4 k-groups of
//     a row load the same word).  One dword per unit rather than a float4 per 4 units: a wave's
//     share of the units starts anywhere and K / 64 need not be a multiple of 4, so the wider
//     load would be unaligned and, on the last row, past the end.
//   * Loads in flight.  A unit is 1 KB of weights per wave, half the bf16 kernel's.  UB = 8 / 8 /
//     4 / 4 units for MT = 1 .. 4 (8 / 8 / 4 / 4 KB per wave).  MT = 1 does not double the bf16
//     kernel's 8 units: at UB = 16 the scheduler hoists every x load of the batch and the kernel
//     takes 242 VGPRs, one wave per SIMD, and at K = 768 a wave's whole share is 3 units anyway,
//     so there the bytes in flight per CU are a matter of occupancy (94 VGPRs, 4 waves per SIMD,
//     against the bf16 kernel's 3), not of batch length.  The table is in profiles/SKINNY_W8.md.
//     A batch is `nb` <= UB units, every load guarded by the wave-uniform i < nb, so a short
//     share (3 units at K = 768) is ONE batch and one round trip to HBM with no unit-by-unit tail
//     loop; K = 3072 is two batches a wave.  The x operands come from L2 and are loaded after the
//     batch's weights, XB units at a time, so that UB units of x need not be live at once.
//   * The quantiser (weight_quantize_f8_kernel) is the cache's fill kernel on a matrix: 4 lanes
//     per 64-k unit, 16 bf16 each.  Not on the hot path.
#include <stdexcept>
#include <string>

#include "dense_skinny_common.h"
#include "kv_f8.h"

namespace {

using namespace dtf_skinny;

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// 8 e4m3 bytes (two dwords) times s = 2^e -> 8 bf16, one MFMA operand
DTF_DEV bf16x8_t dequant8(uint32_t lo, uint32_t hi, float s) {
  uint4 r;
  r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, s, false));
  r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, s, true));
  r.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, s, false));
  r.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, s, true));
  return __builtin_bit_cast(bf16x8_t, r);
}

// the bytes and scales of units u .. u + nb - 1 (nb <= NB, wave-uniform) of the lane's row
template <int NB>
DTF_DEV void load_wq(const uint8_t* qp, const float* sp, int u, int nb, uint4 (&b)[NB],
                     float (&s)[NB]) {
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    b[i] = make_uint4(0u, 0u, 0u, 0u);
    s[i] = 0.f;
    if (i < nb) {
      b[i] = *reinterpret_cast<const uint4*>(qp + (size_t)(u + i) * kUnit);
      s[i] = sp[u + i];
    }
  }
}

// The MFMAs of a loaded batch.  x is loaded here, XB units at a time; PRE: normalised on the
// way, ms[t] the (mean, rstd) of the lane's row of tile t, gp / bp the lane's 16 k of gamma /
// beta in unit 0.
template <int MT, int NB, int XB, bool PRE>
DTF_DEV void mma_batch(const uint4 (&b)[NB], const float (&s)[NB], const bf16_t* const (&xp)[MT],
                       const bool (&live)[MT], const float2 (&ms)[MT], const float* gp,
                       const float* bp, int u, int nb, f32x4_t (&acc)[MT]) {
#pragma unroll
  for (int i0 = 0; i0 < NB; i0 += XB) {
    if (i0 >= nb) break;                   // wave-uniform
    uint4 a[MT][XB][2];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int i = 0; i < XB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          a[t][i][j] = make_uint4(0u, 0u, 0u, 0u);
          if (live[t] && i0 + i < nb)
            a[t][i][j] =
                *reinterpret_cast<const uint4*>(xp[t] + (size_t)(u + i0 + i) * kUnit + 8 * j);
        }
#pragma unroll
    for (int i = 0; i < XB; ++i) {
      if (i0 + i >= nb) break;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint4& q = b[i0 + i];
        const bf16x8_t bw = dequant8(j ? q.z : q.x, j ? q.w : q.y, s[i0 + i]);
        if constexpr (PRE) {
          float gm[8], bt[8];
          load8f(gp, (u + i0 + i) * kUnit + 8 * j, gm);
          load8f(bp, (u + i0 + i) * kUnit + 8 * j, bt);
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            bf16x8_t op = lnb8(a[t][i][j], ms[t], gm, bt);
            if (!live[t]) op = (bf16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
            acc[t] = mfma(op, bw, acc[t]);
          }
        } else {
#pragma unroll
          for (int t = 0; t < MT; ++t)
            acc[t] = mfma(__builtin_bit_cast(bf16x8_t, a[t][i][j]), bw, acc[t]);
        }
      }
    }
  }
}

template <int MT, bool PRE, int RES>
__global__ void __launch_bounds__(64 * kWaves) dense_skinny_w8_kernel(const DenseSkinnyW8Args a) {
  constexpr int UB = MT <= 2 ? 8 : 4;                     // units of W in flight
  constexpr int XB = MT <= 2 ? 4 : 2;                     // units of x loaded together
  const DenseSkinnyLnArgs& h = a.h;
  const DenseSkinnyArgs& g = h.d;
  __shared__ __attribute__((aligned(16))) float Ms[kWaves * MT * 16 * kMp];
  __shared__ float2 St[kMaxM];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, gq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * 16, split = blockIdx.y;
  const int U = g.K / kUnit;
  const int u0 = (int)((long)split * U / g.splits);
  const int nu = (int)((long)(split + 1) * U / g.splits) - u0;
  const int wu1 = u0 + (w + 1) * nu / kWaves;
  int u = u0 + w * nu / kWaves;

  const uint8_t* qp = a.q + (size_t)(n0 + li) * g.K + 16 * gq;
  const float* sp = a.scale + (size_t)(n0 + li) * U;
  const bf16_t* xp[MT];
  bool live[MT];
  float2 ms[MT];
  f32x4_t acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    live[t] = 16 * t + li < g.M;
    xp[t] = g.x + (size_t)(16 * t + li) * g.ldx + 16 * gq;
    ms[t] = make_float2(0.f, 0.f);
    acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  const float* gp = PRE ? h.ln_gamma + 16 * gq : nullptr;
  const float* bp = PRE ? h.ln_beta + 16 * gq : nullptr;

  // The first batch (none for a wave without a unit); PRE: its weights are in flight while the
  // block forms the statistics of x.
  uint4 b[UB];
  float s[UB];
  int nb = min(UB, wu1 - u);
  load_wq<UB>(qp, sp, u, nb, b, s);
  if constexpr (PRE) {
    row_stats<4 * MT>(h, g.x, g.ldx, 0, g.M, w, lane, St);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < MT; ++t)
      if (live[t]) ms[t] = St[16 * t + li];
  }
  mma_batch<MT, UB, XB, PRE>(b, s, xp, live, ms, gp, bp, u, nb, acc);
  for (u += UB; u < wu1; u += UB) {
    nb = min(UB, wu1 - u);
    load_wq<UB>(qp, sp, u, nb, b, s);
    mma_batch<MT, UB, XB, PRE>(b, s, xp, live, ms, gp, bp, u, nb, acc);
  }
  mfma_fence();
  // the residual's statistics: published by the merge barrier
  if constexpr (RES == 2)
    if (g.splits == 1) row_stats<4 * MT>(h, h.res, h.ldres, 0, g.M, w, lane, St);

  merge_waves<MT>(Ms, acc, tid, w, g.M, [&](int m, int c, float4 sum) {
    if (g.splits == 1)
      store4_res<RES>(h, St, m, n0 + c, sum);
    else
      *reinterpret_cast<float4*>(g.ws + ((size_t)split * g.M + m) * g.N + n0 + c) = sum;
  });
}

// One thread per 16 elements, 4 threads per 64-k unit: w [n / 4 units of 64] -> bytes and scales
__global__ void __launch_bounds__(256) weight_quantize_f8_kernel(const bf16_t* w, uint8_t* q,
                                                                 float* scale, long n) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;                    // n % 4 == 0: the 4 lanes of a unit leave together
  const uint4 lo = *reinterpret_cast<const uint4*>(w + idx * 16);
  const uint4 hi = *reinterpret_cast<const uint4*>(w + idx * 16 + 8);
  const int e = kv_f8_exponent(kv_f8_group4_max(max(kv_f8_absmax8(lo), kv_f8_absmax8(hi))));
  *reinterpret_cast<uint4*>(q + idx * 16) = kv_f8_quantize16(lo, hi, kv_f8_pow2(-e));
  if ((idx & 3) == 0) scale[idx >> 2] = kv_f8_pow2(e);
}

template <bool PRE, int RES>
void launch(const DenseSkinnyW8Args& a, hipStream_t st) {
  const dim3 grid(a.h.d.N / 16, a.h.d.splits), block(64 * kWaves);
  switch ((a.h.d.M + 15) / 16) {
    case 1: hipLaunchKernelGGL((dense_skinny_w8_kernel<1, PRE, RES>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((dense_skinny_w8_kernel<2, PRE, RES>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((dense_skinny_w8_kernel<3, PRE, RES>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((dense_skinny_w8_kernel<4, PRE, RES>), grid, block, 0, st, a); break;
  }
}

void check_pair(const uint8_t* q, const float* scale) {
  if (!q || !scale || (uintptr_t)scale % 4)
    throw std::runtime_error("dense_skinny_w8: the weight is a (bytes, fp32 scales) pair");
}

}  // namespace

void dtf_weight_quantize_f8(const bf16_t* w, uint8_t* q, float* scale, int N, int K,
                            hipStream_t st) {
  if (!w || !q || !scale || ((uintptr_t)w | (uintptr_t)q) % 16)
    throw std::runtime_error("weight_quantize_f8: null or unaligned pointer");
  if (N < 1 || K < kUnit || K % kUnit)
    throw std::runtime_error("weight_quantize_f8: N >= 1 and K a multiple of 64, got N " +
                             std::to_string(N) + ", K " + std::to_string(K));
  const long n = (long)N * K / 16;
  if (n > (1L << 31) * 256 - 256)
    throw std::runtime_error("weight_quantize_f8: the matrix is too large for one launch");
  hipLaunchKernelGGL(weight_quantize_f8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     st, w, q, scale, n);
}

void dtf_dense_skinny_w8(const bf16_t* x, const uint8_t* q, const float* scale, const float* bias,
                         bf16_t* y, float* ws, int M, int N, int K, int ldx, int epi, int splits,
                         hipStream_t st) {
  check_pair(q, scale);
  splits = dtf_dense_skinny_checked_splits(x, q, bias, y, ws, M, N, K, ldx, epi, splits);
  const DenseSkinnyW8Args a{{{x, nullptr, bias, y, ws, M, N, K, ldx, splits, epi}}, q, scale};
  launch<false, 0>(a, st);
  if (splits > 1) dtf_dense_skinny_combine(a.h, 0, st);
}

void dtf_dense_skinny_ln_w8(const DenseSkinnyLnArgs& ln, const uint8_t* q, const float* scale,
                            hipStream_t st) {
  check_pair(q, scale);
  DenseSkinnyW8Args a{ln, q, scale};
  DenseSkinnyArgs& g = a.h.d;
  g.w = nullptr;
  g.splits = dtf_dense_skinny_checked_splits(g.x, q, g.bias, g.y, g.ws, g.M, g.N, g.K, g.ldx,
                                             g.epi, g.splits);
  const int res = dtf_dense_skinny_ln_checked_res(a.h);
  if (a.h.pre_ln) {
    if (res == 0) launch<true, 0>(a, st);
    else launch<true, 1>(a, st);
  } else {
    if (res == 1) launch<false, 1>(a, st);
    else launch<false, 2>(a, st);
  }
  if (g.splits > 1) dtf_dense_skinny_combine(a.h, res, st);
}
