// Skinny-M dense layer for decode steps: y[M, N] = epi(x[M, K] @ W[N, K]^T + b[N]) with
// 1 <= M <= 64, x / W / y bf16, b fp32, fp32 accumulation, one rounding of the result.
//
// A decode step's GEMMs have M = batch rows: every weight byte is used for M rows and never
// again, so the call is the time it takes to stream W from HBM.  The persistent GEMM of gemm.hip
// (256-row tiles, operands staged through LDS for reuse, one block per output tile) gives such a
// shape one row tile of padding and as many blocks as there are column tiles; this kernel is
// built around the weight stream instead.
//
// Design.
//   * W's [N, K] rows ARE the B operand of the 16 x 16 x 32 bf16 MFMA: lane l holds 8 consecutive
//     k of row n = l % 16, k-group l / 16.  One 16-B global load per lane is one operand; W never
//     touches LDS (nothing reuses it) and exactly one wave reads each byte of it, once.
//   * x is the A operand in the same layout (row m = l % 16), loaded by the wave that uses it
//     straight into registers: the waves of a block take DIFFERENT k ranges, so no two waves of a
//     block want the same bytes of x and an LDS stage would serve nobody.  x is at most 384 KB
//     and stays in L2.  Rows at or past M are never loaded: their operand is a select to zero.
//   * M > 16 is ceil(M / 16) row tiles (the template parameter MT) that share each loaded W
//     operand: acc[MT] accumulators per wave, the weight bytes still read once.  Row tiles are
//     not a grid dimension.
//   * The split is over N and K only.  Block (tile, split) owns the 16 columns of `tile` and the
//     64-k units [split U / splits, (split + 1) U / splits) of the U = K / 64; its 4 waves take
//     contiguous shares of those units (a wave without a unit keeps acc = +0), leave their
//     accumulators in LDS and the block adds them IN WAVE ORDER.  splits == 1 applies the
//     epilogue and stores y; otherwise the block's fp32 sums go to ws [splits, M, N] and
//     dense_skinny_combine_kernel adds them IN SPLIT ORDER and applies the epilogue.  No atomics:
//     the same inputs and the same `splits` give the same bits.
//   * Loads in flight: a wave issues the W and x loads of UB units before the first MFMA of the
//     batch -- 16 KB of W per wave at MT = 1 (the decode attention kernel's figure,
//     profiles/DECODE.md), less where the x operands of more row tiles need the registers.
//   * Epilogues: 0 none, 1 + b[n], 2 gelu(. + b[n]) with the gelu_f of common.h that
//     bias_gelu_fwd_kernel applies -- on the fp32 sum, so the result rounds once.
#include <stdexcept>
#include <string>

#include "launch.h"

namespace {

constexpr int kWaves = 4;        // waves per block
constexpr int kUnit = 64;        // k per unit: two MFMA steps, two 16-B loads per lane and row
constexpr int kMp = 20;          // merge row pitch in floats: 80-B rows keep float4 alignment and
                                 // put the 4 k-groups' stores on distinct banks

DTF_DEV f32x4_t mfma(const bf16x8_t& a, const bf16x8_t& b, const f32x4_t& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
DTF_DEV void mfma_fence() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// NB units from unit u on: every load first, then the MFMAs
template <int MT, int NB>
DTF_DEV void run_units(const bf16_t* wp, const bf16_t* const (&xp)[MT], const bool (&live)[MT],
                       int u, f32x4_t (&acc)[MT]) {
  bf16x8_t b[NB][2], a[MT][NB][2];
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      b[i][j] = *reinterpret_cast<const bf16x8_t*>(wp + (size_t)(u + i) * kUnit + 32 * j);
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        a[t][i][j] = (bf16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
        if (live[t])
          a[t][i][j] = *reinterpret_cast<const bf16x8_t*>(xp[t] + (size_t)(u + i) * kUnit + 32 * j);
      }
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = mfma(a[t][i][j], b[i][j], acc[t]);
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

template <int MT>
__global__ void __launch_bounds__(64 * kWaves) dense_skinny_kernel(const DenseSkinnyArgs g) {
  constexpr int UB = MT == 1 ? 8 : MT == 2 ? 4 : 2;       // units loaded ahead of their MFMAs
  __shared__ __attribute__((aligned(16))) float Ms[kWaves * MT * 16 * kMp];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, gq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * 16, split = blockIdx.y;
  const int U = g.K / kUnit;
  const int u0 = (int)((long)split * U / g.splits);
  const int nu = (int)((long)(split + 1) * U / g.splits) - u0;
  const int wu1 = u0 + (w + 1) * nu / kWaves;
  int u = u0 + w * nu / kWaves;

  const bf16_t* wp = g.w + (size_t)(n0 + li) * g.K + 8 * gq;
  const bf16_t* xp[MT];
  bool live[MT];
  f32x4_t acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    live[t] = 16 * t + li < g.M;
    xp[t] = g.x + (size_t)(16 * t + li) * g.ldx + 8 * gq;
    acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  for (; u + UB <= wu1; u += UB) run_units<MT, UB>(wp, xp, live, u, acc);
  for (; u < wu1; ++u) run_units<MT, 1>(wp, xp, live, u, acc);
  mfma_fence();

  // acc[t][r] is y[16 t + 4 gq + r][n0 + li]
  float* mine = Ms + w * MT * 16 * kMp;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) mine[(16 * t + 4 * gq + r) * kMp + li] = acc[t][r];
  __syncthreads();

  // thread -> (row, 4 columns): the waves' sums added in wave order
  if (tid >= MT * 64) return;
  const int m = tid >> 2, c = (tid & 3) * 4;
  if (m >= g.M) return;
  float4 s = *reinterpret_cast<const float4*>(Ms + m * kMp + c);
#pragma unroll
  for (int k = 1; k < kWaves; ++k) {
    const float4 p = *reinterpret_cast<const float4*>(Ms + (k * MT * 16 + m) * kMp + c);
    s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
  }
  if (g.splits == 1)
    store4(g, m, n0 + c, s);
  else
    *reinterpret_cast<float4*>(g.ws + ((size_t)split * g.M + m) * g.N + n0 + c) = s;
}

// One thread per (row, 4 columns): the partials of the splits added in split order.
__global__ void __launch_bounds__(256) dense_skinny_combine_kernel(const DenseSkinnyArgs g,
                                                                   int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int nq = g.N / 4;
  const int m = idx / nq, n = (idx % nq) * 4;
  const float* p = g.ws + (size_t)m * g.N + n;
  const size_t slab = (size_t)g.M * g.N;
  float4 s = *reinterpret_cast<const float4*>(p);
  for (int k = 1; k < g.splits; ++k) {
    const float4 q = *reinterpret_cast<const float4*>(p + k * slab);
    s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
  }
  store4(g, m, n, s);
}

constexpr int kCus = 256;            // MI355X
constexpr int kMaxM = 64;
// A split must be worth the combine launch: no split below this many 64-k units per block.
// Measured (tools/dense_bench.py --splits, profiles/SKINNY.md): up to K = 3072 no split wins.
// 768 x 3072 at M = 8 takes 11.3 us a call with one split against 15.3 to 15.7 with 2 to 12, and
// in a kernel trace the main kernel of the 48-block grids gains under 1 us from any split (4.2 us
// against 3.7 to 4.8) while the combine launch adds 2.8 to 3.0 us; the 30528 x 768 kernel only
// loses (14.5 us, then 16.7, 17.4, 20.3, 26.3 for 2, 3, 4, 6).  So the threshold lies above every
// measured K: two splits need K >= 8192.  Larger K: not measured.
constexpr int kMinSplitUnits = 64;

}  // namespace

// `splits` for a launch: enough blocks for two per CU, but no split below kMinSplitUnits units.
// A pure function of (N, K); M does not enter (it is never split).
int dtf_dense_skinny_splits(int M, int N, int K) {
  if (M < 1 || N < 16 || K < kUnit)
    throw std::runtime_error("dense_skinny_splits: M >= 1, N >= 16, K >= 64");
  const int tiles = N / 16, U = K / kUnit;
  int want = (2 * kCus + tiles - 1) / tiles;
  const int cap = U / kMinSplitUnits;
  if (want > cap) want = cap;
  return want < 1 ? 1 : want;
}

void dtf_dense_skinny(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, float* ws,
                      int M, int N, int K, int ldx, int epi, int splits, hipStream_t st) {
  if (!x || !w || !y) throw std::runtime_error("dense_skinny: null pointer");
  if (M < 1 || M > kMaxM)
    throw std::runtime_error("dense_skinny: 1 <= M <= 64, got " + std::to_string(M));
  if (N < 16 || N % 16 || N > (1 << 24))
    throw std::runtime_error("dense_skinny: N must be a multiple of 16, at most 2^24, got " +
                             std::to_string(N));
  if (K < kUnit || K % kUnit || K / kUnit > 65535)
    throw std::runtime_error("dense_skinny: K must be a multiple of 64, at least 64, got " +
                             std::to_string(K));
  if (ldx < K || ldx % 8 || ((uintptr_t)x | (uintptr_t)w) % 16 || (uintptr_t)y % 8)
    throw std::runtime_error("dense_skinny: x rows must start 16-B aligned (row stride " +
                             std::to_string(ldx) + " elements) and hold K elements");
  if (epi < 0 || epi > 2) throw std::runtime_error("dense_skinny: epilogue 0, 1 or 2");
  if (epi && (!bias || (uintptr_t)bias % 16))
    throw std::runtime_error("dense_skinny: the bias epilogues need a 16-B aligned bias");
  if (splits == 0) splits = dtf_dense_skinny_splits(M, N, K);
  if (splits < 1 || splits > K / kUnit)
    throw std::runtime_error("dense_skinny: splits " + std::to_string(splits) + " exceeds the " +
                             std::to_string(K / kUnit) + " 64-k units of K");
  if (splits > 1 && (!ws || (uintptr_t)ws % 16))
    throw std::runtime_error("dense_skinny: splits > 1 needs the workspace");
  const DenseSkinnyArgs g{x, w, bias, y, ws, M, N, K, ldx, splits, epi};
  const dim3 grid(N / 16, splits), block(64 * kWaves);
  switch ((M + 15) / 16) {
    case 1: hipLaunchKernelGGL(dense_skinny_kernel<1>, grid, block, 0, st, g); break;
    case 2: hipLaunchKernelGGL(dense_skinny_kernel<2>, grid, block, 0, st, g); break;
    case 3: hipLaunchKernelGGL(dense_skinny_kernel<3>, grid, block, 0, st, g); break;
    default: hipLaunchKernelGGL(dense_skinny_kernel<4>, grid, block, 0, st, g); break;
  }
  if (splits > 1) {
    const int total = M * (N / 4);
    hipLaunchKernelGGL(dense_skinny_combine_kernel, dim3(dtf_cdiv(total, 256)), dim3(256), 0, st,
                       g, total);
  }
}
