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
//
// Deferred LayerNorm (dense_skinny_ln_kernel<MT, PRE, RES>, dtf_dense_skinny_ln).  A decode
// step's bias + residual + LayerNorm launches move at most 64 x 768 elements each and exist only
// because LayerNorm wants whole rows while this kernel splits the columns over blocks.  Here the
// kernel that forms a sub-layer's sum r = a + bias + residual stores r UN-normalised and every
// consumer of LN(r) normalises it itself, lnb(r) = bf16(((r - mean) * rstd) * gamma + beta) with
// fp32 statistics over the stored bf16 row and the biased variance (reference.layer_norm, rounded
// once).  No block waits for another; the determinism rule above holds.
//   * PRE: y = epi(lnb(x) @ W^T + b).  A lane's 16 B of x are unpacked, normalised with the row's
//     mean / rstd and the gamma / beta of those 8 k (two float4 loads each, shared by the row
//     tiles) and packed again just before the MFMA.  Rows at or past M are neither loaded nor
//     normalised: their operand is the same select to zero.
//   * RES = 1: y = bf16(x @ W^T + b + res), res a bf16 [M, N] matrix; RES = 2: res is lnb(res).
//     Added to the fp32 sum after the bias (epi == 1 only), by the block or, with K splits, by
//     dense_skinny_combine_ln_kernel.
//   * Statistics: every block forms mean / rstd of all M rows of the one normalised matrix
//     itself.  Row m goes to wave m % 4; a wave loads all of its up to 4 MT rows first (16 B per
//     lane and 512 columns, so kLnMaxWidth = 1024 is two loads a row), then reduces each row TWICE
//     from those registers: the mean, then the sum of centred squares (E[x^2] - mean^2 cancels
//     for rows with a common offset).  Results go to LDS as float2[64].  PRE: a prologue, after
//     the wave has issued its first batch of W loads (which do not depend on it); RES = 2: between
//     the main loop and the merge, whose barrier then also publishes the statistics.
//   * Width of the normalised rows: a multiple of 16 up to kLnMaxWidth (BERT-large's hidden size;
//     a third load per row was not tried).
#include <stdexcept>
#include <string>

#include "dense_skinny_common.h"

namespace {

using namespace dtf_skinny;

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

  merge_waves<MT>(Ms, acc, tid, w, g.M, [&](int m, int c, float4 s) {
    if (g.splits == 1)
      store4(g, m, n0 + c, s);
    else
      *reinterpret_cast<float4*>(g.ws + ((size_t)split * g.M + m) * g.N + n0 + c) = s;
  });
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
// A split must be worth the combine launch: no split below this many 64-k units per block.
// Measured (tools/dense_bench.py --splits, profiles/SKINNY.md): up to K = 3072 no split wins.
// 768 x 3072 at M = 8 takes 11.3 us a call with one split against 15.3 to 15.7 with 2 to 12, and
// in a kernel trace the main kernel of the 48-block grids gains under 1 us from any split (4.2 us
// against 3.7 to 4.8) while the combine launch adds 2.8 to 3.0 us; the 30528 x 768 kernel only
// loses (14.5 us, then 16.7, 17.4, 20.3, 26.3 for 2, 3, 4, 6).  So the threshold lies above every
// measured K: two splits need K >= 8192.  Larger K: not measured.
constexpr int kMinSplitUnits = 64;

// ---- deferred LayerNorm
template <int NB>
DTF_DEV void load_w(const bf16_t* wp, int u, bf16x8_t (&b)[NB][2]) {
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      b[i][j] = *reinterpret_cast<const bf16x8_t*>(wp + (size_t)(u + i) * kUnit + 32 * j);
}

// run_units with the A operand normalised on load and W already in registers: ms[t] is the
// (mean, rstd) of the lane's row of tile t, gp / bp point at the lane's k-group of gamma / beta
template <int MT, int NB>
DTF_DEV void mma_units_ln(const bf16x8_t (&b)[NB][2], const bf16_t* const (&xp)[MT],
                          const bool (&live)[MT], const float2 (&ms)[MT], const float* gp,
                          const float* bp, int u, int nb, f32x4_t (&acc)[MT]) {
  uint4 a[MT][NB][2];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        a[t][i][j] = make_uint4(0u, 0u, 0u, 0u);
        if (live[t] && i < nb)
          a[t][i][j] = *reinterpret_cast<const uint4*>(xp[t] + (size_t)(u + i) * kUnit + 32 * j);
      }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    if (i >= nb) break;                    // wave-uniform: a first batch shorter than NB units
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float gm[8], bt[8];
      load8f(gp, (u + i) * kUnit + 32 * j, gm);
      load8f(bp, (u + i) * kUnit + 32 * j, bt);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        bf16x8_t op = lnb8(a[t][i][j], ms[t], gm, bt);
        if (!live[t]) op = (bf16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
        acc[t] = mfma(op, b[i][j], acc[t]);
      }
    }
  }
}

template <int MT, bool PRE, int RES>
__global__ void __launch_bounds__(64 * kWaves) dense_skinny_ln_kernel(const DenseSkinnyLnArgs h) {
  constexpr int UB = MT == 1 ? 8 : MT == 2 ? 4 : 2;       // as dense_skinny_kernel
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
  if constexpr (PRE) {
    // the wave's first batch of W (whole, or one unit of a shorter share) is in flight while
    // the block forms the statistics of x
    const int nb0 = u + UB <= wu1 ? UB : u < wu1 ? 1 : 0;
    bf16x8_t b0[UB][2];
#pragma unroll
    for (int i = 0; i < UB; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        b0[i][j] = (bf16x8_t){0, 0, 0, 0, 0, 0, 0, 0};
        if (i < nb0)
          b0[i][j] = *reinterpret_cast<const bf16x8_t*>(wp + (size_t)(u + i) * kUnit + 32 * j);
      }
    row_stats<4 * MT>(h, g.x, g.ldx, 0, g.M, w, lane, St);
    __syncthreads();
    float2 ms[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) ms[t] = live[t] ? St[16 * t + li] : make_float2(0.f, 0.f);
    const float* gp = h.ln_gamma + 8 * gq;
    const float* bp = h.ln_beta + 8 * gq;
    mma_units_ln<MT, UB>(b0, xp, live, ms, gp, bp, u, nb0, acc);
    u += nb0;
    for (; u + UB <= wu1; u += UB) {
      bf16x8_t b[UB][2];
      load_w<UB>(wp, u, b);
      mma_units_ln<MT, UB>(b, xp, live, ms, gp, bp, u, UB, acc);
    }
    for (; u < wu1; ++u) {
      bf16x8_t b[1][2];
      load_w<1>(wp, u, b);
      mma_units_ln<MT, 1>(b, xp, live, ms, gp, bp, u, 1, acc);
    }
  } else {
    for (; u + UB <= wu1; u += UB) run_units<MT, UB>(wp, xp, live, u, acc);
    for (; u < wu1; ++u) run_units<MT, 1>(wp, xp, live, u, acc);
  }
  mfma_fence();
  // the residual's statistics: published by the merge barrier below
  if constexpr (RES == 2)
    if (g.splits == 1) row_stats<4 * MT>(h, h.res, h.ldres, 0, g.M, w, lane, St);

  merge_waves<MT>(Ms, acc, tid, w, g.M, [&](int m, int c, float4 s) {
    if (g.splits == 1)
      store4_res<RES>(h, St, m, n0 + c, s);
    else
      *reinterpret_cast<float4*>(g.ws + ((size_t)split * g.M + m) * g.N + n0 + c) = s;
  });
}

// dense_skinny_combine_kernel with the residual; RES 2: the block first forms the statistics of
// the rows its 256 threads touch
template <int RES>
__global__ void __launch_bounds__(256) dense_skinny_combine_ln_kernel(const DenseSkinnyLnArgs h,
                                                                      int total) {
  const DenseSkinnyArgs& g = h.d;
  __shared__ float2 St[kMaxM];
  const int nq = g.N / 4;
  if constexpr (RES == 2) {
    const int first = blockIdx.x * 256;
    const int last = (first + 255 < total ? first + 255 : total - 1);
    row_stats<kMaxM / kWaves>(h, h.res, h.ldres, first / nq, last / nq + 1,
                              __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), threadIdx.x & 63,
                              St);
    __syncthreads();
  }
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int m = idx / nq, n = (idx % nq) * 4;
  const float* p = g.ws + (size_t)m * g.N + n;
  const size_t slab = (size_t)g.M * g.N;
  float4 s = *reinterpret_cast<const float4*>(p);
  for (int k = 1; k < g.splits; ++k) {
    const float4 q = *reinterpret_cast<const float4*>(p + k * slab);
    s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
  }
  store4_res<RES>(h, St, m, n, s);
}

template <bool PRE, int RES>
void launch_ln(const DenseSkinnyLnArgs& h, dim3 grid, hipStream_t st) {
  const dim3 block(64 * kWaves);
  switch ((h.d.M + 15) / 16) {
    case 1: hipLaunchKernelGGL((dense_skinny_ln_kernel<1, PRE, RES>), grid, block, 0, st, h); break;
    case 2: hipLaunchKernelGGL((dense_skinny_ln_kernel<2, PRE, RES>), grid, block, 0, st, h); break;
    case 3: hipLaunchKernelGGL((dense_skinny_ln_kernel<3, PRE, RES>), grid, block, 0, st, h); break;
    default: hipLaunchKernelGGL((dense_skinny_ln_kernel<4, PRE, RES>), grid, block, 0, st, h); break;
  }
}

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


// the checks common to every entry -> the `splits` of the launch
int dtf_dense_skinny_checked_splits(const bf16_t* x, const void* w, const float* bias,
                                    const bf16_t* y, const float* ws, int M, int N, int K, int ldx,
                                    int epi, int splits) {
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
  return splits;
}

void dtf_dense_skinny_combine(const DenseSkinnyLnArgs& h, int res, hipStream_t st) {
  const DenseSkinnyArgs& g = h.d;
  const int total = g.M * (g.N / 4);
  const dim3 cgrid(dtf_cdiv(total, 256)), cblock(256);
  if (res == 0)
    hipLaunchKernelGGL(dense_skinny_combine_kernel, cgrid, cblock, 0, st, g, total);
  else if (res == 1)
    hipLaunchKernelGGL(dense_skinny_combine_ln_kernel<1>, cgrid, cblock, 0, st, h, total);
  else
    hipLaunchKernelGGL(dense_skinny_combine_ln_kernel<2>, cgrid, cblock, 0, st, h, total);
}

void dtf_dense_skinny(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, float* ws,
                      int M, int N, int K, int ldx, int epi, int splits, hipStream_t st) {
  splits = dtf_dense_skinny_checked_splits(x, w, bias, y, ws, M, N, K, ldx, epi, splits);
  const DenseSkinnyArgs g{x, w, bias, y, ws, M, N, K, ldx, splits, epi};
  const dim3 grid(N / 16, splits), block(64 * kWaves);
  switch ((M + 15) / 16) {
    case 1: hipLaunchKernelGGL(dense_skinny_kernel<1>, grid, block, 0, st, g); break;
    case 2: hipLaunchKernelGGL(dense_skinny_kernel<2>, grid, block, 0, st, g); break;
    case 3: hipLaunchKernelGGL(dense_skinny_kernel<3>, grid, block, 0, st, g); break;
    default: hipLaunchKernelGGL(dense_skinny_kernel<4>, grid, block, 0, st, g); break;
  }
  if (splits > 1) dtf_dense_skinny_combine(DenseSkinnyLnArgs{g}, 0, st);
}

int dtf_dense_skinny_ln_max_width() { return kLnMaxWidth; }

int dtf_dense_skinny_ln_checked_res(const DenseSkinnyLnArgs& h) {
  const DenseSkinnyArgs& g = h.d;
  const bool ln = h.pre_ln || h.res_is_ln;
  if (!h.pre_ln && !h.res)
    throw std::runtime_error("dense_skinny_ln: neither a normalised x nor a residual: that is "
                             "dense_skinny");
  if (h.pre_ln && h.res_is_ln)
    throw std::runtime_error("dense_skinny_ln: x and the residual cannot both be normalised: a "
                             "call holds the row statistics of one matrix");
  if (h.res_is_ln && !h.res)
    throw std::runtime_error("dense_skinny_ln: a normalised residual needs the residual");
  if (h.res && g.epi != 1)
    throw std::runtime_error("dense_skinny_ln: the residual combines with the bias epilogue only "
                             "(epilogue 1), got " + std::to_string(g.epi));
  if (h.res && (h.ldres < g.N || h.ldres % 8 || (uintptr_t)h.res % 16))
    throw std::runtime_error("dense_skinny_ln: residual rows must start 16-B aligned (row stride " +
                             std::to_string(h.ldres) + " elements) and hold N elements");
  if (ln) {
    if (!h.ln_gamma || !h.ln_beta || ((uintptr_t)h.ln_gamma | (uintptr_t)h.ln_beta) % 16)
      throw std::runtime_error("dense_skinny_ln: gamma and beta must be 16-B aligned fp32");
    if (h.ln_width != (h.pre_ln ? g.K : g.N))
      throw std::runtime_error("dense_skinny_ln: the normalised rows are " +
                               std::to_string(h.pre_ln ? g.K : g.N) + " wide, got ln_width " +
                               std::to_string(h.ln_width));
    if (h.ln_width % 16 || h.ln_width > kLnMaxWidth)
      throw std::runtime_error("dense_skinny_ln: normalised rows must be a multiple of 16 and at "
                               "most " + std::to_string(kLnMaxWidth) + " wide, got " +
                               std::to_string(h.ln_width));
    if (!(h.ln_eps >= 0.f) || h.ln_eps > 1.f)
      throw std::runtime_error("dense_skinny_ln: eps must be in [0, 1]");
  }
  return !h.res ? 0 : h.res_is_ln ? 2 : 1;
}

void dtf_dense_skinny_ln(const DenseSkinnyLnArgs& a, hipStream_t st) {
  DenseSkinnyLnArgs h = a;
  DenseSkinnyArgs& g = h.d;
  g.splits = dtf_dense_skinny_checked_splits(g.x, g.w, g.bias, g.y, g.ws, g.M, g.N, g.K, g.ldx,
                                             g.epi, g.splits);
  const int res = dtf_dense_skinny_ln_checked_res(h);
  const dim3 grid(g.N / 16, g.splits);
  if (h.pre_ln) {
    if (res == 0) launch_ln<true, 0>(h, grid, st);
    else launch_ln<true, 1>(h, grid, st);
  } else {
    if (res == 1) launch_ln<false, 1>(h, grid, st);
    else launch_ln<false, 2>(h, grid, st);
  }
  if (g.splits > 1) dtf_dense_skinny_combine(h, res, st);
}
