// Dense bf16 GEMM on MFMA (gfx950): C[M, N] = A[M, K] . B[N, K]^T  (+ bias[N]) (ReLU) (+ Cin)
//
// The "NT" form -- both operands K-contiguous rows -- is what every dense layer of the framework
// needs: forward y = x W^T (W stored [out][in], the TF/BERT layout) and data gradient
// dx = dy W, with W^T staged once per step by the batched filter-transpose kernel (the weight
// gradient, a sum over tokens, is the conv_wgrad kernel's TN form).  SURVEY.md K8/K9/N-K4/N-K6.
//
// Tiling (cdna_hip_programming.md §5, "glds vs register staging" first row; §5.5 T1/T2/T5):
//   * 512 threads = 8 waves as 2 (M) x 4 (N); block tile 256 x 256, wave tile 128 x 64 built from
//     8 x 4 v_mfma_f32_16x16x32_bf16 fragments (16x16x32 holds a higher clock than 32x32x16 under
//     load: MI355X_MICROARCH.md "DVFS give-back" (7)); BK = 64.
//   * both tiles staged by LDS-DMA (buffer_load_dwordx4 ... lds: no staging VGPRs, no ds_write
//     pass), two 64-KB stages, the next K-step's DMAs issued before the current step's MFMAs;
//     one counted vmcnt + raw s_barrier per K-step (a __syncthreads() would drain the DMAs).
//   * the DMA writes a wave-instruction's 64 x 16 B lane-linearly, so the XOR chunk swizzle that
//     makes the 16-row ds_read_b128 fragment reads conflict-free is applied on the SOURCE side:
//     LDS slot s of row r receives source chunk s ^ ((r >> 1) & 7).
//   * rows past M and K-chunks past K get an out-of-range buffer offset: the hardware range check
//     returns zeros -- no branches, no padding copies.  Each block's buffer descriptors are based
//     at ITS first row (64-bit pointer arithmetic on the host side of the descriptor), so the
//     32-bit offsets only ever span one 256-row panel: tensors far beyond 2 GiB are fine.
//   * XCD-aware bijective block remap, N-tile fastest: blocks sharing an A panel share an L2.
//   * epilogue: accumulators (+bias, ReLU) -> bf16 -> LDS -> 16-B coalesced stores (+Cin: the
//     beta = 1 accumulation used to fold a residual gradient into a data-gradient GEMM).
//
// The default dispatch reaches gemm_nt_kernel as the 256 x 128 tile (variant 1; its conv form is
// the two-group SCHED 3) and the 256 x 256 ping-pong (variant 8), and the persistent
// gemm_pp2_kernel (variant 15).  Variant 13 is gemm_stream.hip.  Two more instantiations of code
// that those routes compile anyway stay behind gemm_set_variant as the references of
// tests/test_dense_gpu.py (test_gemm_pingpong_schedule_bit_identical):
//   * 0: 256 x 256 x 64, two LDS slots, one barrier per K-step (SCHED 0) -- the best of round 2's
//     first five forms at 0.80-0.91x hipBLASLt on the BERT shapes; the ping-pong gained 10-19 %
//     over it (profiles/measurements/r2_gemm_vs_hipblaslt.jsonl, r2_gemm_pingpong_setprio_ab.jsonl)
//   * 10: the two-group 256 x 128 schedule (SCHED 3) on dense operands: 0.95-1.07x of variant 1
//     on the ResNet 1x1 shapes and never made a route (r2_gemm_256x128_pingpong_resnet1x1.jsonl)
// gemm_set_variant keeps these numbers because the records under profiles/ use them.  What was
// tried, measured slower and deleted (the ids are what those records call them):
//   * 2, 3: BK 32 with a four-slot ring (256 x 256, 256 x 128): 0.88-1.00x and 0.75-0.83x of 0 on
//     the BERT shapes (r2_gemm_vs_hipblaslt.jsonl)
//   * 4: SCHED 1, fragments double-buffered in registers and the barrier moved between the two
//     32-deep halves of a step: 0.88-1.00x of 0 on the BERT shapes (r2_gemm_vs_hipblaslt.jsonl)
//   * 5, 6, 7: NW 4, four waves of 128 x 128 with the accumulators in AGPRs (SCHED 0, SCHED 1,
//     BK 32): 0.42-0.80x of the ping-pong -- one wave per SIMD leaves the matrix pipe idle during
//     barriers and LDS waits (r3_gemm_occ2_and_epilogue_split.jsonl "r3_gemm_nw4";
//     r3_gemm_4wave_vgpr_staged.jsonl for the VGPR-staged forms 14 / 15 of that round)
//   * 9: the ping-pong without s_setprio around its MFMA sections: within noise of 8
//     (r2_gemm_pingpong_setprio_ab.jsonl)
//   * 11: gemm_pp_kernel, round 3's persistent kernel with 8-B register-direct stores: bit-identical
//     to 8 but 0.86-1.03x of it -- the tile lookup, per-tile descriptors and conv geometry inside
//     every look-ahead issue spilled SGPRs on the ping-pong's load sections
//     (r3_gemm_persistent_register_epilogue.jsonl, r2_gemm_epilogue_probes.jsonl); gemm_pp2_kernel
//     is its design with that fixed
//   * 12: two 4-wave 256 x 128 blocks per CU (BK 32, three slots) with part of the first round
//     started late: bit-identical to 8 but 0.65-0.9x of it under every stagger policy
//     (r3_gemm_occ2_and_epilogue_split.jsonl)
#include <algorithm>
#include <stdexcept>
#include <string>

#include "launch.h"

namespace {

constexpr int kGT = 512;                     // threads (8 waves)
constexpr uint32_t kGOOB = 0xFFFFFFF0u;

struct GemmArgs {
  const bf16_t* A; const bf16_t* B; bf16_t* C;
  const float* bias;      // [N] fp32 or null
  const bf16_t* Cin;      // accumulate source ([M][ldc], may alias C) or null
  int M, N, K, lda, ldb, ldc;
  int relu;
  float* stats;           // BatchNorm partial sums of the bf16 outputs: [tiles_m][2][N] or null
  const bf16_t* acc_src;  // C += acc_src * relu_bit (a residual BN's masked dy; conv acc mode 2)
  const uint8_t* acc_mask;//   1 bit per element, 1 byte per 8 channels ([M][N] dense C only)
  // implicit-GEMM convolution (CONV kernels): A = the NHWC input X [N][H][W][C] read through a
  // tap table; row m = output pixel (n, p, q), K index = tap * C + channel (C % 64 == 0)
  int H, W, Cc, P, Q, sh, sw, ntaps;
  int tdh[9], tdw[9];
  // the persistent kernel's per-tap pair: [0] the byte offset of tap t from the receptive field's
  // corner, (dh W + dw) C 2; [1] its validity selector, bit (dh - dh0) | bit (8 + dw - dw0), with
  // dh0 / dw0 the smallest deltas of the table (the kernel takes tables spanning < 8 each way)
  int tsel[9][2];
  int dh0, dw0;
  int Ho, Wo, osh, osw, oh0, ow0;   // output rows: (n, p*osh + oh0, q*osw + ow0) of [N][Ho][Wo]
  int nt;                           // non-temporal C stores
  int dbg;                          // timing probes (tools/gemm_overhead.py): 1 = skip epilogue
  // GELU-backward epilogue (a data gradient feeding a GELU, BERT's FFN): C = acc * gelu'(a + b)
  // with a [M][ldc] the GELU's saved input and b [N] its bias; colsum [tiles_m][N] receives the
  // per-tile column sums of C in fp32 (the bias gradient's first level)
  const bf16_t* gelu_a;
  const float* gelu_b;
  float* colsum;
  // bias + GELU forward epilogue (BERT's first FFN GEMM): C = z = acc + bias (bf16) and
  // gelu_out = gelu(z), the pre-activation for the GELU backward and the activation for FFN2
  bf16_t* gelu_out;
  int a_bytes, b_bytes;             // gemm_pp2_kernel: the whole-operand descriptor sizes
  int group_m;                      // > 0: grouped tile order (GM M-panels x all N per group)
};

// chunk swizzle of a [rows][BK] bf16 tile: 16-row ds_read_b128 fragment reads hit 16 slots
template <int BK>
DTF_DEV int gswz(int row, int ch) {
  constexpr int CPR = BK / 8, RPB = 16 / CPR;
  return ch ^ ((row / RPB) % CPR);
}

// BM x BN block tile, BK-deep K-steps, NS-slot LDS ring (DMAs issued NS-1 steps ahead); 8 waves
// as 8 / (BN/64) (M) x BN/64 (N), 64-column wave tiles, 2 waves per SIMD.
template <int BM, int BN, int BK, int NS>
struct GCfg {
  static constexpr int NW = 8;
  static constexpr int NT = NW * 64;
  static constexpr int WN = BN / 64, WM = NW / WN;                 // wave grid
  static constexpr int WTM = BM / WM, WTN = BN / WN;               // wave tile
  static constexpr int FM = WTM / 16, FN = WTN / 16;               // 16x16 fragments per wave
  static constexpr int CPR = BK / 8;                       // 16-B chunks per row
  static constexpr int RPI = 64 / CPR;                     // rows per 1-KB DMA instruction
  static constexpr int DA = BM / RPI / NW, DB = BN / RPI / NW;   // DMAs per wave per stage
  static constexpr int SA = BM * BK, STAGE = (BM + BN) * BK;   // bf16 elements
  static constexpr int LDC = BN + 8;
  static constexpr size_t EPI = (size_t)BM * LDC * 2 + (size_t)WM * 2 * BN * 4;  // + stats
  static constexpr size_t LDS = (size_t)NS * STAGE * 2 > EPI ? (size_t)NS * STAGE * 2 : EPI;
};

// SCHED 0: per K-step {wait; barrier; issue next; reads + MFMAs of both 32-deep halves}.
// SCHED 2 / 3: the ping-pong schedules of the 256 x 256 / 256 x 128 tile (below).
template <int BM, int BN, int BK, int NS, int SCHED = 0, int CONV = 0>
__global__ void __launch_bounds__(kGT, 1)
gemm_nt_kernel(const GemmArgs g) {
  using Cf = GCfg<BM, BN, BK, NS>;
  constexpr int NW = Cf::NW;
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / Cf::WN, wn = wave % Cf::WN;

  const int tiles_n = (g.N + BN - 1) / BN;
  const int tiles_m = (g.M + BM - 1) / BM;
  const int bid = xcd_remap(blockIdx.x, tiles_n * tiles_m);
  // default order: N-tile fastest (consecutive blocks of an XCD share the A panel).  Grouped
  // (group_m = GM): within groups of GM M-panels the M index runs fastest, so the ~32 blocks an
  // XCD runs at once cover a GM x (32 / GM) patch of tiles -- fewer distinct A + B panels per
  // round than 32 / tiles_n x tiles_n when B (tiles_n panels) does not fit the XCD's L2.
  int tm, tn;
  if (g.group_m > 0) {
    const int per = g.group_m * tiles_n, grp = bid / per, first = grp * g.group_m;
    const int gm = min(g.group_m, tiles_m - first), r = bid - grp * per;
    tm = first + r % gm;
    tn = r / gm;
  } else {
    tm = bid / tiles_n;
    tn = bid % tiles_n;
  }
  const int m0 = tm * BM, n0 = tn * BN;
  const int nk = (g.K + BK - 1) / BK;

  // descriptors based at this block's first row / column: 32-bit offsets span one panel only
  const int rows_a = min(BM, g.M - m0), rows_b = min(BN, g.N - n0);
  // CONV: the A descriptor spans the input images this tile's output rows come from
  const int PQc = CONV ? g.P * g.Q : 1;
  const int n_lo = CONV ? m0 / PQc : 0;
  const long img = CONV ? (long)g.H * g.W * g.Cc : 0;
  const i32x4_t ra =
      CONV ? rsrc_quad(g.A + n_lo * img,
                       (uint32_t)(((m0 + rows_a - 1) / PQc - n_lo + 1) * img * 2))
           : rsrc_quad(g.A + (long)m0 * g.lda, (uint32_t)((long)(rows_a - 1) * g.lda + g.K) * 2u);
  const i32x4_t rb = rsrc_quad(g.B + (long)n0 * g.ldb, (uint32_t)((long)(rows_b - 1) * g.ldb + g.K) * 2u);
  const uint32_t lds0 = lds_addr(lds);

  // this wave fills DMA row-groups (RPI rows x BK) wave + 8 j of A, then of B
  const int lrow = lane / Cf::CPR, slot = lane % Cf::CPR;
  uint32_t a_off[Cf::DA], b_off[Cf::DB];
  int a_ch[Cf::DA], b_ch[Cf::DB];
#pragma unroll
  for (int j = 0; j < Cf::DA; ++j) {
    const int row = Cf::RPI * (wave + NW * j) + lrow;
    a_ch[j] = gswz<BK>(row, slot) * 8;
    a_off[j] = row < rows_a ? (uint32_t)(row * g.lda + a_ch[j]) * 2u : kGOOB;
  }
#pragma unroll
  for (int j = 0; j < Cf::DB; ++j) {
    const int row = Cf::RPI * (wave + NW * j) + lrow;
    b_ch[j] = gswz<BK>(row, slot) * 8;
    b_off[j] = row < rows_b ? (uint32_t)(row * g.ldb + b_ch[j]) * 2u : kGOOB;
  }

  // steps past the end are issued too, every lane out of range (no traffic): the number of
  // DMAs in flight behind each step is then a constant and the wait count a literal
  auto issue = [&](int kt, int stage) {
    const bool live = kt < nk;
    const int k0 = (live ? kt : 0) * BK;
    const uint32_t base = lds0 + (uint32_t)(stage * Cf::STAGE + wave * 512) * 2u;
#pragma unroll
    for (int j = 0; j < Cf::DA; ++j) {
      const bool ok = live && k0 + a_ch[j] < g.K && a_off[j] != kGOOB;
      dma16(ra, base + j * NW * 1024, ok ? a_off[j] + k0 * 2u : kGOOB);
    }
#pragma unroll
    for (int j = 0; j < Cf::DB; ++j) {
      const bool ok = live && k0 + b_ch[j] < g.K && b_off[j] != kGOOB;
      dma16(rb, base + Cf::SA * 2 + j * NW * 1024, ok ? b_off[j] + k0 * 2u : kGOOB);
    }
  };

  f32x4_t acc[Cf::FM][Cf::FN];
#pragma unroll
  for (int i = 0; i < Cf::FM; ++i)
#pragma unroll
    for (int j = 0; j < Cf::FN; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fq = lane >> 4;
  auto compute = [&](const bf16_t* sa) {
    const bf16_t* sb = sa + Cf::SA;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      bf16x8_t af[Cf::FM], bfr[Cf::FN];
      const int ch = ks * 4 + fq;
#pragma unroll
      for (int j = 0; j < Cf::FN; ++j) {
        const int r = wn * Cf::WTN + j * 16 + frow;
        bfr[j] = *reinterpret_cast<const bf16x8_t*>(sb + r * BK + gswz<BK>(r, ch) * 8);
      }
#pragma unroll
      for (int i = 0; i < Cf::FM; ++i) {
        const int r = wm * Cf::WTM + i * 16 + frow;
        af[i] = *reinterpret_cast<const bf16x8_t*>(sa + r * BK + gswz<BK>(r, ch) * 8);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < Cf::FM; ++i)
#pragma unroll
        for (int j = 0; j < Cf::FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  };

  if constexpr (SCHED == 2) {
    // Ping-pong schedule (cdna_hip_programming.md "256^2 8-phase template"; our own derivation):
    // every K-step is 4 phases, one per quadrant of the 128 x 64 wave tile (64 x 32 x K64 = 16
    // MFMAs).  Phase = {fragment reads | one 16-KB LDS-DMA piece (2 per thread) | counted vmcnt |
    // barrier | MFMAs | barrier}.  The wave rows (wm = 1) run ONE barrier behind the wm = 0
    // waves, so on every SIMD (one wave of each group) one wave is in its MFMA section while the
    // other reads LDS and issues DMAs -- the two barriers per phase enforce the alternation.
    //   reads:  q0: B-left + A-top   q1: B-right   q2: A-bottom   q3: -
    //   DMA pieces issued:  q0: (t+1).B-right  q1: (t+1).A-bottom  q2: (t+2).A-top  q3: (t+2).B-left
    // (reading the next step's B-left in q3 instead balances the reads 8/4/8/4 but costs 16
    // more VGPRs for a second B-left set and measured the same.)
    // RAW: a piece is waited (vmcnt(8): the 4 youngest pieces may fly) in the phase BEFORE the
    // one that reads it, ahead of that phase's first barrier -- with the one-barrier stagger
    // every reader then passes a barrier that follows every issuer's wait.  WAR: a region is
    // restaged >= 2 phases after its last read (reads retire by lgkmcnt(0) right after the
    // reading phase's first barrier).
    static_assert(BM == 256 && BN == 256 && BK == 64 && NS == 2, "SCHED 2 geometry");
    // piece p, instruction j: this wave's 8-row group (first row r0) of A top (p0) / B left (p1)
    // / B right (p2) / A bottom (p3)
    uint32_t poff[4][2], plds[4][2];
    int pch[4][2];
    // CONV: per A row (pieces 0 / 3) the input image base pixel and the top-left input (h, w)
    // of its receptive field; invalid rows get h far out of range
    int cpix[4][2], chw[4][2];
#pragma unroll
    for (int pc = 0; pc < 4; ++pc)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if constexpr (CONV) {
          if (pc == 0 || pc == 3) {
            const int r0c = pc == 0 ? j * 128 + 8 * wave : 64 + j * 128 + 8 * wave;
            const int m = m0 + r0c + lrow;
            const bool ok = m < g.M;
            const int mm = ok ? m : m0;
            const int q = mm % g.Q, t = mm / g.Q;
            const int p = t % g.P, n = t / g.P;
            cpix[pc][j] = (n - n_lo) * g.H * g.W;
            chw[pc][j] = ((ok ? p * g.sh : 0x7000) << 16) | (q * g.sw);   // invalid: h far out
          }
        }
        const bool isA = pc == 0 || pc == 3;
        const int r0 = pc == 0 ? j * 128 + 8 * wave
                     : pc == 3 ? 64 + j * 128 + 8 * wave
                               : (2 * j + (wave >> 2)) * 64 + (pc == 2 ? 32 : 0) + (wave & 3) * 8;
        const int row = r0 + lrow;
        const int ch = gswz<BK>(row, slot) * 8;   // the same for every piece (rows 8k + lrow)
        pch[pc][j] = ch;
        const int rows = isA ? rows_a : rows_b;
        const int ld = isA ? g.lda : g.ldb;
        // rows past the operand: offset 2^31, past every descriptor (the host keeps each panel
        // under 2^31 bytes), so "+ k0" stays out of range without a per-lane test
        poff[pc][j] = row < rows ? (uint32_t)(row * ld + ch) * 2u : 0x80000000u;
        plds[pc][j] = (uint32_t)((isA ? 0 : Cf::SA) + r0 * BK) * 2u;
      }
    const bool ktail = (g.K % BK) != 0;
    // steps past the end re-read step 0 into a slot nobody reads again (constant vmcnt counts)
    auto issue_piece = [&](int kt, int pc) {
      const bool live = kt < nk;
      const int k0 = (live ? kt : 0) * BK;
      const uint32_t base = lds0 + (uint32_t)((kt & 1) * Cf::STAGE) * 2u;
      if constexpr (CONV) {
        if (pc == 0 || pc == 3) {
          // K-step -> (tap, 64-channel block): wave-uniform
          const int cb = g.Cc / BK;
          const int tap = (live ? kt : 0) / cb, c0 = ((live ? kt : 0) % cb) * BK;
          const int dh = g.tdh[tap], dw = g.tdw[tap];
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int h = (chw[pc][j] >> 16) + dh, w = (chw[pc][j] & 0xFFFF) + dw;
            const bool ok = live && (unsigned)h < (unsigned)g.H && (unsigned)w < (unsigned)g.W;
            const uint32_t off =
                ok ? (uint32_t)(((cpix[pc][j] + h * g.W + w) * g.Cc + c0 + pch[0][0]) * 2) : kGOOB;
            dma16(ra, base + plds[pc][j], off);
          }
          return;
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        uint32_t off = poff[pc][j] + (uint32_t)k0 * 2u;
        if (ktail && k0 + pch[pc][j] >= g.K) off = kGOOB;
        dma16((pc == 0 || pc == 3) ? ra : rb, base + plds[pc][j], off);
      }
    };
    bf16x8_t fA[8], fBl[4], fBr[4];
    auto rdA = [&](const bf16_t* sa, int half) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = wm * 128 + half * 64 + i * 16 + frow, ch = ks * 4 + fq;
          fA[ks * 4 + i] = *reinterpret_cast<const bf16x8_t*>(sa + r * BK + gswz<BK>(r, ch) * 8);
        }
    };
    auto rdB = [&](bf16x8_t* fb, const bf16_t* sa, int half) {
      const bf16_t* sb = sa + Cf::SA;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int r = wn * 64 + half * 32 + j * 16 + frow, ch = ks * 4 + fq;
          fb[ks * 2 + j] = *reinterpret_cast<const bf16x8_t*>(sb + r * BK + gswz<BK>(r, ch) * 8);
        }
    };
    auto sync = [&]() {
      __builtin_amdgcn_sched_barrier(0);
      raw_barrier();
      __builtin_amdgcn_sched_barrier(0);
    };
    auto mfma_phase = [&](const bf16x8_t* fb, int ah, int bh) {
      sync();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[ah * 4 + i][bh * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                fA[ks * 4 + i], fb[ks * 2 + j], acc[ah * 4 + i][bh * 2 + j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      sync();
    };
    // prologue: step 0 whole + step 1's A-top / B-left; step 0's A-top / B-left landed
    issue_piece(0, 0); issue_piece(0, 1); issue_piece(0, 2); issue_piece(0, 3);
    issue_piece(1, 0); issue_piece(1, 1);
    DTF_WAIT_VM(8);
    sync();
    if (wm == 1) sync();                       // the one-barrier stagger
    for (int kt = 0; kt < nk; ++kt) {
      const bf16_t* cur = lds + (kt & 1) * Cf::STAGE;
      rdB(fBl, cur, 0);
      __builtin_amdgcn_sched_barrier(0);
      rdA(cur, 0);
      issue_piece(kt + 1, 2);
      DTF_WAIT_VM(8);
      mfma_phase(fBl, 0, 0);                   // q0: top x left
      rdB(fBr, cur, 1);
      issue_piece(kt + 1, 3);
      DTF_WAIT_VM(8);
      mfma_phase(fBr, 0, 1);                   // q1: top x right
      rdA(cur, 1);
      issue_piece(kt + 2, 0);
      DTF_WAIT_VM(8);
      mfma_phase(fBr, 1, 1);                   // q2: bottom x right
      issue_piece(kt + 2, 1);
      DTF_WAIT_VM(8);
      mfma_phase(fBl, 1, 0);                   // q3: bottom x left
    }
    if (wm == 0) sync();                       // re-align the barrier counts
  } else if constexpr (SCHED == 3) {
    // 256 x 128 ping-pong (N <= 128): 8 waves as 4 (M) x 2 (N) of 64 x 64, three 48-KB LDS
    // slots; each 64-deep K-step is 2 phases, one per 32-row half of the wave tile (2 x 4 x 2 =
    // 16 MFMAs), waves 4-7 one barrier behind waves 0-3 (one wave of each group per SIMD).
    //   reads:  q0: B + A-top   q1: A-bottom
    //   pieces issued in step t:  q0: (t+2).A-top + (t+2).B   q1: (t+2).A-bottom
    // RAW: A-top/B of step t+1 are waited (vmcnt(8)) in t.q1, A-bottom of step t (vmcnt(10))
    // in t.q0 -- always the phase before the reader.  WAR: step t+2 reuses step t-1's slot,
    // whose regions were last read 2 phases before they are restaged.
    static_assert(BM == 256 && BN == 128 && BK == 64 && NS == 3, "SCHED 3 geometry");
    const int grp = wave >> 2;
    uint32_t poff[3][2], plds[3][2];
    int pch[3][2], cpix[3][2], chw[3][2];
#pragma unroll
    for (int pc = 0; pc < 3; ++pc)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool isA = pc != 1;
        const int r0 = pc == 1 ? j * 64 + 8 * wave
                               : (2 * j + (wave >> 2)) * 64 + (pc == 2 ? 32 : 0) + (wave & 3) * 8;
        const int row = r0 + lrow;
        const int ch = gswz<BK>(row, slot) * 8;
        pch[pc][j] = ch;
        const int rows = isA ? rows_a : rows_b;
        const int ld = isA ? g.lda : g.ldb;
        poff[pc][j] = row < rows ? (uint32_t)(row * ld + ch) * 2u : 0x80000000u;
        plds[pc][j] = (uint32_t)((isA ? 0 : Cf::SA) + r0 * BK) * 2u;
        cpix[pc][j] = chw[pc][j] = 0;
        if constexpr (CONV) {
          if (isA) {
            const int m = m0 + row;
            const bool ok = m < g.M;
            const int mm = ok ? m : m0;
            const int q = mm % g.Q, t = mm / g.Q;
            const int p = t % g.P, n = t / g.P;
            cpix[pc][j] = (n - n_lo) * g.H * g.W;
            chw[pc][j] = ((ok ? p * g.sh : 0x7000) << 16) | (q * g.sw);
          }
        }
      }
    const bool ktail = (g.K % BK) != 0;
    auto issue_piece = [&](int kt, int pc) {
      const bool live = kt < nk;
      const int k0 = (live ? kt : 0) * BK;
      const uint32_t base = lds0 + (uint32_t)((kt % 3) * Cf::STAGE) * 2u;
      if constexpr (CONV) {
        if (pc != 1) {
          const int cb = g.Cc / BK;
          const int tap = (live ? kt : 0) / cb, c0 = ((live ? kt : 0) % cb) * BK;
          const int dh = g.tdh[tap], dw = g.tdw[tap];
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int h = (chw[pc][j] >> 16) + dh, w = (chw[pc][j] & 0xFFFF) + dw;
            const bool ok = live && (unsigned)h < (unsigned)g.H && (unsigned)w < (unsigned)g.W;
            const uint32_t off =
                ok ? (uint32_t)(((cpix[pc][j] + h * g.W + w) * g.Cc + c0 + pch[pc][j]) * 2) : kGOOB;
            dma16(ra, base + plds[pc][j], off);
          }
          return;
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        uint32_t off = poff[pc][j] + (uint32_t)k0 * 2u;
        if (ktail && k0 + pch[pc][j] >= g.K) off = kGOOB;
        dma16(pc != 1 ? ra : rb, base + plds[pc][j], off);
      }
    };
    bf16x8_t fA[4], fB[8];
    auto rdA = [&](const bf16_t* sa, int half) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int r = wm * 64 + half * 32 + i * 16 + frow, ch = ks * 4 + fq;
          fA[ks * 2 + i] = *reinterpret_cast<const bf16x8_t*>(sa + r * BK + gswz<BK>(r, ch) * 8);
        }
    };
    auto rdB = [&](const bf16_t* sa) {
      const bf16_t* sb = sa + Cf::SA;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = wn * 64 + j * 16 + frow, ch = ks * 4 + fq;
          fB[ks * 4 + j] = *reinterpret_cast<const bf16x8_t*>(sb + r * BK + gswz<BK>(r, ch) * 8);
        }
    };
    auto sync = [&]() {
      __builtin_amdgcn_sched_barrier(0);
      raw_barrier();
      __builtin_amdgcn_sched_barrier(0);
    };
    auto mfma_phase = [&](int half) {
      sync();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[half * 2 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                fA[ks * 2 + i], fB[ks * 4 + j], acc[half * 2 + i][j], 0, 0, 0);
      sync();
    };
    issue_piece(0, 0); issue_piece(0, 1); issue_piece(0, 2);
    issue_piece(1, 0); issue_piece(1, 1); issue_piece(1, 2);
    DTF_WAIT_VM(8);                            // step 0's A-top / B landed
    sync();
    if (grp == 1) sync();                      // the one-barrier stagger
    for (int kt = 0; kt < nk; ++kt) {
      const bf16_t* cur = lds + (kt % 3) * Cf::STAGE;
      rdB(cur);
      __builtin_amdgcn_sched_barrier(0);
      rdA(cur, 0);
      issue_piece(kt + 2, 0);
      issue_piece(kt + 2, 1);
      DTF_WAIT_VM(10);                         // this step's A-bottom landed
      mfma_phase(0);
      rdA(cur, 1);
      issue_piece(kt + 2, 2);
      DTF_WAIT_VM(8);                          // the next step's A-top / B landed
      mfma_phase(1);
    }
    if (grp == 0) sync();
  } else {
#pragma unroll
    for (int s = 0; s < NS - 1; ++s) issue(s, s);
    for (int kt = 0; kt < nk; ++kt) {
      // this wave's DMAs of step kt landed (the NS-2 younger steps may still fly) ...
      wait_vm<(NS - 2) * (Cf::DA + Cf::DB)>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      raw_barrier();    // ... and every wave's; every wave finished reading step kt-1's slot
      issue(kt + NS - 1, (kt + NS - 1) % NS);
      compute(lds + (kt % NS) * Cf::STAGE);
    }
  }
  DTF_WAIT_VM(0);       // the trailing no-op DMAs still target the ring
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  raw_barrier();        // all fragment reads done: reuse LDS for C
  if (g.dbg & 1) {      // timing probe: keep the accumulators live, skip staging and stores
    float keep = 0.f;
#pragma unroll
    for (int i = 0; i < Cf::FM; ++i)
#pragma unroll
      for (int j = 0; j < Cf::FN; ++j) keep += acc[i][j][0];
    if (keep == 1.2345f) g.C[tid] = 0;
    return;
  }

  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  float bj[Cf::FN];
#pragma unroll
  for (int j = 0; j < Cf::FN; ++j) {
    const int col = n0 + wn * Cf::WTN + j * 16 + frow;
    bj[j] = (g.bias && col < g.N) ? g.bias[col] : 0.f;
  }
  // BN statistics from the registers: each lane sums its column's bf16-rounded values over its
  // 4 * FM rows, then the 4 lane groups sharing a column (lanes l, l+16, l+32, l+48) combine
  // by cross-lane adds; the WM waves of a column meet in LDS after the staging barrier.  (A
  // pass over the staged tile instead costs ~128 LDS reads per thread -- exposed, since this
  // kernel runs one block per CU.)
  float s1[Cf::FN], s2[Cf::FN];
#pragma unroll
  for (int j = 0; j < Cf::FN; ++j) s1[j] = s2[j] = 0.f;
  const bool do_stats = g.stats != nullptr;
#pragma unroll
  for (int i = 0; i < Cf::FM; ++i)
#pragma unroll
    for (int j = 0; j < Cf::FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * Cf::WTM + i * 16 + fq * 4 + r;
        const int col = wn * Cf::WTN + j * 16 + frow;
        float v = acc[i][j][r] + bj[j];
        if (g.relu) v = fmaxf(v, 0.f);
        const bf16_t h = f2bf(v);
        lds[row * Cf::LDC + col] = h;
        if (do_stats && m0 + row < g.M) {
          const float q = bf2f(h);
          s1[j] += q;
          s2[j] += q * q;
        }
      }
  if (do_stats) {
#pragma unroll
    for (int j = 0; j < Cf::FN; ++j) {
      s1[j] += __shfl_xor(s1[j], 16, 64);
      s1[j] += __shfl_xor(s1[j], 32, 64);
      s2[j] += __shfl_xor(s2[j], 16, 64);
      s2[j] += __shfl_xor(s2[j], 32, 64);
    }
    float* red = reinterpret_cast<float*>(lds + BM * Cf::LDC);   // [WM][2][BN], past the tile
    if (fq == 0) {
#pragma unroll
      for (int j = 0; j < Cf::FN; ++j) {
        const int col = wn * Cf::WTN + j * 16 + frow;
        red[(wm * 2 + 0) * BN + col] = s1[j];
        red[(wm * 2 + 1) * BN + col] = s2[j];
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  raw_barrier();
  if (do_stats && tid < BN && n0 + tid < g.N) {
    const float* red = reinterpret_cast<const float*>(lds + BM * Cf::LDC);
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < Cf::WM; ++k) { a += red[(k * 2 + 0) * BN + tid]; b += red[(k * 2 + 1) * BN + tid]; }
    g.stats[((long)tm * 2 + 0) * g.N + n0 + tid] = a;
    g.stats[((long)tm * 2 + 1) * g.N + n0 + tid] = b;
  }
  constexpr int OCPR = BN / 8;                 // 16-B chunks per output row
  constexpr int OROWS = Cf::NT / OCPR;
  const int oc = tid % OCPR;
  const bool col_ok = n0 + oc * 8 < g.N;
  float gb[8], cs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    gb[e] = (g.gelu_b && col_ok) ? g.gelu_b[n0 + oc * 8 + e] : 0.f;
    cs[e] = 0.f;
  }
#pragma unroll 4
  for (int k = 0; k < BM / OROWS; ++k) {
    const int r = tid / OCPR + k * OROWS;
    if (!col_ok || m0 + r >= g.M) continue;
    uint4 v = *reinterpret_cast<const uint4*>(lds + r * Cf::LDC + oc * 8);
    long orow = m0 + r;
    if constexpr (CONV) {
      if (g.osh != 1 || g.osw != 1) {   // a data-gradient phase: pixel (n, p, q) of the phase grid
        const int m = m0 + r;
        const int q = m % g.Q, t = m / g.Q;
        const int p = t % g.P, n = t / g.P;
        orow = ((long)n * g.Ho + p * g.osh + g.oh0) * g.Wo + q * g.osw + g.ow0;
      }
    }
    const long off = orow * g.ldc + n0 + oc * 8;
    if (g.Cin) {
      float a[8], b[8];
      unpack8(v, a);
      unpack8(*reinterpret_cast<const uint4*>(g.Cin + off), b);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += b[e];
      v = pack8(a);
    } else if (g.acc_mask) {
      float a[8], b[8];
      unpack8(v, a);
      unpack8(*reinterpret_cast<const uint4*>(g.acc_src + off), b);
      const uint32_t mb = g.acc_mask[off >> 3];
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += (mb >> e) & 1u ? b[e] : 0.f;
      v = pack8(a);
    } else if (g.gelu_a) {
      float d[8], a[8];
      unpack8(v, d);
      unpack8(*reinterpret_cast<const uint4*>(g.gelu_a + off), a);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        d[e] *= gelu_grad(a[e] + gb[e]);
        cs[e] += d[e];
      }
      v = pack8(d);
    }
    st16(g.C + off, v, g.nt);
    if (g.gelu_out) {
      float z[8];
      unpack8(v, z);
#pragma unroll
      for (int e = 0; e < 8; ++e) z[e] = gelu_f(z[e]);
      st16(g.gelu_out + off, pack8(z), g.nt);
    }
  }
  if (g.colsum) {
    // the OROWS threads of a column chunk meet in LDS (the staged tile is dead after a barrier)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    float* red = reinterpret_cast<float*>(lds);                 // [OROWS][BN]
    const int rg = tid / OCPR;
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rg * BN + oc * 8 + e] = cs[e];
    __syncthreads();
    if (tid < BN && n0 + tid < g.N) {
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < OROWS; ++j) t += red[j * BN + tid];
      g.colsum[(long)tm * g.N + n0 + tid] = t;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Persistent ping-pong GEMM (gemm_pp2_kernel): one block per CU walking tiles (strided by the
// grid), the LDS-DMA piece stream running ACROSS tiles -- the K loop's look-ahead issues of
// "step nk, nk + 1" are the NEXT tile's steps 0 / 1, and the ring slot parity follows the block's
// global step count -- so the next tile's first pieces fly while this tile's outputs are stored
// straight from the registers (no LDS staging, no barrier), with a main loop that is
// instruction-for-instruction the per-tile SCHED 2 loop.  Its round-3 predecessor (variant 11 in
// the list at the top of this file) lost its main loop to the cross-tile issue path (tile lookup,
// two per-tile buffer descriptors and the CONV receptive-field geometry recomputed inside every
// look-ahead issue: SGPR spills on the ping-pong's critical load sections,
// profiles/measurements/r2_gemm_epilogue_probes.jsonl p1/p4).  Here
//   * the buffer descriptors span the WHOLE operands (host: < 2^31 bytes), built once;
//   * every piece's per-lane source offset (dense) or image pixel / receptive-field corner (CONV)
//     is computed ONCE per tile for the current AND the next tile; a look-ahead issue selects
//     between the two sets with a wave-uniform condition (v_cndmask), nothing else -- the CONV
//     form adds the K-step's scalar tap + channel offset, carried in a cursor per look-ahead
//     distance, and tests the tap's validity bits (no division, table load or bounds test in
//     the issue: profiles/CONV_GEMM_ISSUE.md);
//   * K % 64 == 0 (no K-tail test in the issue).
// Every lane issues the same number of stores per tile (out-of-range ones carry an offset past
// the C descriptor and are dropped by the hardware range check), so the counted vmcnt waits of
// the next tile's first phases know exactly how many stores sit behind the pieces they need.
// EPI bits (each instantiation carries only the epilogue operands it uses -- SGPR pressure):
// 1 BN statistics, 2 accumulate (Cin / masked acc), 4 strided (dgrad phase) output rows,
// 8 / 16 GELU forward / backward (below), 32 ReLU (a compile-time bit: as the runtime flag it
// cost a v_max + v_cndmask per output element in every epilogue, ReLU or not)
// TAP0 (probe builds only, wrong results): every CONV A piece reads tap 0 / channel block 0 --
// the issue path with no per-step state at all, the ceiling of what the tap cursors can reach
template <int CONV, int EPI, bool TAP0 = false>
__global__ void __launch_bounds__(512, 1)
gemm_pp2_kernel(const GemmArgs g) {
  using Cf = GCfg<256, 256, 64, 2>;
  constexpr int BM = 256, BN = 256, BK = 64;
  constexpr int NSTORE = Cf::FM * Cf::FN;          // 8-B stores per lane per tile (32)
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / Cf::WN, wn = wave % Cf::WN;
  const int tiles_n = (g.N + BN - 1) / BN, tiles_m = (g.M + BM - 1) / BM;
  const int ntiles = tiles_n * tiles_m;
  const int nk = g.K / BK;                         // >= 2, K % 64 == 0 (host)
  const uint32_t lds0 = lds_addr(lds);
  const int lrow = lane / Cf::CPR, slot = lane % Cf::CPR;
  const int frow = lane & 15, fq = lane >> 4;
  const int PQc = CONV ? g.P * g.Q : 1;
  constexpr bool strided = CONV && (EPI & 4);

  auto prow = [&](int pc, int j) {
    const int r0 = pc == 0 ? j * 128 + 8 * wave
                 : pc == 3 ? 64 + j * 128 + 8 * wave
                           : (2 * j + (wave >> 2)) * 64 + (pc == 2 ? 32 : 0) + (wave & 3) * 8;
    return r0 + lrow;
  };
  const int pch = gswz<BK>(prow(0, 0), slot) * 8;   // the same for every piece of this wave
  // ILV (the non-strided instantiations without BN statistics): the MFMA operands in their
  // natural order and the B rows INTERLEAVED over the wave's four 16-column fragments --
  // fragment jj's row f holds output column 4 f + jj of the wave's 64-column strip -- so lane
  // (frow, fq) ends up holding C[4 fq + r][4 frow .. 4 frow + 3] of each 16-row fragment: one
  // 8-B store per (fragment row, register) and 16 lanes cover 128 contiguous bytes of a row, i.e.
  // every store instruction writes four WHOLE 128-B lines (the swapped layout wrote 16 rows x
  // 32 B per instruction and completed a line only over four instructions 8 apart).  The K order
  // per output is unchanged: bit-identical to the swapped layout.
  // (round 6: the strided dgrad-phase rows too -- their output rows are addressed through a
  // per-wave LDS row table, see the epilogue -- so the swapped layout below is no longer used)
  constexpr bool ILV = true;
  auto plds = [&](int pc, int j) {
    const bool isA = pc == 0 || pc == 3;
    return (uint32_t)((isA ? 0 : Cf::SA) + (prow(pc, j) - lrow) * BK) * 2u;
  };
  // whole-operand descriptors (host: A / X and B below 2^31 bytes)
  const i32x4_t ra = rsrc_quad(g.A, (uint32_t)g.a_bytes);
  const i32x4_t rb = rsrc_quad(g.B, (uint32_t)g.b_bytes);

  auto tile_mn = [&](int seq, int& m0, int& n0) {
    const long phys = (long)blockIdx.x + (long)seq * gridDim.x;
    if (phys >= ntiles) { m0 = -1; n0 = 0; return false; }
    const int bid = xcd_remap((int)phys, ntiles);
    m0 = (bid / tiles_n) * BM;
    n0 = (bid % tiles_n) * BN;
    return true;
  };
  // per-tile piece operands: dense -> byte offset (2^31 = out of range); CONV A pieces -> per
  // row the byte offset of its receptive field's top-left corner (tap offsets, which may be
  // negative, are added to it mod 2^32) and, per piece, the two rows' validity bit fields (row
  // j at bits 16 j: bit i set when image row h0 + dh0 + i exists, bit 8 + i when image column
  // w0 + dw0 + i does; 0 for rows past M and for an invalid tile).  The K loop adds the step's
  // scalar (tap offset + channel offset) and tests the tap's two bits (GemmArgs::tsel): no
  // decode, no bounds test and no multiply per issue.
  auto tile_offsets = [&](bool valid, int m0, int n0, uint32_t (&o)[4][2], uint32_t (&pb)[2][2],
                          uint32_t (&pv)[2]) {
    if constexpr (CONV) pv[0] = pv[1] = 0u;
#pragma unroll
    for (int pc = 0; pc < 4; ++pc)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool isA = pc == 0 || pc == 3;
        const int row = prow(pc, j);
        if (isA) {
          const int m = m0 + row;
          const bool ok = valid && m < g.M;
          if constexpr (CONV) {
            const int mm = ok ? m : 0;
            const int q = mm % g.Q, t = mm / g.Q;
            const int p = t % g.P, n = t / g.P;
            const int h0 = p * g.sh, w0 = q * g.sw;
            pb[pc == 3][j] = (uint32_t)((((n * g.H + h0) * g.W + w0) * g.Cc + pch) * 2);
            // i in [lo, hi) of 0 .. 8 are inside the image: bits (1 << hi) - (1 << lo)
            const int hlo = min(max(-(h0 + g.dh0), 0), 8), hhi = min(max(g.H - (h0 + g.dh0), hlo), 8);
            const int wlo = min(max(-(w0 + g.dw0), 0), 8), whi = min(max(g.W - (w0 + g.dw0), wlo), 8);
            const uint32_t bits = ((1u << hhi) - (1u << hlo)) | ((1u << whi) - (1u << wlo)) << 8;
            pv[pc == 3] |= (ok ? bits : 0u) << (16 * j);
            o[pc][j] = 0x80000000u;
          } else {
            o[pc][j] = ok ? (uint32_t)(m * g.lda + pch) * 2u : 0x80000000u;
          }
        } else {
          // ILV: LDS row (half 32 + j 16 + f) of a wave's 64-row strip holds output column
          // 4 f + 2 half + j of the strip, so fragment (half, j) of the ping-pong reads covers
          // columns 4 f + jj -- the interleave lives in the DMA source rows; the LDS layout, the
          // swizzle and the pieces' row ranges (each phase's RAW waits) are the swapped kernel's
          const int rho = row & 63;
          const int nl = ILV ? (row & ~63) + 4 * (rho & 15) + 2 * (rho >> 5) + ((rho >> 4) & 1)
                             : row;
          const int n = n0 + nl;
          const bool ok = valid && n < g.N;
          o[pc][j] = ok ? (uint32_t)(n * g.ldb + pch) * 2u : 0x80000000u;
        }
      }
  };

  int seq = 0, cm0, cn0, xm0, xn0;
  if (!tile_mn(0, cm0, cn0)) return;
  bool nxt_valid = tile_mn(1, xm0, xn0);
  uint32_t ocur[4][2], onxt[4][2];
  uint32_t pbcur[2][2], pbnxt[2][2], pvcur[2], pvnxt[2];
  tile_offsets(true, cm0, cn0, ocur, pbcur, pvcur);
  tile_offsets(nxt_valid, xm0, xn0, onxt, pbnxt, pvnxt);
  int gstep0 = 0;

  // CONV: where a K-step's A pieces read, as wave-uniform carried state -- the tap, the channel
  // block's byte offset cs = c0 * 2, koff = tsel[tap][0] + cs and sel = tsel[tap][1].  One cursor
  // per look-ahead distance (steps kt + 1 and kt + 2), stepped once per K-step by add / compare /
  // select; the step after a tile's last is the next tile's step 0 (tap 0, cs 0).
  struct TapCur { int tap, cs; uint32_t koff, sel; };
  const int cc2 = CONV ? g.Cc * 2 : 0;
  auto cur_step = [&](TapCur& c) {
    if constexpr (TAP0) return;              // probe: every step reads tap 0, channel block 0
    c.cs += BK * 2;
    const bool wrap = c.cs == cc2;
    c.cs = wrap ? 0 : c.cs;
    c.tap += wrap ? 1 : 0;
    c.tap = c.tap == g.ntaps ? 0 : c.tap;
  };

  // piece pc of step kt of the current tile (kt >= nk: the next tile's step kt - nk); ac: the
  // step's cursor (CONV A pieces)
  auto issue_piece = [&](int kt, int pc, const TapCur& ac) {
    const bool nx = kt >= nk;
    const int kk = nx ? kt - nk : kt;
    const uint32_t base = lds0 + (uint32_t)(((gstep0 + kt) & 1) * Cf::STAGE) * 2u;
    const bool isA = pc == 0 || pc == 3;
    if constexpr (CONV) {
      if (isA) {
        const uint32_t v = nx ? pvnxt[pc == 3] : pvcur[pc == 3];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint32_t b = nx ? pbnxt[pc == 3][j] : pbcur[pc == 3][j];
          const uint32_t s = ac.sel << (16 * j);
          dma16(ra, base + plds(pc, j), (v & s) == s ? b + ac.koff : kGOOB);
        }
        return;
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t o = nx ? onxt[pc][j] : ocur[pc][j];
      dma16(isA ? ra : rb, base + plds(pc, j), o + (uint32_t)(kk * BK) * 2u);
    }
  };

  f32x4_t acc[Cf::FM][Cf::FN];
#pragma unroll
  for (int i = 0; i < Cf::FM; ++i)
#pragma unroll
    for (int j = 0; j < Cf::FN; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  bf16x8_t fA[8], fBl[4], fBr[4];
  auto rdA = [&](const bf16_t* sa, int half) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = wm * 128 + half * 64 + i * 16 + frow, ch = ks * 4 + fq;
        fA[ks * 4 + i] = *reinterpret_cast<const bf16x8_t*>(sa + r * BK + gswz<BK>(r, ch) * 8);
      }
  };
  auto rdB = [&](bf16x8_t* fb, const bf16_t* sa, int half) {
    const bf16_t* sb = sa + Cf::SA;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = wn * 64 + half * 32 + j * 16 + frow, ch = ks * 4 + fq;
        fb[ks * 2 + j] = *reinterpret_cast<const bf16x8_t*>(sb + r * BK + gswz<BK>(r, ch) * 8);
      }
  };
  auto sync = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    raw_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  auto mfma_phase = [&](const bf16x8_t* fb, int ah, int bh) {
    sync();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[ah * 4 + i][bh * 2 + j] = ILV
              ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(fA[ks * 4 + i], fb[ks * 2 + j],
                                                        acc[ah * 4 + i][bh * 2 + j], 0, 0, 0)
              : __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[ks * 2 + j], fA[ks * 4 + i],
                                                        acc[ah * 4 + i][bh * 2 + j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    sync();
  };

  float* red = reinterpret_cast<float*>(lds + 2 * Cf::STAGE);   // [WM][2][BN] past the ring
  // EPI 8: bias + GELU forward (C = z, gelu_out = gelu(z): two stores per row); EPI 16: GELU
  // backward (C = acc * gelu'(a + b) with the per-tile column sums into colsum)
  constexpr bool gelu_fwd = (EPI & 8) != 0, gelu_bwd = (EPI & 16) != 0;
  static_assert(!((gelu_fwd || gelu_bwd) && (EPI & 7)), "GELU epilogues are plain dense ones");
  // the first phases of a tile wait for pieces issued BEFORE the previous tile's stores: allow
  // those stores (32 per lane, 64 with the GELU output) plus the 8 younger pieces to fly
  // (vmcnt saturates at 63: with 64 stores the wait also drains 9 of them)
  auto wait_after_stores = [&]() {
    if constexpr (gelu_fwd) DTF_WAIT_VM(63);
    else DTF_WAIT_VM(40);
  };
  // EPI 0 (BERT's dense layers): C (+ bias) (+ ReLU) only -- the statistics / accumulate
  // operands and their SGPRs are compiled out
  constexpr bool do_stats = (EPI & 1) != 0;
  constexpr bool has_acc = (EPI & 2) != 0;
  constexpr bool relu = (EPI & 32) != 0;
  static_assert(!relu || !(EPI & (1 | 4 | 8 | 16)), "ReLU: the plain / accumulate dense epilogues");

  // c1 / c2: the cursors of steps kt + 1 / kt + 2 (nk >= 2: steps 0 and 1 are this tile's)
  TapCur c1{0, 0, 0u, 0u}, c2{0, 0, 0u, 0u};
  if constexpr (CONV) {
    c1.koff = (uint32_t)g.tsel[0][0];
    c1.sel = (uint32_t)g.tsel[0][1];
    issue_piece(0, 0, c1); issue_piece(0, 1, c1); issue_piece(0, 2, c1); issue_piece(0, 3, c1);
    cur_step(c1);
    c1.koff = (uint32_t)(g.tsel[c1.tap][0] + c1.cs);
    c1.sel = (uint32_t)g.tsel[c1.tap][1];
    c2 = c1;
  } else {
    issue_piece(0, 0, c1); issue_piece(0, 1, c1); issue_piece(0, 2, c1); issue_piece(0, 3, c1);
  }
  issue_piece(1, 0, c1); issue_piece(1, 1, c1);
  DTF_WAIT_VM(8);
  bool first = true;
  for (;; ++seq) {
    sync();
    if (wm == 1) sync();                       // the one-barrier stagger
    for (int kt = 0; kt < nk; ++kt) {
      const bf16_t* cur_lds = lds + ((gstep0 + kt) & 1) * Cf::STAGE;
      // step kt + 2's tap pair: the scalar load is issued here, two phases (each with its
      // lgkmcnt(0)) before the cursor takes it at the top of the third load section, where no
      // LDS read of that section has been issued yet
      int toff2 = 0, tsel2 = 0;
      if constexpr (CONV) {
        cur_step(c2);
        toff2 = g.tsel[c2.tap][0];
        tsel2 = g.tsel[c2.tap][1];
      }
      rdB(fBl, cur_lds, 0);
      __builtin_amdgcn_sched_barrier(0);
      rdA(cur_lds, 0);
      issue_piece(kt + 1, 2, c1);
      if (!first && kt == 0) wait_after_stores(); else DTF_WAIT_VM(8);
      mfma_phase(fBl, 0, 0);
      rdB(fBr, cur_lds, 1);
      issue_piece(kt + 1, 3, c1);
      if (!first && kt == 0) wait_after_stores(); else DTF_WAIT_VM(8);
      mfma_phase(fBr, 0, 1);
      if constexpr (CONV) {
        c2.koff = (uint32_t)(toff2 + c2.cs);
        c2.sel = (uint32_t)tsel2;
        __builtin_amdgcn_sched_barrier(0);
      }
      rdA(cur_lds, 1);
      issue_piece(kt + 2, 0, c2);
      DTF_WAIT_VM(8);
      mfma_phase(fBr, 1, 1);
      issue_piece(kt + 2, 1, c2);
      DTF_WAIT_VM(8);
      mfma_phase(fBl, 1, 0);
      c1 = c2;
    }
    if (wm == 0) sync();

    // ---- epilogue: lane (frow, fq) of fragment (i, j) holds C[m][n .. n + 3]
    const int n_lo = CONV ? cm0 / PQc : 0;
    const int rows_a = min(BM, g.M - cm0);
    long cbase;
    uint32_t cbytes;
    if (strided) {
      const int n_hi = (cm0 + rows_a - 1) / PQc;
      // opaque: as closed forms the image-size products are hoisted above the tile loop and
      // held (64-bit, spilled) across every K loop; here they cost three s_mul per tile
      int ho = g.Ho;
      asm volatile("" : "+s"(ho));
      cbase = (long)n_lo * ho * g.Wo * g.ldc;
      cbytes = (uint32_t)((long)(n_hi - n_lo + 1) * ho * g.Wo * g.ldc * 2);
    } else {
      cbase = (long)cm0 * g.ldc;
      cbytes = (uint32_t)(((long)(rows_a - 1) * g.ldc + g.N) * 2);
    }
    const __amdgpu_buffer_rsrc_t rc =
        __builtin_amdgcn_make_buffer_rsrc(g.C + cbase, 0, (int)cbytes, 0x00020000);
    const bool nt_store = g.nt != 0;
    typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
    if constexpr (ILV) {
      // lane (frow, fq), fragment row i, register r: C[m][ncol .. ncol + 3], m = 16 i + 4 fq + r
      const int ncol = cn0 + wn * 64 + 4 * frow;
      const bool col_ok = ncol < g.N;
      float b4[4] = {0.f, 0.f, 0.f, 0.f};
      // with BN statistics the host passes no bias and no ReLU (gemm_nt / gemm_conv): compiled out
      if (!do_stats && g.bias && col_ok) {
        const float4 bv = *reinterpret_cast<const float4*>(g.bias + ncol);
        b4[0] = bv.x; b4[1] = bv.y; b4[2] = bv.z; b4[3] = bv.w;
      }
      float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
      float gb4[4] = {0.f, 0.f, 0.f, 0.f};          // GELU backward: the GELU's bias
      if (gelu_bwd && g.gelu_b && col_ok) {
        const float4 bv = *reinterpret_cast<const float4*>(g.gelu_b + ncol);
        gb4[0] = bv.x; gb4[1] = bv.y; gb4[2] = bv.z; gb4[3] = bv.w;
      }
      const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(
          gelu_fwd ? (void*)(g.gelu_out + cbase) : gelu_bwd ? (void*)(g.gelu_a + cbase) : (void*)g.C,
          0, (gelu_fwd || gelu_bwd) ? (int)cbytes : 0, 0x00020000);
      // byte offset of this lane's element run, advanced one row at a time by an opaque VALU add
      // (as closed forms the compiler hoists 32 row offsets / row tests into SGPRs and spills).
      // Rows past M lie past the descriptor's end; a column past N starts at 2^31 (beyond any
      // C descriptor): the hardware range check drops those stores and zero-fills those loads.
      int vo = col_ok ? ((wm * 128 + fq * 4) * g.ldc + ncol) * 2 : (int)0x80000000u;
      const int ldc2 = g.ldc * 2;
      // strided (dgrad phase) rows: not uniformly spaced -- each wave decodes its 128 rows
      // (two per lane) into a private LDS table of byte offsets from cbase (2^31: no row), and the
      // stores / accumulate loads read 4 rows' offsets per fragment row with one ds_read_b128
      int* rtab = reinterpret_cast<int*>(red + Cf::WM * 2 * BN) + wave * 128;
      const int colb = col_ok ? ncol * 2 : (int)0x80000000u;
      if constexpr (strided) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int m = cm0 + wm * 128 + lane + 64 * t;
          int o = (int)0x80000000u;
          if (m < g.M) {
            const int q = m % g.Q, tt = m / g.Q;
            const int p = tt % g.P, n = tt / g.P;
            o = ((((n - n_lo) * g.Ho + p * g.osh + g.oh0) * g.Wo + q * g.osw + g.ow0) * g.ldc) * 2;
          }
          rtab[lane + 64 * t] = o;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's own table
      }
      auto rows4 = [&](int i) -> i32x4_t {        // strided: fragment row i's 4 row offsets
        return *reinterpret_cast<const i32x4_t*>(rtab + 16 * i + 4 * fq);
      };
      // accumulate operands (the unused one points at C with zero size); the strided rows
      // accumulate from Cin only (launcher), so their kernels carry no mask operands
      const bool masked = has_acc && !strided && !g.Cin;
      const __amdgpu_buffer_rsrc_t rcin = __builtin_amdgcn_make_buffer_rsrc(
          has_acc ? const_cast<bf16_t*>(masked ? g.acc_src + cbase : g.Cin + cbase) : g.C, 0,
          has_acc ? (int)cbytes : 0, 0x00020000);
      const __amdgpu_buffer_rsrc_t rmask = __builtin_amdgcn_make_buffer_rsrc(
          masked ? const_cast<uint8_t*>(g.acc_mask + (cbase >> 3)) : (uint8_t*)g.C,
          // exactly the mask bytes of the valid region (cbytes / 2 elements, 8 per byte): a
          // row past M must fall outside it (a +1 here let row M's first lanes read one byte past
          // the mask allocation -- a device fault when that byte was unmapped)
          0, masked ? (int)(cbytes / 16) : 0, 0x00020000);
      // the accumulate / GELU operands of fragment row i + 1 are loaded while row i is formed
      // (one fragment row = 4 output rows per lane): their latency hides under the conversions
      // and stores instead of stalling every row
      constexpr bool has_ld = has_acc || gelu_bwd;
      typedef uint32_t u32x2l_t __attribute__((ext_vector_type(2)));
      const __amdgpu_buffer_rsrc_t rld = gelu_bwd ? rg : rcin;
      const int mshift = ncol & 7;                     // ldc % 8 == 0: the same for every row
      u32x2l_t pa[4], pn[4];
      uint32_t pm[4], pmn[4];
      auto load_rows = [&](int vrow, int fi, u32x2l_t (&d)[4], uint32_t (&m)[4]) {
        i32x4_t t4 = {0, 0, 0, 0};
        if constexpr (strided) t4 = rows4(fi);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int o = strided ? (col_ok ? t4[r] + colb : (int)0x80000000u) : vrow + r * ldc2;
          d[r] = __builtin_bit_cast(u32x2l_t, __builtin_amdgcn_raw_buffer_load_b64(rld, o, 0, 0));
          m[r] = masked ? (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rmask, o >> 4, 0, 0) : 0u;
        }
      };
      if constexpr (has_ld) load_rows(vo, 0, pa, pm);
#pragma unroll
      for (int i = 0; i < Cf::FM; ++i) {
        if constexpr (has_ld) {
          if (i + 1 < Cf::FM) load_rows(vo + 16 * ldc2, i + 1, pn, pmn);
        }
        i32x4_t t4 = {0, 0, 0, 0};
        if constexpr (strided) t4 = rows4(i);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int vr = strided ? (col_ok ? t4[r] + colb : (int)0x80000000u) : vo + r * ldc2;
          bf16_t h[4];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            float v = acc[i][jj][r] + b4[jj];
            if (relu) v = fmaxf(v, 0.f);
            h[jj] = f2bf(v);
            // rows past M / columns past N hold exact zeros (zero-filled operands, no bias with
            // statistics: host), so they add nothing -- no per-row test (its 32 compare masks
            // would live in SGPRs)
            if (do_stats) {
              const float qv = bf2f(h[jj]);
              s1[jj] += qv;
              s2[jj] += qv * qv;
            }
          }
          if constexpr (has_acc) {
            const u32x2l_t sv = pa[r];
            const uint32_t bits = masked ? (pm[r] >> mshift) & 0xFu : 0xFu;
            const float sf[4] = {__builtin_bit_cast(float, sv.x << 16),
                                 __builtin_bit_cast(float, sv.x & 0xffff0000u),
                                 __builtin_bit_cast(float, sv.y << 16),
                                 __builtin_bit_cast(float, sv.y & 0xffff0000u)};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
              h[jj] = f2bf(bf2f(h[jj]) + ((bits >> jj) & 1u ? sf[jj] : 0.f));
          }
          if constexpr (gelu_bwd) {
            // d = bf16(acc) * gelu'(a + b) (the LDS-staged kernel's arithmetic: bit-identical);
            // its fp32 value feeds the column sums (rows past M: acc and a are zero-filled ... d
            // = 0 * gelu'(b): exact zero)
            const u32x2l_t av = pa[r];
            const float af[4] = {__builtin_bit_cast(float, av.x << 16),
                                 __builtin_bit_cast(float, av.x & 0xffff0000u),
                                 __builtin_bit_cast(float, av.y << 16),
                                 __builtin_bit_cast(float, av.y & 0xffff0000u)};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
              const float d = bf2f(h[jj]) * gelu_grad(af[jj] + gb4[jj]);
              s1[jj] += d;
              h[jj] = f2bf(d);
            }
          }
          const u32x2_t w = {(uint32_t)h[0] | ((uint32_t)h[1] << 16),
                             (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
          if (nt_store) __builtin_amdgcn_raw_buffer_store_b64(w, rc, vr, 0, 2);
          else __builtin_amdgcn_raw_buffer_store_b64(w, rc, vr, 0, 0);
          if constexpr (gelu_fwd) {
            bf16_t q[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) q[jj] = f2bf(gelu_f(bf2f(h[jj])));
            const u32x2_t wq = {(uint32_t)q[0] | ((uint32_t)q[1] << 16),
                                (uint32_t)q[2] | ((uint32_t)q[3] << 16)};
            if (nt_store) __builtin_amdgcn_raw_buffer_store_b64(wq, rg, vr, 0, 2);
            else __builtin_amdgcn_raw_buffer_store_b64(wq, rg, vr, 0, 0);
          }
        }
        asm volatile("v_add_u32 %0, %0, %1" : "+v"(vo) : "s"(16 * ldc2));
        if constexpr (has_ld) {
#pragma unroll
          for (int r = 0; r < 4; ++r) { pa[r] = pn[r]; pm[r] = pmn[r]; }
        }
        __builtin_amdgcn_sched_barrier(0);     // one fragment row at a time (register pressure)
      }
      if constexpr (gelu_bwd) {
        // per-tile column sums of d: lane groups by cross-lane adds, the two wave rows in LDS,
        // then one fp32 row of colsum per M tile
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          s1[jj] += __shfl_xor(s1[jj], 16, 64);
          s1[jj] += __shfl_xor(s1[jj], 32, 64);
        }
        if (fq == 0) {
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) red[wm * BN + wn * 64 + 4 * frow + jj] = s1[jj];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        raw_barrier();
        if (tid < BN && cn0 + tid < g.N) {
          float t = 0.f;
#pragma unroll
          for (int k = 0; k < Cf::WM; ++k) t += red[k * BN + tid];
          g.colsum[(long)(cm0 / BM) * g.N + cn0 + tid] = t;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        raw_barrier();
      }
      if (do_stats) {
        // the four lane groups of a column (lanes frow + 16 q) meet by cross-lane adds, the WM
        // waves of a column in LDS
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          s1[jj] += __shfl_xor(s1[jj], 16, 64);
          s1[jj] += __shfl_xor(s1[jj], 32, 64);
          s2[jj] += __shfl_xor(s2[jj], 16, 64);
          s2[jj] += __shfl_xor(s2[jj], 32, 64);
        }
        if (fq == 0) {
          const int col = wn * 64 + 4 * frow;
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            red[(wm * 2 + 0) * BN + col + jj] = s1[jj];
            red[(wm * 2 + 1) * BN + col + jj] = s2[jj];
          }
        }
      }
    } else {
    // element offset of row m from cbase (within the C descriptor: < 2^30), -1: no row
    int rowoff[Cf::FM];
#pragma unroll
    for (int i = 0; i < Cf::FM; ++i) {
      const int m = cm0 + wm * 128 + i * 16 + frow;
      int o = -1;
      if (m < g.M) {
        if (strided) {
          const int q = m % g.Q, t = m / g.Q;
          const int p = t % g.P, n = t / g.P;
          o = (((n - n_lo) * g.Ho + p * g.osh + g.oh0) * g.Wo + q * g.osw + g.ow0) * g.ldc;
        } else {
          o = (m - cm0) * g.ldc;
        }
      }
      rowoff[i] = o;
    }
#pragma unroll
    for (int j = 0; j < Cf::FN; ++j) {
      const int ncol = cn0 + wn * 64 + j * 16 + fq * 4;
      const bool col_ok = ncol < g.N;
      float b4[4] = {0.f, 0.f, 0.f, 0.f};
      if (g.bias && col_ok) {
        const float4 bv = *reinterpret_cast<const float4*>(g.bias + ncol);
        b4[0] = bv.x; b4[1] = bv.y; b4[2] = bv.z; b4[3] = bv.w;
      }
      float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < Cf::FM; ++i) {
        const bool ok = col_ok && rowoff[i] >= 0;
        float v[4];
        bf16_t h[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = acc[i][j][r] + b4[r];
          if (relu) v[r] = fmaxf(v[r], 0.f);
          h[r] = f2bf(v[r]);
          if (do_stats && ok) {
            const float qv = bf2f(h[r]);
            s1[r] += qv;
            s2[r] += qv * qv;
          }
        }
        const int eoff = rowoff[i] + ncol;
        if (has_acc && ok) {
          const bf16_t* src = g.Cin ? g.Cin + cbase + eoff : g.acc_src + cbase + eoff;
          const uint2 sv = *reinterpret_cast<const uint2*>(src);
          const uint32_t bits = g.Cin ? 0xFu
                                      : (g.acc_mask[(cbase + eoff) >> 3] >> ((cbase + eoff) & 7)) & 0xFu;
          const float sf[4] = {__builtin_bit_cast(float, sv.x << 16),
                               __builtin_bit_cast(float, sv.x & 0xffff0000u),
                               __builtin_bit_cast(float, sv.y << 16),
                               __builtin_bit_cast(float, sv.y & 0xffff0000u)};
#pragma unroll
          for (int r = 0; r < 4; ++r) h[r] = f2bf(bf2f(h[r]) + ((bits >> r) & 1u ? sf[r] : 0.f));
        }
        const u32x2_t w = {(uint32_t)h[0] | ((uint32_t)h[1] << 16),
                           (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
        const int so = ok ? eoff * 2 : (int)kGOOB;
        if (nt_store) __builtin_amdgcn_raw_buffer_store_b64(w, rc, so, 0, 2);
        else __builtin_amdgcn_raw_buffer_store_b64(w, rc, so, 0, 0);
      }
      if (do_stats) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) {
            s1[r] += __shfl_xor(s1[r], o, 64);
            s2[r] += __shfl_xor(s2[r], o, 64);
          }
        }
        if (frow == 0) {
          const int col = wn * 64 + j * 16 + fq * 4;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            red[(wm * 2 + 0) * BN + col + r] = s1[r];
            red[(wm * 2 + 1) * BN + col + r] = s2[r];
          }
        }
      }
    }
    }   // swapped layout
    if (do_stats) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      raw_barrier();
      if (tid < BN && cn0 + tid < g.N) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int k = 0; k < Cf::WM; ++k) { a += red[(k * 2 + 0) * BN + tid]; b += red[(k * 2 + 1) * BN + tid]; }
        const int tm = cm0 / BM;
        g.stats[((long)tm * 2 + 0) * g.N + cn0 + tid] = a;
        g.stats[((long)tm * 2 + 1) * g.N + cn0 + tid] = b;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      raw_barrier();
    }
    if (!nxt_valid) break;
#pragma unroll
    for (int i = 0; i < Cf::FM; ++i)
#pragma unroll
      for (int j = 0; j < Cf::FN; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    gstep0 += nk;
    cm0 = xm0;
    cn0 = xn0;
#pragma unroll
    for (int pc = 0; pc < 4; ++pc)
#pragma unroll
      for (int j = 0; j < 2; ++j) ocur[pc][j] = onxt[pc][j];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      pvcur[a] = pvnxt[a];
#pragma unroll
      for (int j = 0; j < 2; ++j) pbcur[a][j] = pbnxt[a][j];
    }
    nxt_valid = tile_mn(seq + 2, xm0, xn0);
    tile_offsets(nxt_valid, xm0, xn0, onxt, pbnxt, pvnxt);
    first = false;
    static_assert(NSTORE == 32, "the counted waits assume 32 stores per lane per tile");
  }
  DTF_WAIT_VM(0);       // the trailing look-ahead DMAs still target the ring
}

template <int CONV, int EPI, bool TAP0 = false>
void launch_gemm_pp2_t(const GemmArgs& g0, long a_bytes, long b_bytes, hipStream_t st) {
  using Cf = GCfg<256, 256, 64, 2>;
  // + the strided epilogue's per-wave row tables (8 waves x 128 ints)
  constexpr size_t LDS = (size_t)2 * Cf::STAGE * 2 + (size_t)Cf::WM * 2 * 256 * 4 +
                         ((EPI & 4) ? (size_t)8 * 128 * 4 : 0);
  static bool attr = false;
  static int ncu = 0;
  if (!attr) {
    HIP_CHECK(hipFuncSetAttribute((const void*)gemm_pp2_kernel<CONV, EPI, TAP0>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS));
    hipFuncAttributes fa{};
    HIP_CHECK(hipFuncGetAttributes(&fa, (const void*)gemm_pp2_kernel<CONV, EPI, TAP0>));
    if (fa.localSizeBytes > 0)
      throw std::runtime_error("gemm_pp2_kernel was compiled with register spills (scratch " +
                               std::to_string(fa.localSizeBytes) + " B/lane)");
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    attr = true;
  }
  if (a_bytes <= 0 || a_bytes >= 0x7FFFFF00L || b_bytes <= 0 || b_bytes >= 0x7FFFFF00L ||
      g0.K % 64 || g0.K < 128)
    throw std::runtime_error("gemm_pp2: operands below 2^31 bytes, K % 64 == 0, K >= 128");
  GemmArgs g = g0;
  g.a_bytes = (int)a_bytes;
  g.b_bytes = (int)b_bytes;
  const long tiles = (long)((g.M + 255) / 256) * ((g.N + 255) / 256);
  long grid = tiles < ncu ? tiles : (ncu / 8) * 8;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((gemm_pp2_kernel<CONV, EPI, TAP0>), dim3((unsigned)grid), dim3(Cf::NT), LDS,
                     st, g);
}

// one epilogue's instantiation; in a probe build GemmArgs::dbg bit 1 selects the CONV kernels'
// tap-0 timing probe (wrong results)
template <int CONV, int EPI>
void launch_gemm_pp2_e(const GemmArgs& g, long a_bytes, long b_bytes, hipStream_t st) {
#ifdef DTF_PROBES
  if (CONV && (g.dbg & 2)) {
    launch_gemm_pp2_t<CONV, EPI, CONV != 0>(g, a_bytes, b_bytes, st);
    return;
  }
#endif
  launch_gemm_pp2_t<CONV, EPI>(g, a_bytes, b_bytes, st);
}

template <int CONV>
void launch_gemm_pp2(const GemmArgs& g, long a_bytes, long b_bytes, hipStream_t st) {
  const bool stats = g.stats != nullptr, acc = g.Cin || g.acc_mask;
  const bool strided = CONV && (g.osh != 1 || g.osw != 1);
  if (g.relu && (CONV || stats || strided || g.gelu_out || g.gelu_a))
    throw std::runtime_error("gemm_pp2: ReLU only on the plain / accumulate dense epilogues");
  if (strided && acc && !g.Cin)
    throw std::runtime_error("gemm_pp2: strided output rows accumulate from Cin only");
  if constexpr (!CONV) {
    if (g.gelu_out) { launch_gemm_pp2_t<0, 8>(g, a_bytes, b_bytes, st); return; }
    if (g.gelu_a) { launch_gemm_pp2_t<0, 16>(g, a_bytes, b_bytes, st); return; }
    if (g.relu) {
      if (acc) launch_gemm_pp2_t<0, 34>(g, a_bytes, b_bytes, st);
      else launch_gemm_pp2_t<0, 32>(g, a_bytes, b_bytes, st);
      return;
    }
  }
  if constexpr (CONV) {
    if (strided) {
      if (acc) launch_gemm_pp2_e<CONV, 6>(g, a_bytes, b_bytes, st);
      else launch_gemm_pp2_e<CONV, 4>(g, a_bytes, b_bytes, st);
      return;
    }
  }
  if (stats) {
    launch_gemm_pp2_e<CONV, 1>(g, a_bytes, b_bytes, st);
  } else if (acc) {
    launch_gemm_pp2_e<CONV, 2>(g, a_bytes, b_bytes, st);
  } else {
    launch_gemm_pp2_e<CONV, 0>(g, a_bytes, b_bytes, st);
  }
}

// round-5 persistent kernel (gemm_pp2): bit 0 gemm_nt (0.92-1.05x hipBLASLt on the BERT shapes,
// profiles/measurements/r5_gemm_pp2_interleaved_epilogue_vs_v8.jsonl; ResNet-50 +0.6 %), bit 1 the
// unit-stride implicit-GEMM convs (2-5 % per layer, r5_conv_pp2_per_layer_b1984.jsonl)
int g_gemm_pp2 = 3;
// the strided data-gradient phases on gemm_pp2 too (round 6: their rows through an LDS row table
// in the interleaved full-line epilogue; round 5's swapped 32-B epilogue ran them 1.2-1.5x slower
// than the ping-pong kernel)
int g_gemm_pp2_strided = 1;
int g_gemm_stream = 1;     // output-heavy shapes on the row-streaming kernel (gemm_stream.hip)

int g_gemm_variant = -1;   // -1: auto, or one of 0, 1, 8, 10, 13, 15 (dtf_gemm_set_variant)
// non-temporal C stores: on since the persistent kernel's full-line stores (BERT-base b512 +1.1 %,
// profiles/measurements/r5_bert_gemm_nt_stores.jsonl); ResNet-50 A/B neutral in round 2
int g_gemm_nt = 1;
int g_gemm_dbg = 0;        // GemmArgs::dbg for timing probes
int g_gemm_group = 0;      // grouped tile order (GemmArgs::group_m) for the non-conv GEMMs

template <int BM, int BN, int BK, int NS, int SCHED = 0, int CONV = 0>
void launch_gemm(const GemmArgs& g0, hipStream_t st) {
  using Cf = GCfg<BM, BN, BK, NS>;
  static bool attr = false;
  if (!attr) {
    HIP_CHECK(hipFuncSetAttribute((const void*)gemm_nt_kernel<BM, BN, BK, NS, SCHED, CONV>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)Cf::LDS));
    attr = true;
  }
  GemmArgs g = g0;
  if (!CONV) g.group_m = g_gemm_group;
  const long tiles = (long)((g.M + BM - 1) / BM) * ((g.N + BN - 1) / BN);
  hipLaunchKernelGGL((gemm_nt_kernel<BM, BN, BK, NS, SCHED, CONV>), dim3((unsigned)tiles),
                     dim3(Cf::NT), Cf::LDS, st, g);
}

// the dense entry points' per-block descriptors span at most one 256-row panel
void check_dense_ld(const char* who, int K, int lda, int ldb) {
  if ((long)256 * lda * 2 + 2L * K >= (1L << 31) || (long)256 * ldb * 2 + 2L * K >= (1L << 31))
    throw std::runtime_error(std::string(who) + ": leading dimension too large");
}

// The dense entry points' route.  variant -1 (auto): 256 x 128 tiles when N <= 128 (measured
// 1.02-1.07x the 256 x 256 tile on the N = 128 ResNet 1x1 convs,
// profiles/measurements/r2_gemm_vs_conv_resnet1x1_b1280.jsonl), else the persistent kernel when
// it takes the shape and the entry's epilogue (pp2_epi), else the ping-pong; 0 / 1 / 8 / 10 / 15
// force one (0 and 10: the tests' reference schedules, see the top of this file).
void launch_dense(const char* who, const GemmArgs& g, int variant, bool pp2_epi, hipStream_t st) {
  const bool pp2_ok = dtf_gemm_pp2_ok(g.M, g.N, g.K, g.lda, g.ldb) && pp2_epi;
  if (variant < 0) variant = g.N <= 128 ? 1 : (g_gemm_pp2 & 1) && pp2_ok ? 15 : 8;
  switch (variant) {
    case 0: launch_gemm<256, 256, 64, 2>(g, st); break;
    case 1: launch_gemm<256, 128, 64, 3>(g, st); break;
    case 10: launch_gemm<256, 128, 64, 3, 3>(g, st); break;
    case 8: launch_gemm<256, 256, 64, 2, 2>(g, st); break;
    case 15:
      if (!pp2_ok)
        throw std::runtime_error(std::string(who) +
                                 ": shape not supported by the persistent kernel (variant 15)");
      launch_gemm_pp2<0>(g, (long)(g.M - 1) * g.lda * 2 + 2L * g.K,
                         (long)(g.N - 1) * g.ldb * 2 + 2L * g.K, st);
      break;
  }
}

}  // namespace

void dtf_gemm_set_variant(int v) {
  if (v != -1 && v != 0 && v != 1 && v != 8 && v != 10 && v != 13 && v != 15)
    throw std::runtime_error("gemm_set_variant: " + std::to_string(v) + " is no variant; -1 "
                             "(auto), 1 (256 x 128), 8 (ping-pong), 13 (row-streaming), 15 "
                             "(persistent), or the tests' references 0 and 10");
  g_gemm_variant = v;
}
void dtf_gemm_set_stream(int v) { g_gemm_stream = v; }
void dtf_gemm_set_pp2(int v) { g_gemm_pp2 = v; }
void dtf_gemm_set_pp2_strided(int v) { g_gemm_pp2_strided = v; }
int dtf_gemm_get_pp2() { return g_gemm_pp2; }
void dtf_gemm_set_nt(int v) { g_gemm_nt = v; }
void dtf_gemm_set_dbg(int v) { g_gemm_dbg = v; }
void dtf_gemm_set_group(int gm) { g_gemm_group = gm < 0 ? 0 : gm; }

// Implicit-GEMM convolution on the ping-pong GEMM: Y[M = N*P*Q][Kout] (+= Cin / masked acc)
// = X (through the tap table) . Wt[Kout][Kpad]^T, Kpad = taps * C, C % 64 == 0, <= 9 taps.
// Output row m = (n, p, q) lands at pixel (n, p*osh + oh0, q*osw + ow0) of [N][Ho][Wo] (the
// phase classes of a strided data gradient; forward convs: osh = 1, Ho = P).  BN statistics
// slab rows = dtf_gemm_tile_rows(M).
// images per part when a gemm-conv input exceeds one 32-bit buffer descriptor: a multiple of
// 256 / gcd(P Q, 256) images (whole 256-row tiles) whose input stays under 2^31 bytes; 0 when no
// split is needed, -1 when none exists
int dtf_gemm_conv_part_images(int N, int H, int W, int C, int P, int Q) {
  const long img = (long)H * W * C * 2;
  if ((long)N * img < 0x7FFFFF00L) return 0;
  long a = (long)P * Q, b = 256;
  while (b) { const long t = a % b; a = b; b = t; }
  const long unit = 256 / a;
  const long per = (0x7FFFFF00L / img) / unit * unit;
  return per >= 1 && per < N && N < 2048 && H < 1000 && W < 1000 ? (int)per : -1;
}

void dtf_gemm_conv(const bf16_t* X, const bf16_t* Wt, bf16_t* Y, int N, int H, int W, int C,
                   int P, int Q, int sh, int sw, int Kout, int ntaps, const int* dh, const int* dw,
                   int Ho, int Wo, int osh, int osw, int oh0, int ow0,
                   float* stats, const bf16_t* Cin, const bf16_t* acc_src,
                   const uint8_t* acc_mask, hipStream_t st) {
  if (C % 64 || Kout % 8 || ntaps < 1 || ntaps > 9 || H >= 16384 || W >= 32768)
    throw std::runtime_error("gemm_conv: C % 64, Kout % 8, 1..9 taps, H < 2^14, W < 2^15");
  const long M = (long)N * P * Q;
  if (M >= (1L << 31) || 2.0 * H * W * C * (256.0 / (P * Q) + 2) >= 2147483647.0)
    throw std::runtime_error("gemm_conv: tile span too large for 32-bit buffer offsets");
  GemmArgs g{};
  g.A = X; g.B = Wt; g.C = Y; g.Cin = Cin; g.stats = stats; g.acc_src = acc_src;
  g.acc_mask = acc_mask;
  g.M = (int)M; g.N = Kout; g.K = ntaps * C; g.lda = C; g.ldb = ntaps * C; g.ldc = Kout;
  g.H = H; g.W = W; g.Cc = C; g.P = P; g.Q = Q; g.sh = sh; g.sw = sw; g.ntaps = ntaps;
  g.dh0 = *std::min_element(dh, dh + ntaps);
  g.dw0 = *std::min_element(dw, dw + ntaps);
  bool tap_span = true;              // the persistent kernel: 8 validity bits each way per row
  for (int t = 0; t < ntaps; ++t) {
    g.tdh[t] = dh[t]; g.tdw[t] = dw[t];
    tap_span = tap_span && dh[t] - g.dh0 < 8 && dw[t] - g.dw0 < 8;
    g.tsel[t][0] = (int)(((long)dh[t] * W + dw[t]) * C * 2);   // added mod 2^32 in the kernel
    g.tsel[t][1] = tap_span ? 1 << (dh[t] - g.dh0) | 1 << (8 + dw[t] - g.dw0) : 0;
  }
  g.Ho = Ho; g.Wo = Wo; g.osh = osh; g.osw = osw; g.oh0 = oh0; g.ow0 = ow0;
  g.nt = g_gemm_nt;
  g.dbg = g_gemm_dbg & 2;          // probe builds: the persistent kernel's tap-0 probe
  if ((osh != 1 || osw != 1) && (stats || acc_mask))
    throw std::runtime_error("gemm_conv: strided outputs take no BN statistics / masked acc");
  if ((long)256 * g.ldb * 2 + 2L * g.K >= (1L << 31))
    throw std::runtime_error("gemm_conv: filter too large");
  const bool pp_span = !(osh != 1 || osw != 1) ||
      (256.0 / (P * Q) + 2) * Ho * Wo * (double)Kout * 2 < 2147483647.0;
  const long x_bytes = (long)N * H * W * C * 2, w_bytes = (long)Kout * g.ldb * 2;
  // an input past one 32-bit descriptor (the stage-1 projection shortcut at b1984 reads a 3.2 GB
  // tensor) on the persistent kernel: the batch in parts of a whole number of 256-row tiles, so
  // the BN statistics slab rows of the parts continue exactly as one launch's would
  const int part_n = dtf_gemm_conv_part_images(N, H, W, C, P, Q);
  if (part_n > 0 && part_n < N && Kout > 128 && osh == 1 && osw == 1 && !Cin && !acc_src &&
      (g_gemm_pp2 & 2)) {
    const long pq = (long)P * Q;
    for (int n0 = 0; n0 < N; n0 += part_n) {
      const int cnt = std::min(part_n, N - n0);
      dtf_gemm_conv(X + (long)n0 * H * W * C, Wt, Y + (long)n0 * pq * Kout, cnt, H, W, C, P, Q, sh,
                    sw, Kout, ntaps, dh, dw, Ho, Wo, osh, osw, oh0, ow0,
                    stats ? stats + (long)n0 * pq / 256 * 2 * Kout : nullptr, nullptr, nullptr,
                    nullptr, st);
    }
    return;
  }
  if (Kout <= 128) launch_gemm<256, 128, 64, 3, 3, 1>(g, st);
  // the persistent kernel where it takes the launch (whole operands and the strided phases' image
  // span below 2^31 bytes, taps within 8 of each other): the unit-stride convs gain 2-5 % on it
  // (profiles/measurements/r5_conv_pp2_per_layer_b1984.jsonl), and the strided data-gradient
  // phases run on it too since their rows go through the epilogue's LDS row table
  // (g_gemm_pp2_strided)
  else if ((g_gemm_pp2 & 2) && (g_gemm_pp2_strided || (osh == 1 && osw == 1)) && g.K >= 128 &&
           x_bytes < 0x7FFFFF00L && w_bytes < 0x7FFFFF00L && N < 2048 && H < 1000 && W < 1000 &&
           pp_span && tap_span)
    launch_gemm_pp2<1>(g, x_bytes, w_bytes, st);
  else launch_gemm<256, 256, 64, 2, 2, 1>(g, st);
}

// dX = dY . W (gemm_nt form, B = W^T rows) for a data gradient that feeds a GELU: the epilogue
// applies gelu'(a + b) and leaves the per-tile column sums of the result (the GELU bias's
// gradient, first level) in colsum [dtf_gemm_tile_rows(M)][N]; C and a dense [M][N].
void dtf_gemm_nt_gelu_bwd(const bf16_t* A, const bf16_t* B, bf16_t* C, int M, int N, int K,
                          int lda, int ldb, const bf16_t* gelu_a, const float* gelu_b,
                          float* colsum, hipStream_t st) {
  if (M <= 0 || N <= 0 || K <= 0) return;
  if (K % 8 || N % 8 || lda % 8 || ldb % 8 || lda < K || ldb < K || !gelu_a || !colsum)
    throw std::runtime_error("gemm_nt_gelu_bwd: K, N, leading dims % 8; gelu_a and colsum needed");
  check_dense_ld("gemm_nt_gelu_bwd", K, lda, ldb);
  GemmArgs g{};
  g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = N;
  g.gelu_a = gelu_a; g.gelu_b = gelu_b; g.colsum = colsum;
  g.nt = g_gemm_nt;
  launch_dense("gemm_nt_gelu_bwd", g, -1, true, st);
}

// Z = A . B^T + bias (bf16) and H = gelu(Z) in one pass (BERT's first FFN GEMM: replaces a
// library GEMM + the bias_gelu_fwd pass that re-read its output)
void dtf_gemm_nt_bias_gelu(const bf16_t* A, const bf16_t* B, bf16_t* Z, bf16_t* H, int M, int N,
                           int K, int lda, int ldb, const float* bias, hipStream_t st) {
  if (M <= 0 || N <= 0 || K <= 0) return;
  if (K % 8 || N % 8 || lda % 8 || ldb % 8 || lda < K || ldb < K || !bias || !H)
    throw std::runtime_error("gemm_nt_bias_gelu: K, N, leading dims % 8; bias and H needed");
  check_dense_ld("gemm_nt_bias_gelu", K, lda, ldb);
  GemmArgs g{};
  g.A = A; g.B = B; g.C = Z; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = N;
  g.bias = bias; g.gelu_out = H;
  g.nt = g_gemm_nt;
  launch_dense("gemm_nt_bias_gelu", g, -1, true, st);
}

// the persistent kernel gemm_pp2 takes this dense GEMM: K % 64 == 0, K >= 128, whole operands
// addressable with 32-bit buffer offsets
bool dtf_gemm_pp2_ok(int M, int N, int K, int lda, int ldb) {
  return K % 64 == 0 && K >= 128 && (long)(M - 1) * lda * 2 + 2L * K < 0x7FFFFF00L &&
         (long)(N - 1) * ldb * 2 + 2L * K < 0x7FFFFF00L;
}

// block-tile rows of every variant (the BatchNorm statistics slab has one row per M tile)
int dtf_gemm_tile_rows(int M) { return (M + 255) / 256; }

void dtf_gemm_nt(const bf16_t* A, const bf16_t* B, bf16_t* C, int M, int N, int K, int lda,
                 int ldb, int ldc, const float* bias, const bf16_t* Cin, int relu, float* stats,
                 hipStream_t st, const bf16_t* acc_src, const uint8_t* acc_mask) {
  if (M <= 0 || N <= 0 || K <= 0) return;
  if (K % 8 || N % 8 || lda % 8 || ldb % 8 || ldc % 8 || lda < K || ldb < K || ldc < N)
    throw std::runtime_error("gemm_nt: K, N and the leading dimensions must be multiples of 8");
  check_dense_ld("gemm_nt", K, lda, ldb);
  if (stats && (bias || relu || Cin))
    throw std::runtime_error("gemm_nt: BN statistics epilogue excludes bias / ReLU / accumulate");
  if (acc_mask && (!acc_src || Cin || ldc != N))
    throw std::runtime_error("gemm_nt: masked accumulation needs acc_src and a dense C");
  // short K, output at least as wide (N >= K): the row-streaming kernel overlaps each 64-column
  // chunk's stores with the next chunk's MFMAs (gemm_stream.hip); no bias / ReLU epilogue there
  const bool stream_ok = !bias && !relu && (stats ? 1 : 0) + (Cin ? 1 : 0) +
      (acc_mask ? 1 : 0) <= 1 && dtf_gemm_stream_ok(M, N, K, lda, ldb, ldc);
  if (g_gemm_variant == 13 || (g_gemm_variant < 0 && g_gemm_stream && stream_ok && N >= K)) {
    if (!stream_ok) throw std::runtime_error("gemm_nt: shape not supported by variant 13");
    dtf_gemm_stream(A, B, C, M, N, K, lda, ldb, ldc, Cin, stats, acc_src, acc_mask, g_gemm_nt, st);
    return;
  }
  GemmArgs g{A, B, C, bias, Cin, M, N, K, lda, ldb, ldc, relu, stats, acc_src, acc_mask};
  g.nt = g_gemm_nt;
  g.dbg = g_gemm_dbg;
  launch_dense("gemm_nt", g, g_gemm_variant, !(stats && (bias || relu)), st);
}
