// Append attention for the causal model: T new tokens per sequence against a per-sequence cache
// of keys and values -- the shape between the causal forward (S queries against the same S keys)
// and the decode kernel (one query against the cache).  Chunked prefill, extending a conversation
// and scoring drafted tokens all run here.
//
// Cache layout as in attn_decode.hip: k_cache / v_cache are bf16 [B, H, C, 64], C % 64 == 0.
//
// dtf_attn_append, per row b, everything read ON THE DEVICE:
//   p0 = clamp(pos[b], 0, C),  n = clamp(n_new ? n_new[b] : T, 0, min(T, C - p0));
//   1. cache rows p0 .. p0 + n - 1 take the K / V of new tokens 0 .. n - 1 (kv_cache_append_kernel,
//      bit for bit; nothing else is written);
//   2. query i < n attends keys 0 .. p0 + i: out = softmax2(q . K^T * scale * log2 e) V, rounded
//      once to bf16; output rows i >= n are exactly zero.
//
// Design.
//   * The copy runs FIRST, as its own launch on the same stream: the attention kernel then reads
//     keys and values only from the cache (the new rows are warm in L2) and no launch reads what it
//     writes.  The decode kernel's trick -- the new row kept in registers -- does not scale to T
//     rows, several query blocks and splits.
//   * MFMA: one wave owns a 16-query x 64-key tile as attn_fwd_kernel does -- Q in registers as
//     the B operand of S^T = K Q^T, K rows from LDS as the A operand, P packed to bf16 in
//     registers as the B operand of O^T = V^T P^T, V read transposed by ds_read_tr16_b64.
//   * Work split.  A block has 4 waves and stages 64-key K / V tiles from the contiguous 128-B
//     cache rows into LDS (pitch 72).  How the waves are dealt depends on T:
//       QT = 4 (T > 16): 4 query tiles x 1 key sub-tile.  One 64-key tile is staged per step and
//         serves all 64 queries of the block: the cache is streamed once per 64 queries.
//       QT = 1 (T <= 16): 1 query tile x 4 key sub-tiles.  Four tiles (256 keys) are staged per
//         step and wave w takes sub-tile w, so a drafted-token call keeps all four waves busy.
//     Either way each wave leaves (acc[16][64], m[16], l[16]) in LDS (over the staging area) and
//     the block merges the KS waves of a query tile IN WAVE ORDER -- for QT = 4 that is a plain
//     pass-through, one epilogue serves both.
//   * Grid (splits x query blocks, H, B).  A block's keys are the tiles 0 .. (p0 + its last live
//     query) / 64 of ITS row, cut into `splits` contiguous ranges as the decode kernel cuts them;
//     splits == 1 writes out directly, otherwise fp32 partials [acc[64], m, l, pad 2] go to the
//     workspace [B, H, T, splits, 68] and attn_append_combine_kernel merges them IN SPLIT ORDER.
//     No atomics, no counters: the same inputs and `splits` give the same bits.
//   * A wave skips a tile that starts above its last live query (wave-uniform; there is no
//     barrier inside the skipped part); the block's loop ends at its last live query's tile.
//   * Unlike its two neighbours this kernel meets query rows with NO visible key in a tile, a
//     wave's share or a split (the diagonal crosses a 64-key boundary inside a wave's 16 queries;
//     rows i >= n; empty splits).  So every rescale and merge weight is merge_weight(): a select
//     that gives 0 for m = -inf, never exp2(-inf - -inf); p is formed against a maximum that a
//     select has made finite; and the final 1 / l of a row that saw nothing is a select to 0.
//   * Cache rows >= p0 + n may hold anything, NaN bit patterns included.  A hidden score is
//     SELECTED to -inf (copes with NaN in K), but P V is an MFMA and 0 x NaN is NaN, so K and V rows
//     >= p0 + n are zero-filled on the way into LDS (they are never loaded).
//   * Query lanes >= T load nothing (zeros) and store nothing.
//   * The FP8 cache (dtf_attn_append_f8; format and helpers in kv_f8.h) is the template parameter
//     F8 of the same kernel.  Its copy quantises (kv_cache_append_f8_kernel); its staging loads 16
//     bytes and the row's scale and writes their 16 exactly dequantised bf16 into the same LDS
//     tile (half the global traffic, half the staging steps).  From LDS on nothing differs, so it
//     computes the bf16 kernel's function of the dequantised cache.
#include <stdexcept>
#include <string>

#include "kv_f8.h"
#include "launch.h"

namespace {

constexpr int kHd = 64;          // head dim
constexpr int kTile = 64;        // keys per tile
constexpr int kWaves = 4;        // waves per block
constexpr int kLd = 72;          // LDS row pitch in elements (144 B), as nlp.hip
constexpr int kWsRow = 68;       // acc[64], m, l, 2 pad: 272-B rows take 16-B stores
constexpr float kNegInf = -__builtin_inff();

typedef __attribute__((ext_vector_type(4))) short s4_t;
typedef __attribute__((address_space(3))) s4_t lds_s4_t;

// the fragment helpers of nlp.hip (see there for the operand layouts)
DTF_DEV bf16x8_t lds_row8(const bf16_t* base, int row, int col) {
  return *(const bf16x8_t*)(base + row * kLd + col);
}
DTF_DEV bf16x8_t lds_tr8(const bf16_t* base, int row0, int col0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const bf16_t* p = base + (row0 + 4 * g + (i >> 2)) * kLd + col0 + 4 * (i & 3);
  const s4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(p));
  const s4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(p + 16 * kLd));
  return (bf16x8_t){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
DTF_DEV bf16x8_t pack_frag(const f32x4_t& x0, const f32x4_t& x1) {
  return (bf16x8_t){(short)f2bf(x0[0]), (short)f2bf(x0[1]), (short)f2bf(x0[2]), (short)f2bf(x0[3]),
                    (short)f2bf(x1[0]), (short)f2bf(x1[1]), (short)f2bf(x1[2]), (short)f2bf(x1[3])};
}
DTF_DEV f32x4_t mfma(const bf16x8_t& a, const bf16x8_t& b, const f32x4_t& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
DTF_DEV void mfma_fence() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 7\n\ts_nop 7" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
// weight of a partial with maximum m in a merge whose maximum is M: an empty partial (m = -inf)
// weighs exactly 0, also when M is -inf
DTF_DEV float merge_weight(float m, float M) {
  return m == kNegInf ? 0.f : __builtin_amdgcn_exp2f(m - M);
}

// the row's first free cache row and the number of new tokens it takes
DTF_DEV void row_extent(const AttnAppendArgs& g, int b, int& p0, int& n) {
  p0 = min(max(g.pos[b], 0), g.C);
  n = min(max(g.n_new ? g.n_new[b] : g.T, 0), min(g.T, g.C - p0));
}

// The K and V thirds of new tokens 0 .. n - 1 of qkv_new [B*T, 3*H*64] into cache rows p0 + t.
// One thread per 16-B chunk, chunk-fastest then head then token, as kv_cache_fill_kernel.
__global__ void __launch_bounds__(256) kv_cache_append_kernel(const AttnAppendArgs g, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int sub = (int)(idx & 7);
  long r = idx >> 3;
  const int h = (int)(r % g.H);
  r /= g.H;
  const int t = (int)(r % g.T);
  r /= g.T;
  const int b = (int)(r % g.B);
  const int which = (int)(r / g.B);                       // 0: K, 1: V
  int p0, n;
  row_extent(g, b, p0, n);
  if (t >= n) return;
  const long HD = (long)g.H * kHd;
  const bf16_t* src = g.qkv_new + ((long)b * g.T + t) * 3 * HD + (1 + which) * HD + h * kHd + sub * 8;
  bf16_t* dst = (which ? g.v_cache : g.k_cache) + (((long)b * g.H + h) * g.C + p0 + t) * kHd + sub * 8;
  *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
}

// The same copy into an FP8 cache (kv_f8.h): one thread per 16 output bytes (32 B of bf16 in), the
// row maximum over the 4 lanes of a row by shuffles, then the scale, then the bytes.  A row's 4
// lanes share t and b, so they leave together; rows outside p0 .. p0 + n - 1 and their scales are
// not touched.
__global__ void __launch_bounds__(256) kv_cache_append_f8_kernel(const AttnAppendArgs g, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int sub = (int)(idx & 3);
  long r = idx >> 2;
  const int h = (int)(r % g.H);
  r /= g.H;
  const int t = (int)(r % g.T);
  r /= g.T;
  const int b = (int)(r % g.B);
  const int which = (int)(r / g.B);                       // 0: K, 1: V
  int p0, n;
  row_extent(g, b, p0, n);
  if (t >= n) return;
  const long HD = (long)g.H * kHd;
  const bf16_t* src = g.qkv_new + ((long)b * g.T + t) * 3 * HD + (1 + which) * HD + h * kHd + sub * 16;
  const uint4 lo = *reinterpret_cast<const uint4*>(src);
  const uint4 hi = *reinterpret_cast<const uint4*>(src + 8);
  const int e = kv_f8_exponent(kv_f8_group4_max(max(kv_f8_absmax8(lo), kv_f8_absmax8(hi))));
  const long row = ((long)b * g.H + h) * g.C + p0 + t;
  uint8_t* dst = reinterpret_cast<uint8_t*>(which ? g.v_cache : g.k_cache) + row * kHd + sub * 16;
  *reinterpret_cast<uint4*>(dst) = kv_f8_quantize16(lo, hi, kv_f8_pow2(-e));
  if (sub == 0) (which ? g.v_scale : g.k_scale)[row] = kv_f8_pow2(e);
}

// F8: the caches are e4m3 bytes with one scale per row (kv_f8.h); only the staging differs -- a
// thread's 16 bytes are dequantised, exactly, to the 16 bf16 the bf16 cache would hold.
template <int QT, bool F8>
__global__ void __launch_bounds__(64 * kWaves) attn_append_kernel(const AttnAppendArgs g) {
  constexpr int KS = kWaves / QT;                         // 64-key sub-tiles per staged chunk
  constexpr int CH = kTile * KS;                          // keys per staged chunk
  static_assert(2 * CH * kLd * sizeof(bf16_t) >= kWaves * 16 * kWsRow * sizeof(float),
                "the merge area lies over the staging area");
  extern __shared__ __attribute__((aligned(16))) bf16_t sm[];
  bf16_t* Ks = sm;
  bf16_t* Vs = sm + CH * kLd;
  float* Ms = reinterpret_cast<float*>(sm);               // [wave][16 queries][kWsRow], after the loop
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, gq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qt = w % QT, ks = w / QT;                     // the wave's query tile and key sub-tile
  const int split = blockIdx.x % g.splits, qb = blockIdx.x / g.splits;
  const int h = blockIdx.y, b = blockIdx.z;
  int p0, n;
  row_extent(g, b, p0, n);
  const int q0 = qb * 16 * QT;                            // the block's first query
  const int qlast = min(n, q0 + 16 * QT) - 1;             // its last live one (< q0: none)
  const int ntiles = qlast >= q0 ? (p0 + qlast) / kTile + 1 : 0;
  const int t0 = (int)((long)split * ntiles / g.splits);
  const int t1 = (int)((long)(split + 1) * ntiles / g.splits);
  const int kend = min(p0 + n, t1 * kTile);               // rows at or past it are staged as zeros
  const int qw0 = q0 + 16 * qt;                           // the wave's first query
  const int qwl = min(n, qw0 + 16) - 1;                   // its last live one (< qw0: none)
  const int q = qw0 + li;
  const bool live = q < n;
  const long HD = (long)g.H * kHd;

  bf16x8_t bq0 = {0, 0, 0, 0, 0, 0, 0, 0}, bq1 = bq0;
  if (q < g.T) {
    const bf16_t* qrow = g.qkv_new + ((long)b * g.T + q) * 3 * HD + h * kHd;
    bq0 = *(const bf16x8_t*)(qrow + 8 * gq);
    bq1 = *(const bf16x8_t*)(qrow + 32 + 8 * gq);
  }
  const long base = ((long)b * g.H + h) * g.C * kHd;
  const bf16_t* kc = g.k_cache + base;
  const bf16_t* vc = g.v_cache + base;

  float m = kNegInf, l = 0.f;
  f32x4_t acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) acc[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  for (int tc = t0; tc < t1; tc += KS) {
    __syncthreads();
    if constexpr (F8) {
      // CH rows x 64 B of K and of V: 16 B (16 values) per thread and step, 16 whole rows per wave
      // instruction, and the row's scale (the 4 lanes of a row read the same word)
      const long bh = (long)b * g.H + h;
#pragma unroll
      for (int i = 0; i < 2 * CH * 4 / (64 * kWaves); ++i) {
        const int v = tid + 64 * kWaves * i;
        const int sel = v / (CH * 4), row = (v >> 2) % CH, cc = (v & 3) * 16;
        const int key = tc * kTile + row;
        uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
        if (key < kend) {
          const uint8_t* c8 = reinterpret_cast<const uint8_t*>(sel ? g.v_cache : g.k_cache);
          const uint4 x = *reinterpret_cast<const uint4*>(c8 + (bh * g.C + key) * kHd + cc);
          kv_f8_dequantize16(x, (sel ? g.v_scale : g.k_scale)[bh * g.C + key], lo, hi);
        }
        bf16_t* d = (sel ? Vs : Ks) + row * kLd + cc;
        *reinterpret_cast<uint4*>(d) = lo;
        *reinterpret_cast<uint4*>(d + 8) = hi;
      }
    } else {
      // CH rows x 128 B of K and of V: 16 B per thread and step, 8 whole rows per wave instruction
#pragma unroll
      for (int i = 0; i < 2 * CH * 8 / (64 * kWaves); ++i) {
        const int v = tid + 64 * kWaves * i;
        const int sel = v / (CH * 8), row = (v >> 3) % CH, cc = (v & 7) * 8;
        const int key = tc * kTile + row;
        uint4 x = make_uint4(0, 0, 0, 0);
        if (key < kend) x = *reinterpret_cast<const uint4*>((sel ? vc : kc) + (long)key * kHd + cc);
        *reinterpret_cast<uint4*>((sel ? Vs : Ks) + row * kLd + cc) = x;
      }
    }
    __syncthreads();
    const int tile = tc + ks;
    // wave-uniform: past the split's range, no live query, or the tile starts above the last one
    if (tile >= t1 || qwl < qw0 || tile * kTile > p0 + qwl) continue;
    const bf16_t* Kb = Ks + ks * kTile * kLd;
    const bf16_t* Vb = Vs + ks * kTile * kLd;
    f32x4_t s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
      s[t] = mfma(lds_row8(Kb, 16 * t + li, 8 * gq), bq0, s[t]);
      s[t] = mfma(lds_row8(Kb, 16 * t + li, 32 + 8 * gq), bq1, s[t]);
    }
    mfma_fence();
    // every key of the tile visible to every query of the wave: no selects
    const bool full = tile * kTile + kTile - 1 <= p0 + qw0 && qw0 + 15 <= qwl;
    const int vis = live ? p0 + q - tile * kTile : -1;    // keys of the tile at or below it are seen
    float mloc = kNegInf;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float x = s[t][r] * g.c;
        if (!full && 16 * t + 4 * gq + r > vis) x = kNegInf;
        s[t][r] = x;
        mloc = fmaxf(mloc, x);
      }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    const float mnew = fmaxf(m, mloc);
    // a row that has seen no key so far keeps m = -inf: its p are exp2(-inf - 0) = 0, not NaN
    const float mref = mnew == kNegInf ? 0.f : mnew;
    const float alpha = merge_weight(m, mnew);
    l *= alpha;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) acc[dt] *= alpha;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(s[t][r] - mref);
        l += p;
        s[t][r] = p;
      }
    const bf16x8_t bp0 = pack_frag(s[0], s[1]);
    const bf16x8_t bp1 = pack_frag(s[2], s[3]);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      acc[dt] = mfma(lds_tr8(Vb, 0, 16 * dt, lane), bp0, acc[dt]);
      acc[dt] = mfma(lds_tr8(Vb, 32, 16 * dt, lane), bp1, acc[dt]);
    }
    m = mnew;
  }
  mfma_fence();
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);

  // every wave leaves its 16 rows in LDS; the staging area is free once all waves are here
  __syncthreads();
  float* mine = Ms + (w * 16 + li) * kWsRow;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *reinterpret_cast<float4*>(mine + 16 * dt + 4 * gq) =
        make_float4(acc[dt][0], acc[dt][1], acc[dt][2], acc[dt][3]);
  if (gq == 0) *reinterpret_cast<float2*>(mine + 64) = make_float2(m, l);
  __syncthreads();

  // thread -> (query, 4 head dims): the KS waves of the query's tile merged in wave order
#pragma unroll
  for (int it = 0; it < QT; ++it) {
    const int item = tid + 64 * kWaves * it;
    const int qi = item >> 4, dc = item & 15;
    const int qq = q0 + qi;
    if (qq >= g.T) continue;
    const float* rows = Ms + ((qi >> 4) * 16 + (qi & 15)) * kWsRow;   // wave ks * QT + (qi >> 4)
    float M = kNegInf;
#pragma unroll
    for (int k = 0; k < KS; ++k) M = fmaxf(M, rows[k * QT * 16 * kWsRow + 64]);
    float L = 0.f;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < KS; ++k) {
      const float* r = rows + k * QT * 16 * kWsRow;
      const float f = merge_weight(r[64], M);
      const float4 a = *reinterpret_cast<const float4*>(r + 4 * dc);
      L = __builtin_fmaf(r[65], f, L);
      A.x = __builtin_fmaf(a.x, f, A.x);
      A.y = __builtin_fmaf(a.y, f, A.y);
      A.z = __builtin_fmaf(a.z, f, A.z);
      A.w = __builtin_fmaf(a.w, f, A.w);
    }
    if (g.splits == 1) {
      const float inv = L > 0.f ? 1.f / L : 0.f;           // a row that saw nothing: zeros
      bf16_t* o = g.out + ((long)b * g.T + qq) * HD + h * kHd + 4 * dc;
      *reinterpret_cast<uint2*>(o) = make_uint2(pack2(A.x * inv, A.y * inv), pack2(A.z * inv, A.w * inv));
    } else {
      float* ws = g.ws + ((((long)b * g.H + h) * g.T + qq) * g.splits + split) * kWsRow;
      *reinterpret_cast<float4*>(ws + 4 * dc) = A;
      if (dc == 0) *reinterpret_cast<float2*>(ws + 64) = make_float2(M, L);
    }
  }
}

// One thread per (b, h, query, 4 head dims): the partials of the splits merged in split order.
__global__ void __launch_bounds__(256) attn_append_combine_kernel(const AttnAppendArgs g, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int dc = (int)(idx & 15);
  const long row = idx >> 4;                               // (b H + h) T + q
  const int qq = (int)(row % g.T);
  const long bh = row / g.T;
  const float* ws = g.ws + row * g.splits * kWsRow;
  float M = kNegInf;
  for (int s = 0; s < g.splits; ++s) M = fmaxf(M, ws[s * kWsRow + 64]);
  float L = 0.f;
  float4 A = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < g.splits; ++s) {
    const float* r = ws + s * kWsRow;
    const float2 ml = *reinterpret_cast<const float2*>(r + 64);
    const float f = merge_weight(ml.x, M);
    const float4 a = *reinterpret_cast<const float4*>(r + 4 * dc);
    L = __builtin_fmaf(ml.y, f, L);
    A.x = __builtin_fmaf(a.x, f, A.x);
    A.y = __builtin_fmaf(a.y, f, A.y);
    A.z = __builtin_fmaf(a.z, f, A.z);
    A.w = __builtin_fmaf(a.w, f, A.w);
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;
  const long b = bh / g.H, h = bh % g.H;
  bf16_t* o = g.out + (b * g.T + qq) * (long)g.H * kHd + h * kHd + 4 * dc;
  *reinterpret_cast<uint2*>(o) = make_uint2(pack2(A.x * inv, A.y * inv), pack2(A.z * inv, A.w * inv));
}

constexpr int kCus = 256;            // MI355X
// A split must be worth the combine launch: no split below this many 64-key tiles -- one staged
// chunk of the T <= 16 kernel.  Measured at B = 1, H = 12 (tools/attn_bench.py --append, medians,
// profiles/APPEND.md): at 2 tiles (len 128) two splits lose, 14.2 us against 12.0; at 8 tiles
// (len 512) two splits of 4 tiles win, 13.9 against 15.6 (T = 8) and 17.4 against 22.1 (T = 64);
// at 32 tiles (len 2048) 8 splits of 4 tiles take 19.8 us against 41.5 for 2 and 71.0 for 1.
// The decode kernel's 8 (a call of ~8 us) is too coarse here: a tile costs this kernel more
// (LDS staging, a barrier pair) and the call's floor is two launches, ~11 us.
constexpr int kMinSplitTiles = 4;
constexpr int kMaxSplits = 64;
constexpr int kSmallT = 16;          // up to here: one query tile, four key sub-tiles per block

int tiles_of(int len) { return (len + kTile - 1) / kTile; }
int query_blocks(int T) { return T <= kSmallT ? 1 : (T + 63) / 64; }

template <int QT, bool F8>
void launch_append(const AttnAppendArgs& g, int nqb, hipStream_t st) {
  constexpr int kLds = 2 * kTile * (kWaves / QT) * kLd * (int)sizeof(bf16_t);
  if constexpr (kLds > 64 * 1024) {
    static bool once = false;
    if (!once) {
      HIP_CHECK(hipFuncSetAttribute((const void*)attn_append_kernel<QT, F8>,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
      once = true;
    }
  }
  hipLaunchKernelGGL((attn_append_kernel<QT, F8>), dim3(g.splits * nqb, g.H, g.B),
                     dim3(64 * kWaves), kLds, st, g);
}

}  // namespace

// `splits` for a launch: enough blocks for two per CU, but no split below kMinSplitTiles tiles.
// A pure function of (B * H * query blocks, max_len).
int dtf_attn_append_splits(int B, int H, int T, int max_len) {
  if (B < 1 || H < 1 || T < 1 || max_len < 1)
    throw std::runtime_error("attn_append_splits: B, H, T, max_len >= 1");
  const long blocks = (long)B * H * query_blocks(T);
  long want = (2 * kCus + blocks - 1) / blocks;
  const long cap = tiles_of(max_len) / kMinSplitTiles;
  if (want > cap) want = cap;
  if (want > kMaxSplits) want = kMaxSplits;
  if (want <= 1) return 1;
  // the fewest splits with the same longest range: at 32 tiles 6 splits of 5 or 6 tiles took
  // 38.5 us where 4 of 8 took 29.1 (B = 8, T = 8) -- both are two 4-tile steps of the T <= 16 kernel
  const long chunks = cap, per = (chunks + want - 1) / want;
  return (int)((chunks + per - 1) / per);
}

long dtf_attn_append_ws_floats(int B, int H, int T, int splits) {
  return splits > 1 ? (long)B * H * T * splits * kWsRow : 0;
}

namespace {

// F8: k_cache / v_cache point at e4m3 bytes and the scales are set
template <bool F8>
void append_any(const char* name, const bf16_t* qkv_new, const int* pos, const int* n_new,
                void* k_cache, void* v_cache, float* k_scale, float* v_scale, bf16_t* out,
                float* ws, int B, int T, int H, int C, int max_len, int splits, float scale,
                hipStream_t st) {
  const std::string nm(name);
  if (!qkv_new || !pos || !k_cache || !v_cache || !out || (F8 && (!k_scale || !v_scale)))
    throw std::runtime_error(nm + ": null pointer");
  if (B < 1 || H < 1 || B > 65535 || H > 65535)
    throw std::runtime_error(nm + ": 1 <= B, H <= 65535");
  if (C < kTile || C % kTile)
    throw std::runtime_error(nm + ": cache capacity must be a multiple of 64, at least 64");
  if (T < 1) throw std::runtime_error(nm + ": at least one new token per row (T >= 1)");
  if (max_len < T || max_len > C)
    throw std::runtime_error(nm + ": T <= max_len <= capacity");
  if (splits == 0) splits = dtf_attn_append_splits(B, H, T, max_len);
  if (splits < 1 || splits > tiles_of(max_len))
    throw std::runtime_error(nm + ": splits " + std::to_string(splits) + " exceeds the " +
                             std::to_string(tiles_of(max_len)) + " tiles of max_len");
  if (splits > 1 && !ws) throw std::runtime_error(nm + ": splits > 1 needs the workspace");
  const AttnAppendArgs g{qkv_new, pos, n_new, static_cast<bf16_t*>(k_cache),
                         static_cast<bf16_t*>(v_cache), out, ws, B, T, H, C, splits,
                         scale * 1.4426950408889634f, k_scale, v_scale};
  const long chunks = 2L * B * T * H * (F8 ? 4 : 8);
  if (chunks >= 2147483647L * 256) throw std::runtime_error(nm + ": tensor too large");
  if constexpr (F8)
    hipLaunchKernelGGL(kv_cache_append_f8_kernel, dim3(dtf_cdiv(chunks, 256)), dim3(256), 0, st,
                       g, chunks);
  else
    hipLaunchKernelGGL(kv_cache_append_kernel, dim3(dtf_cdiv(chunks, 256)), dim3(256), 0, st, g,
                       chunks);
  const int nqb = query_blocks(T);
  if (T <= kSmallT)
    launch_append<1, F8>(g, nqb, st);
  else
    launch_append<4, F8>(g, nqb, st);
  if (splits > 1) {
    const long rows = (long)B * H * T * 16;
    hipLaunchKernelGGL(attn_append_combine_kernel, dim3(dtf_cdiv(rows, 256)), dim3(256), 0, st, g,
                       rows);
  }
}

}  // namespace

void dtf_attn_append(const bf16_t* qkv_new, const int* pos, const int* n_new, bf16_t* k_cache,
                     bf16_t* v_cache, bf16_t* out, float* ws, int B, int T, int H, int C,
                     int max_len, int splits, float scale, hipStream_t st) {
  append_any<false>("attn_append", qkv_new, pos, n_new, k_cache, v_cache, nullptr, nullptr, out,
                    ws, B, T, H, C, max_len, splits, scale, st);
}

void dtf_attn_append_f8(const bf16_t* qkv_new, const int* pos, const int* n_new, uint8_t* k_cache,
                        uint8_t* v_cache, float* k_scale, float* v_scale, bf16_t* out, float* ws,
                        int B, int T, int H, int C, int max_len, int splits, float scale,
                        hipStream_t st) {
  append_any<true>("attn_append_f8", qkv_new, pos, n_new, k_cache, v_cache, k_scale, v_scale, out,
                   ws, B, T, H, C, max_len, splits, scale, st);
}
