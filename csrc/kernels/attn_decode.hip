// Incremental decoding for the causal model: attention of ONE new query per sequence against a
// per-sequence cache of keys and values, and the prefill copy that fills that cache.
//
// Cache layout: k_cache / v_cache are bf16 [B, H, C, 64] (C = capacity in tokens, C % 64 == 0):
// the keys of one (batch, head) are one contiguous run of 128-B rows, which is what a streaming
// read wants (the token-major QKV matrix interleaves the heads every 128 B).
//
// dtf_attn_decode, per (b, h), with pos = clamp(pos[b], 0, C - 1) read ON THE DEVICE:
//   1. the new token's K / V rows (from qkv_new) are stored into the caches at row pos;
//   2. out = softmax2(q . K^T * scale * log2 e) V over keys 0 .. pos, the new one among them;
//   3. out is rounded once to bf16.
//
// Design.  One query per (b, h) is 256 FLOPs per 256 B of K and V: 1 FLOP per byte, three orders
// of magnitude under the MFMA roofline and bandwidth-bound even on plain VALU FMAs, so there is
// no MFMA here (a 16-query tile would be 1/16 full and would need p rounded to bf16 for its B
// operand; fp32 FMAs keep p, l and the accumulator in fp32 for free).
//   * Work split: grid (splits, H, B), 4 waves per block.  The ceil(len / 64) 64-key tiles of a
//     row are cut into `splits` contiguous ranges [s n / splits, (s + 1) n / splits) -- balanced
//     for the row's OWN length, so a short row leaves whole splits empty rather than one split
//     with everything -- and a block's range is dealt round-robin to its 4 waves (neighbouring
//     waves stream neighbouring 8-KB tiles).
//   * Data movement: a tile is 64 rows x 128 B.  Lane l owns the 16-B chunk l & 7 (head dims
//     8 (l & 7) .. + 7) of rows (l >> 3) + 8 i, i = 0 .. 7: every load is 16 B per lane and one
//     wave instruction covers 8 whole rows (1 KB).  All 8 K and 8 V loads of a tile are issued
//     before the first is used (16 KB in flight per wave); nothing goes through LDS, every byte
//     is used exactly once.  The query's 8 values for the lane's chunk sit in registers.
//   * Scores: 8 FMAs per row and lane, summed over the 8 lanes of a row with 3 xor-shuffles; the
//     tile maximum with 3 more across the row groups.  The lane then holds the 8 scores of its
//     rows; p = exp2(s - m) stays fp32 and multiplies the lane's V chunk into acc[8].  l and acc
//     are per-row-group partials until the wave's tiles are done (one 3-step reduction at the end).
//   * Rows past pos are never loaded (the lane's 16 B are zeros instead) and their scores are
//     SELECTED to -inf, so NaN bit patterns in unwritten cache rows cannot reach a product.  Row
//     pos itself comes from the registers that hold the new K / V chunk, never from the cache: the
//     store of step 1 (made by the last split, which always owns the last tile) is read by nobody
//     in this launch.
//   * Combine: each wave leaves (m, l, acc[64]) in LDS; 8 threads merge the 4 waves IN WAVE ORDER.
//     A wave or split without a key carries m = -inf, l = 0 and is given the factor 0 by a select
//     (no exp2(-inf - -inf)).  splits == 1 writes out directly; otherwise the block writes its
//     fp32 partial [acc[64], m, l] to the workspace [B, H, splits, 66] and
//     attn_decode_combine_kernel merges the partials IN SPLIT ORDER.  No atomics, no counters:
//     the same inputs and the same `splits` give the same bits.
//   * The key loop's bound comes from pos[b] on the device; the host's max_len only bounds
//     `splits`.  A generation loop never synchronises to launch a step.
#include <stdexcept>
#include <string>

#include "attn_decode_merge.h"
#include "launch.h"

namespace {

using decode_merge::kNegInf;
using decode_merge::kWaves;
using decode_merge::kWsRow;
using decode_merge::merge_weight;

constexpr int kHd = 64;          // head dim
constexpr int kTile = 64;        // keys per tile

DTF_DEV float group8_sum(float v) {            // over the 8 lanes that share a row
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  return v;
}
DTF_DEV float groups_sum(float v) {            // over the 8 row groups of a wave
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
DTF_DEV float groups_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 8, 64));
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  v = fmaxf(v, __shfl_xor(v, 32, 64));
  return v;
}

// One 64-key tile of one wave's online softmax.  LAST: the tile that holds row pos -- rows past
// pos are not loaded and score -inf, row pos is the new token's chunk from registers.
template <bool LAST>
DTF_DEV void decode_tile(const bf16_t* kc, const bf16_t* vc, int t, int rg, int pos,
                         const uint4& knew, const uint4& vnew, const float (&q)[8], float c,
                         float& m, float& l, float (&acc)[8]) {
  const int key0 = t * kTile + rg;
  uint4 kr[8], vr[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int key = key0 + 8 * i;
    if (LAST) kr[i] = key == pos ? knew : make_uint4(0, 0, 0, 0);
    if (!LAST || key < pos) kr[i] = *reinterpret_cast<const uint4*>(kc + (long)key * kHd);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int key = key0 + 8 * i;
    if (LAST) vr[i] = key == pos ? vnew : make_uint4(0, 0, 0, 0);
    if (!LAST || key < pos) vr[i] = *reinterpret_cast<const uint4*>(vc + (long)key * kHd);
  }
  float s[8], tmax = kNegInf;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float f[8], d = 0.f;
    unpack8(kr[i], f);
#pragma unroll
    for (int e = 0; e < 8; ++e) d = __builtin_fmaf(q[e], f[e], d);
    d = group8_sum(d) * c;
    s[i] = !LAST || key0 + 8 * i <= pos ? d : kNegInf;
    tmax = fmaxf(tmax, s[i]);
  }
  // every tile a wave visits holds a visible key, so the new maximum is finite
  const float mn = fmaxf(m, groups_max(tmax));
  const float alpha = __builtin_amdgcn_exp2f(m - mn);      // first tile: exp2(-inf) = 0
  l *= alpha;
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] *= alpha;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float p = __builtin_amdgcn_exp2f(s[i] - mn);     // hidden key: exp2(-inf) = 0
    float f[8];
    unpack8(vr[i], f);
    l += p;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = __builtin_fmaf(p, f[e], acc[e]);
  }
  m = mn;
}

__global__ void __launch_bounds__(64 * kWaves) attn_decode_kernel(const AttnDecodeArgs g) {
  __shared__ __attribute__((aligned(16))) float sm[kWaves][kWsRow + 2];
  const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane & 7, rg = lane >> 3;
  const int pos = min(max(g.pos[b], 0), g.C - 1);
  const int ntiles = (pos + kTile) / kTile;
  const int t0 = (int)((long)split * ntiles / g.splits);
  const int t1 = (int)((long)(split + 1) * ntiles / g.splits);
  const long HD = (long)g.H * kHd;

  // the lane's chunk of the new token's q, k and v
  const bf16_t* nrow = g.qkv_new + (long)b * 3 * HD + h * kHd + sub * 8;
  float q[8];
  unpack8(*reinterpret_cast<const uint4*>(nrow), q);
  const uint4 knew = *reinterpret_cast<const uint4*>(nrow + HD);
  const uint4 vnew = *reinterpret_cast<const uint4*>(nrow + 2 * HD);
  const long base = ((long)b * g.H + h) * g.C * kHd + sub * 8;
  bf16_t* kc = g.k_cache + base;
  bf16_t* vc = g.v_cache + base;
  if (split == g.splits - 1 && w == 0) {               // 8 lanes x 16 B per row
    if (rg == 0) *reinterpret_cast<uint4*>(kc + (long)pos * kHd) = knew;
    if (rg == 1) *reinterpret_cast<uint4*>(vc + (long)pos * kHd) = vnew;
  }

  float m = kNegInf, l = 0.f, acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  // tiles wholly below pos stream with plain loads; only the tile of pos pays for the selects
  for (int t = t0 + w; t < t1; t += kWaves) {
    if (t * kTile + kTile - 1 < pos)
      decode_tile<false>(kc, vc, t, rg, pos, knew, vnew, q, g.c, m, l, acc);
    else
      decode_tile<true>(kc, vc, t, rg, pos, knew, vnew, q, g.c, m, l, acc);
  }
  // a row group's 8 lanes hold the same l; the groups hold disjoint keys
  l = groups_sum(l);
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = groups_sum(acc[e]);
  if (rg == 0) {
    *reinterpret_cast<float4*>(&sm[w][sub * 8]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(&sm[w][sub * 8 + 4]) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    if (sub == 0) {
      sm[w][64] = m;
      sm[w][65] = l;
    }
  }
  __syncthreads();
  if (threadIdx.x >= 8) return;

  // threads 0 .. 7: head dims 8 sub .. + 7 of the 4 waves, in wave order
  decode_merge::merge_waves(sm, sub, g.out, g.ws, g.splits, split, (long)b * g.H + h);
}

// 8 threads per (b, h): the partials of its splits merged in split order.  The last split always
// holds the last tile, so the merged maximum is finite and L > 0.
__global__ void __launch_bounds__(256) attn_decode_combine_kernel(const AttnDecodeArgs g) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long bh = idx >> 3;
  const int sub = (int)(idx & 7);
  if (bh >= (long)g.B * g.H) return;
  const float* ws = g.ws + bh * g.splits * kWsRow;
  float M = kNegInf;
  for (int s = 0; s < g.splits; ++s) M = fmaxf(M, ws[s * kWsRow + 64]);
  float L = 0.f, A[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) A[e] = 0.f;
  for (int s = 0; s < g.splits; ++s) {
    const float* r = ws + s * kWsRow;
    const float2 ml = *reinterpret_cast<const float2*>(r + 64);
    const float f = merge_weight(ml.x, M);
    L = __builtin_fmaf(ml.y, f, L);
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      const float2 a = *reinterpret_cast<const float2*>(r + sub * 8 + e);
      A[e] = __builtin_fmaf(a.x, f, A[e]);
      A[e + 1] = __builtin_fmaf(a.y, f, A[e + 1]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) A[e] /= L;
  *reinterpret_cast<uint4*>(g.out + bh * kHd + sub * 8) = pack8(A);
}

// Prefill: the K and V thirds of qkv [B*S, 3*H*64] into rows 0 .. S-1 of the caches.  One thread
// per 16-B chunk, chunk-fastest then head then token: a wave reads 8 whole 128-B head rows of one
// token and writes 8 whole cache rows.  One writer per element; rows >= S are not touched.
__global__ void __launch_bounds__(256) kv_cache_fill_kernel(const KvFillArgs g) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= g.n) return;
  const int sub = (int)(idx & 7);
  long r = idx >> 3;
  const int h = (int)(r % g.H);
  r /= g.H;
  const int s = (int)(r % g.S);
  r /= g.S;
  const int b = (int)(r % g.B);
  const int which = (int)(r / g.B);                       // 0: K, 1: V
  const long HD = (long)g.H * kHd;
  const bf16_t* src = g.qkv + ((long)b * g.S + s) * 3 * HD + (1 + which) * HD + h * kHd + sub * 8;
  bf16_t* dst = (which ? g.v_cache : g.k_cache) + (((long)b * g.H + h) * g.C + s) * kHd + sub * 8;
  *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
}

constexpr int kCus = 256;            // MI355X
// the combine launch costs ~2.5 us: measured worth it from two tiles per wave per split on (at 8
// tiles, len 512, two splits were 10 us against 8 us; at 32 tiles 11 against 18 at B = 1)
constexpr int kMinSplitTiles = 8;
constexpr int kMaxSplits = 64;

int tiles_of(int len) { return (len + kTile - 1) / kTile; }

}  // namespace

// `splits` for a launch: enough blocks for two per CU, but no split below kMinSplitTiles tiles.
// A pure function of (B * H, max_len).
int dtf_attn_decode_splits(int B, int H, int max_len) {
  if (B < 1 || H < 1 || max_len < 1) throw std::runtime_error("attn_decode_splits: B, H, max_len >= 1");
  const long bh = (long)B * H;
  long want = (2 * kCus + bh - 1) / bh;
  const long cap = tiles_of(max_len) / kMinSplitTiles;
  if (want > cap) want = cap;
  if (want > kMaxSplits) want = kMaxSplits;
  return want < 1 ? 1 : (int)want;
}

long dtf_attn_decode_ws_floats(int B, int H, int splits) {
  return splits > 1 ? (long)B * H * splits * kWsRow : 0;
}

// the combine launch alone (reads g.ws, g.splits, g.B, g.H; writes g.out): attn_f8.hip's decode
// kernel leaves the same workspace rows
void dtf_attn_decode_combine(const AttnDecodeArgs& g, hipStream_t st) {
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(dtf_cdiv((long)g.B * g.H * 8, 256)),
                     dim3(256), 0, st, g);
}

void dtf_attn_decode(const bf16_t* qkv_new, const int* pos, bf16_t* k_cache, bf16_t* v_cache,
                     bf16_t* out, float* ws, int B, int H, int C, int max_len, int splits,
                     float scale, hipStream_t st) {
  if (!qkv_new || !pos || !k_cache || !v_cache || !out)
    throw std::runtime_error("attn_decode: null pointer");
  if (B < 1 || H < 1 || B > 65535 || H > 65535)
    throw std::runtime_error("attn_decode: 1 <= B, H <= 65535");
  if (C < kTile || C % kTile)
    throw std::runtime_error("attn_decode: cache capacity must be a multiple of 64, at least 64");
  if (max_len < 1 || max_len > C) throw std::runtime_error("attn_decode: 1 <= max_len <= capacity");
  if (splits == 0) splits = dtf_attn_decode_splits(B, H, max_len);
  if (splits < 1 || splits > tiles_of(max_len))
    throw std::runtime_error("attn_decode: splits " + std::to_string(splits) + " exceeds the " +
                             std::to_string(tiles_of(max_len)) + " tiles of max_len");
  if (splits > 1 && !ws) throw std::runtime_error("attn_decode: splits > 1 needs the workspace");
  const AttnDecodeArgs g{qkv_new, pos, k_cache, v_cache, out, ws, B, H, C, splits,
                         scale * 1.4426950408889634f};
  hipLaunchKernelGGL(attn_decode_kernel, dim3(splits, H, B), dim3(64 * kWaves), 0, st, g);
  if (splits > 1) dtf_attn_decode_combine(g, st);
}

void dtf_kv_cache_fill(const bf16_t* qkv, bf16_t* k_cache, bf16_t* v_cache, int B, int S, int H,
                       int C, hipStream_t st) {
  if (!qkv || !k_cache || !v_cache) throw std::runtime_error("kv_cache_fill: null pointer");
  if (C < kTile || C % kTile)
    throw std::runtime_error("kv_cache_fill: cache capacity must be a multiple of 64, at least 64");
  if (B < 1 || H < 1 || S < 1 || S > C)
    throw std::runtime_error("kv_cache_fill: B, H >= 1 and 1 <= seq_len <= capacity");
  const long n = 2L * B * S * H * 8;
  if (n >= 2147483647L * 256) throw std::runtime_error("kv_cache_fill: tensor too large");
  const KvFillArgs g{qkv, k_cache, v_cache, B, S, H, C, n};
  hipLaunchKernelGGL(kv_cache_fill_kernel, dim3(dtf_cdiv(n, 256)), dim3(256), 0, st, g);
}
