// Incremental decoding against an FP8 key / value cache: the decode kernel and the quantising
// prefill copy.  (The append kernels for this cache are attn_append.hip's, by a template
// parameter.)  The format -- e4m3 bytes [B, H, C, 64], one fp32 power-of-two scale per 64-B row,
// [B, H, C] -- and its quantise / dequantise helpers are kv_f8.h.
//
// dtf_attn_decode_f8 keeps the contract of dtf_attn_decode (attn_decode.hip): pos read on the
// device, rows past pos never loaded, hidden scores selected to -inf, merges in wave and split
// order, no atomics, the same inputs and `splits` give the same bits.  Because float(byte) scale
// is exact, it computes exactly the bf16 kernel's function of the DEQUANTISED cache.
//
// Design.  A cached row is 64 B, half the bf16 row, so the shape of a tile changes:
//   * Data movement: lane l owns the 16-B chunk l & 3 (head dims 16 (l & 3) .. + 15) of rows
//     (l >> 2) + 16 i: one wave instruction covers 16 whole rows (1 KB).  A tile is 128 keys,
//     i = 0 .. 7: 8 K and 8 V loads per lane, all issued before the first is used -- the 16 KB in
//     flight per wave of the bf16 kernel, for twice the keys.  The rows' 8 + 8 scales ride along as
//     4-B loads (the 4 lanes of a row read the same word).  Nothing goes through LDS.
//   * Scores: the 16 bytes convert to fp32 by v_cvt_pk_f32_fp8 (2 values per instruction), 16 FMAs
//     against the query chunk in registers, 2 xor-shuffles over the row's 4 lanes; the K scale
//     multiplies the fp32 score together with scale log2 e, after the dot product.
//   * p = exp2(s - m) stays fp32; l sums the unscaled p and p * v_scale (exact: a power of two)
//     multiplies the unscaled V values into acc[16].  l and acc are per-row-group partials until
//     the wave's tiles are done (one 4-step reduction over the 16 row groups at the end).
//   * The new token's K / V rows are quantised in registers (every row group holds the whole row:
//     a 2-step integer maximum over its 4 lanes gives the scale) and enter the softmax as those
//     bytes and that scale, exactly what later steps will read from the cache.  The last split,
//     which always owns the last tile, stores them (4 lanes x 16 B, and the scale) -- read by
//     nobody in this launch.
//   * Rows past pos: bytes and scales are not loaded (zeros instead) and the score is selected to
//     -inf, so 0x7F bytes and NaN scales in unwritten rows cannot reach a product.
//   * Work split and combine as attn_decode.hip, in 128-key tiles: grid (splits, H, B), 4 waves,
//     a split's tiles dealt round-robin to the waves, the block merge and the workspace rows are
//     attn_decode_merge.h's and the combine launch is attn_decode.hip's.  `splits` comes from
//     dtf_attn_decode_splits (64-key units); a split whose range holds no 128-key tile carries
//     m = -inf, l = 0 and weighs 0.
//
// dtf_kv_cache_fill_f8: one thread per 16 output bytes (32 B of bf16 in), the row maximum over the
// 4 lanes of a row by shuffles, then the scale, then the bytes: a wave writes 16 whole rows in
// 16-B stores and their 16 scales in 4-B stores.  One writer per element; rows >= S and their
// scales are not touched.
#include <stdexcept>
#include <string>

#include "attn_decode_merge.h"
#include "kv_f8.h"
#include "launch.h"

namespace {

using decode_merge::kNegInf;
using decode_merge::kWaves;
using decode_merge::kWsRow;

constexpr int kHd = 64;          // head dim = bytes per cached row
constexpr int kTile = 128;       // keys per tile
constexpr int kRows = kTile / 16;  // rows per lane and tile

DTF_DEV float group4_sum(float v) {            // over the 4 lanes that share a row
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}
DTF_DEV float groups_sum(float v) {            // over the 16 row groups of a wave
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}
DTF_DEV float groups_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 4, 64));
  v = fmaxf(v, __shfl_xor(v, 8, 64));
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  v = fmaxf(v, __shfl_xor(v, 32, 64));
  return v;
}

// the lane's 16-element chunk of a new row, quantised: its bytes and the row's scale
DTF_DEV uint4 quantize_new(const bf16_t* p, float& scale) {
  const uint4 lo = *reinterpret_cast<const uint4*>(p);
  const uint4 hi = *reinterpret_cast<const uint4*>(p + 8);
  const int e = kv_f8_exponent(kv_f8_group4_max(max(kv_f8_absmax8(lo), kv_f8_absmax8(hi))));
  scale = kv_f8_pow2(e);
  return kv_f8_quantize16(lo, hi, kv_f8_pow2(-e));
}

// One 128-key tile of one wave's online softmax.  LAST: the tile that holds row pos -- rows past
// pos are not loaded and score -inf, row pos is the new token's bytes and scale from registers.
template <bool LAST>
DTF_DEV void decode_tile(const uint8_t* kc, const uint8_t* vc, const float* ks, const float* vs,
                         int t, int rg, int sub, int pos, const uint4& knew, const uint4& vnew,
                         float ksn, float vsn, const float (&q)[16], float c, float& m, float& l,
                         float (&acc)[16]) {
  const int key0 = t * kTile + rg;
  // kc / vc / ks / vs are wave-uniform; the lane's part is a 32-bit offset and row i a constant
  const uint32_t off = (uint32_t)key0 * kHd + sub * 16;
  uint4 kr[kRows], vr[kRows];
  float ksc[kRows], vsc[kRows];
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const int key = key0 + 16 * i;
    if (LAST) {
      kr[i] = key == pos ? knew : make_uint4(0, 0, 0, 0);
      ksc[i] = key == pos ? ksn : 0.f;
    }
    if (!LAST || key < pos) {
      kr[i] = *reinterpret_cast<const uint4*>(kc + off + i * 16 * kHd);
      ksc[i] = ks[(uint32_t)key0 + i * 16];
    }
  }
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const int key = key0 + 16 * i;
    if (LAST) {
      vr[i] = key == pos ? vnew : make_uint4(0, 0, 0, 0);
      vsc[i] = key == pos ? vsn : 0.f;
    }
    if (!LAST || key < pos) {
      vr[i] = *reinterpret_cast<const uint4*>(vc + off + i * 16 * kHd);
      vsc[i] = vs[(uint32_t)key0 + i * 16];
    }
  }
  // The scheduler would otherwise convert all 16 chunks to fp32 at once (256 registers): every
  // row's convert-and-FMA group is fenced, so one chunk's 16 floats are live at a time.  All the
  // loads above are already in flight.
  __builtin_amdgcn_sched_barrier(0);
  float s[kRows], tmax = kNegInf;
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    float f[16], d = 0.f;
    kv_f8_unpack16(kr[i], f);
#pragma unroll
    for (int e = 0; e < 16; ++e) d = __builtin_fmaf(q[e], f[e], d);
    s[i] = d;
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const float d = group4_sum(s[i]) * (c * ksc[i]);
    s[i] = !LAST || key0 + 16 * i <= pos ? d : kNegInf;
    tmax = fmaxf(tmax, s[i]);
  }
  // every tile a wave visits holds a visible key, so the new maximum is finite
  const float mn = fmaxf(m, groups_max(tmax));
  const float alpha = __builtin_amdgcn_exp2f(m - mn);      // first tile: exp2(-inf) = 0
  l *= alpha;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] *= alpha;
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    const float p = __builtin_amdgcn_exp2f(s[i] - mn);     // hidden key: exp2(-inf) = 0
    l += p;
    s[i] = p * vsc[i];
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < kRows; ++i) {
    float f[16];
    kv_f8_unpack16(vr[i], f);
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = __builtin_fmaf(s[i], f[e], acc[e]);
    __builtin_amdgcn_sched_barrier(0);
  }
  m = mn;
}

__global__ void __launch_bounds__(64 * kWaves) attn_decode_f8_kernel(const AttnDecodeF8Args g) {
  __shared__ __attribute__((aligned(16))) float sm[kWaves][kWsRow + 2];
  const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane & 3, rg = lane >> 2;
  const int pos = min(max(g.pos[b], 0), g.C - 1);
  const int ntiles = (pos + kTile) / kTile;
  const int t0 = (int)((long)split * ntiles / g.splits);
  const int t1 = (int)((long)(split + 1) * ntiles / g.splits);
  const long HD = (long)g.H * kHd;
  const long bh = (long)b * g.H + h;

  // the lane's chunk of the new token's q, and of its k and v as the cache will hold them
  const bf16_t* nrow = g.qkv_new + (long)b * 3 * HD + h * kHd + sub * 16;
  float q[16];
  unpack8(*reinterpret_cast<const uint4*>(nrow), q);
  unpack8(*reinterpret_cast<const uint4*>(nrow + 8), q + 8);
  float ksn, vsn;
  const uint4 knew = quantize_new(nrow + HD, ksn);
  const uint4 vnew = quantize_new(nrow + 2 * HD, vsn);
  uint8_t* kc = g.k_cache + bh * g.C * kHd;
  uint8_t* vc = g.v_cache + bh * g.C * kHd;
  float* ks = g.k_scale + bh * g.C;
  float* vs = g.v_scale + bh * g.C;
  if (split == g.splits - 1 && w == 0) {                 // 4 lanes x 16 B per row, one scale
    if (rg == 0) {
      *reinterpret_cast<uint4*>(kc + (long)pos * kHd + sub * 16) = knew;
      if (sub == 0) ks[pos] = ksn;
    }
    if (rg == 1) {
      *reinterpret_cast<uint4*>(vc + (long)pos * kHd + sub * 16) = vnew;
      if (sub == 0) vs[pos] = vsn;
    }
  }

  float m = kNegInf, l = 0.f, acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  // tiles wholly below pos stream with plain loads; only the tile of pos pays for the selects
  for (int t = t0 + w; t < t1; t += kWaves) {
    if (t * kTile + kTile - 1 < pos)
      decode_tile<false>(kc, vc, ks, vs, t, rg, sub, pos, knew, vnew, ksn, vsn, q, g.c, m, l, acc);
    else
      decode_tile<true>(kc, vc, ks, vs, t, rg, sub, pos, knew, vnew, ksn, vsn, q, g.c, m, l, acc);
  }
  // a row group's 4 lanes hold the same l; the groups hold disjoint keys
  l = groups_sum(l);
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = groups_sum(acc[e]);
  if (rg == 0) {
#pragma unroll
    for (int e = 0; e < 16; e += 4)
      *reinterpret_cast<float4*>(&sm[w][sub * 16 + e]) =
          make_float4(acc[e], acc[e + 1], acc[e + 2], acc[e + 3]);
    if (sub == 0) {
      sm[w][64] = m;
      sm[w][65] = l;
    }
  }
  __syncthreads();
  if (threadIdx.x >= 8) return;
  decode_merge::merge_waves(sm, threadIdx.x, g.out, g.ws, g.splits, split, bh);
}

// Prefill: the K and V thirds of qkv [B*S, 3*H*64] quantised into rows 0 .. S-1 of the caches.
// One thread per 16 output bytes, chunk-fastest then head then token; n % 4 == 0, so the 4 lanes of
// a row leave together.
__global__ void __launch_bounds__(256) kv_cache_fill_f8_kernel(const KvFillF8Args g) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= g.n) return;
  const int sub = (int)(idx & 3);
  long r = idx >> 2;
  const int h = (int)(r % g.H);
  r /= g.H;
  const int s = (int)(r % g.S);
  r /= g.S;
  const int b = (int)(r % g.B);
  const int which = (int)(r / g.B);                       // 0: K, 1: V
  const long HD = (long)g.H * kHd;
  const bf16_t* src = g.qkv + ((long)b * g.S + s) * 3 * HD + (1 + which) * HD + h * kHd + sub * 16;
  const long row = ((long)b * g.H + h) * g.C + s;
  float scale;
  const uint4 bytes = quantize_new(src, scale);
  *reinterpret_cast<uint4*>((which ? g.v_cache : g.k_cache) + row * kHd + sub * 16) = bytes;
  if (sub == 0) (which ? g.v_scale : g.k_scale)[row] = scale;
}

}  // namespace

void dtf_attn_decode_f8(const bf16_t* qkv_new, const int* pos, uint8_t* k_cache, uint8_t* v_cache,
                        float* k_scale, float* v_scale, bf16_t* out, float* ws, int B, int H,
                        int C, int max_len, int splits, float scale, hipStream_t st) {
  if (!qkv_new || !pos || !k_cache || !v_cache || !k_scale || !v_scale || !out)
    throw std::runtime_error("attn_decode_f8: null pointer");
  if (B < 1 || H < 1 || B > 65535 || H > 65535)
    throw std::runtime_error("attn_decode_f8: 1 <= B, H <= 65535");
  if (C < 64 || C % 64)
    throw std::runtime_error(
        "attn_decode_f8: cache capacity must be a multiple of 64, at least 64");
  if (max_len < 1 || max_len > C)
    throw std::runtime_error("attn_decode_f8: 1 <= max_len <= capacity");
  if (splits == 0) splits = dtf_attn_decode_splits(B, H, max_len);
  const int tiles64 = (max_len + 63) / 64;
  if (splits < 1 || splits > tiles64)
    throw std::runtime_error("attn_decode_f8: splits " + std::to_string(splits) + " exceeds the " +
                             std::to_string(tiles64) + " tiles of max_len");
  if (splits > 1 && !ws) throw std::runtime_error("attn_decode_f8: splits > 1 needs the workspace");
  const AttnDecodeF8Args g{qkv_new, pos, k_cache, v_cache, k_scale, v_scale, out, ws, B, H, C,
                           splits, scale * 1.4426950408889634f};
  hipLaunchKernelGGL(attn_decode_f8_kernel, dim3(splits, H, B), dim3(64 * kWaves), 0, st, g);
  if (splits > 1) {
    AttnDecodeArgs cg{};
    cg.out = out;
    cg.ws = ws;
    cg.B = B;
    cg.H = H;
    cg.splits = splits;
    dtf_attn_decode_combine(cg, st);
  }
}

void dtf_kv_cache_fill_f8(const bf16_t* qkv, uint8_t* k_cache, uint8_t* v_cache, float* k_scale,
                          float* v_scale, int B, int S, int H, int C, hipStream_t st) {
  if (!qkv || !k_cache || !v_cache || !k_scale || !v_scale)
    throw std::runtime_error("kv_cache_fill_f8: null pointer");
  if (C < 64 || C % 64)
    throw std::runtime_error(
        "kv_cache_fill_f8: cache capacity must be a multiple of 64, at least 64");
  if (B < 1 || H < 1 || S < 1 || S > C)
    throw std::runtime_error("kv_cache_fill_f8: B, H >= 1 and 1 <= seq_len <= capacity");
  const long n = 2L * B * S * H * 4;
  if (n >= 2147483647L * 256) throw std::runtime_error("kv_cache_fill_f8: tensor too large");
  const KvFillF8Args g{qkv, k_cache, v_cache, k_scale, v_scale, B, S, H, C, n};
  hipLaunchKernelGGL(kv_cache_fill_f8_kernel, dim3(dtf_cdiv(n, 256)), dim3(256), 0, st, g);
}
