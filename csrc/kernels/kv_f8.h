// The FP8 key / value cache format, device side (the rule is ops/reference.py kv_quantize_rows and
// the kernels reproduce it bit for bit).
//
// A cache row is 64 OCP e4m3 bytes (448 the largest value, 0x7F / 0xFF NaN) and one fp32 scale
// s = 2^e.  With a = max |x_i| = f 2^k, f in [0.5, 1):  e = k - 9 if f <= 0.875 (448 = 0.875 2^9),
// else k - 8, clamped to [-100, 120]; a == 0 gives e = 0.  Byte i is rne_e4m3(x_i 2^-e): by
// construction |x_i 2^-e| <= 448, nothing saturates.  float(byte) s is exact in fp32 and, with the
// clamp, a normal bf16: the attention kernels see exactly the dequantised cache.
//
// Everything about the exponent is integer arithmetic on the bf16 bit patterns (magnitudes of
// bf16 order as integers), so denormal modes cannot move a scale.  Non-finite input is outside
// the contract; it lands on e = 120 and converts to whatever the instruction gives.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(2))) float f32x2_t;

// largest magnitude (bf16 bits, sign cleared) among the 8 bf16 of a 16-B chunk
DTF_DEV uint32_t kv_f8_absmax8(const uint4& v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t a = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) a = max(a, max(w[i] & 0x7fffu, (w[i] >> 16) & 0x7fffu));
  return a;
}
// over the 4 lanes that share a 64-element row (16 elements each)
DTF_DEV uint32_t kv_f8_group4_max(uint32_t a) {
  a = max(a, (uint32_t)__shfl_xor((int)a, 1, 64));
  a = max(a, (uint32_t)__shfl_xor((int)a, 2, 64));
  return a;
}
// the row's exponent e from its largest magnitude
DTF_DEV int kv_f8_exponent(uint32_t absmax16) {
  const int k = (int)(absmax16 >> 7) - 126;               // a = 1.m 2^(k - 1); a denormal a clamps
  const int e = (absmax16 & 0x7fu) <= 0x60u ? k - 9 : k - 8;   // 1.m <= 1.75
  return absmax16 == 0 ? 0 : min(max(e, -100), 120);
}
DTF_DEV float kv_f8_pow2(int e) { return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23); }

// 16 bf16 (two 16-B chunks) times inv = 2^-e -> 16 e4m3 bytes
DTF_DEV uint4 kv_f8_quantize16(const uint4& lo, const uint4& hi, float inv) {
  float f[16];
  unpack8(lo, f);
  unpack8(hi, f + 8);
  uint32_t r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i] * inv, f[4 * i + 1] * inv, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * i + 2] * inv, f[4 * i + 3] * inv, w, true);
    r[i] = (uint32_t)w;
  }
  return make_uint4(r[0], r[1], r[2], r[3]);
}
// 16 e4m3 bytes -> their 16 values as fp32, unscaled
DTF_DEV void kv_f8_unpack16(const uint4& v, float* f) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f32x2_t b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    f[4 * i] = a[0];
    f[4 * i + 1] = a[1];
    f[4 * i + 2] = b[0];
    f[4 * i + 3] = b[1];
  }
}
// 16 e4m3 bytes times s = 2^e -> 16 bf16, exactly (the products have 4 significant bits)
DTF_DEV void kv_f8_dequantize16(const uint4& v, float s, uint4& lo, uint4& hi) {
  float f[16];
  kv_f8_unpack16(v, f);
  uint32_t r[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
    r[i] = (__builtin_bit_cast(uint32_t, f[2 * i] * s) >> 16) |
           (__builtin_bit_cast(uint32_t, f[2 * i + 1] * s) & 0xffff0000u);
  lo = make_uint4(r[0], r[1], r[2], r[3]);
  hi = make_uint4(r[4], r[5], r[6], r[7]);
}
