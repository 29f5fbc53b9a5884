// The block epilogue shared by the decode kernels (attn_decode.hip, attn_f8.hip): every wave has
// left its (acc[64], m, l) in LDS and 8 threads merge the waves IN WAVE ORDER.
#pragma once
#include "common.h"

namespace decode_merge {

constexpr int kWaves = 4;        // waves per block
constexpr int kWsRow = 66;       // acc[64], m, l
constexpr float kNegInf = -__builtin_inff();

// weight of a partial with maximum m in a merge whose maximum is M: an empty partial (m = -inf)
// weighs exactly 0, also when M is -inf
DTF_DEV float merge_weight(float m, float M) {
  return m == kNegInf ? 0.f : __builtin_amdgcn_exp2f(m - M);
}

// thread sub = 0 .. 7: head dims 8 sub .. + 7 of the 4 waves, in wave order.  splits == 1 writes
// row bh of out [B*H, 64]; otherwise the fp32 partial [acc[64], m, l] goes to row
// (bh splits + split) of the workspace (264-B rows: 8-B aligned).
DTF_DEV void merge_waves(const float (&sm)[kWaves][kWsRow + 2], int sub, bf16_t* out, float* wsp,
                         int splits, int split, long bh) {
  float M = kNegInf;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) M = fmaxf(M, sm[i][64]);
  float L = 0.f, A[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) A[e] = 0.f;
#pragma unroll
  for (int i = 0; i < kWaves; ++i) {
    const float f = merge_weight(sm[i][64], M);
    L = __builtin_fmaf(sm[i][65], f, L);
#pragma unroll
    for (int e = 0; e < 8; ++e) A[e] = __builtin_fmaf(sm[i][sub * 8 + e], f, A[e]);
  }
  if (splits == 1) {
#pragma unroll
    for (int e = 0; e < 8; ++e) A[e] /= L;
    *reinterpret_cast<uint4*>(out + bh * 64 + sub * 8) = pack8(A);
    return;
  }
  float* ws = wsp + (bh * splits + split) * kWsRow;
#pragma unroll
  for (int e = 0; e < 8; e += 2)
    *reinterpret_cast<float2*>(ws + sub * 8 + e) = make_float2(A[e], A[e + 1]);
  if (sub == 0) *reinterpret_cast<float2*>(ws + 64) = make_float2(M, L);
}

}  // namespace decode_merge
