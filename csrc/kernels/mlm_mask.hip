// Fused on-device masked-LM example creation for HBM-resident token sets (data/tokens.py): one
// launch turns a batch of example indices into the six tensors BERT pre-training reads,
//   gather -> input mask / segment ids -> choose the positions to predict -> 80 / 10 / 10
//   replacement -> input_ids, segment_ids, input_mask, masked_lm_positions / ids / weights.
//
// The rule is integer arithmetic (ops/reference.py mlm_mask_tokens is the same rule in torch and
// the tests' oracle; the two agree to the bit).  Row b reads example idx[b]; its hashes are keyed
// on the example number n = ex_offset + idx[b] * ex_stride (a shard passes the global number):
//   row_seed = fmix32(lo32(n) * 0x9E3779B1 + seed) ^ hi32(n)
//   key[j]   = fmix32(j * 0x9E3779B1 + row_seed)
//   input_mask[j]  = t[j] != pad;  segment_ids[j] = input_mask[j] && j > first sep
//   candidates: t[j] not in {pad, cls, sep};  nc of them
//   T = nc == 0 ? 0 : min(P, nc, max(1, (nc * prob_q16 + 32768) >> 16))
//   selected: the T candidates with the smallest (key[j], j); listed in ascending j
//   at a selected j: h2 = fmix32(key[j] + 0x85EBCA6B), d = ((h2 & 0xFFFF) * 10) >> 16
//     d < 8 -> mask_id;  d == 8 -> t[j];
//     d == 9 -> random_low + ((fmix32(h2 + 0x9E3779B1) * (vocab - random_low)) >> 32)
//
// Mapping: one 64-lane wave per row, 4 waves per block, rows grid-strided.  A lane owns positions
// lane, lane + 64, ... (at most 8: S <= 512) and keeps their tokens and keys in registers.  The
// first sep and nc come from ballots.  The rank of a candidate among the (key, j) pairs is counted
// against the whole row, staged as 64-bit (key << 32 | j) words in the wave's own LDS slice
// (every lane reads the same word: a broadcast); a position that is no candidate is staged as all
// ones, so it is never below a candidate.  The output slot of a selected position is the number
// of selected positions below it: a ballot prefix per 64-column group plus a running base.  A wave
// shares nothing with another wave, so the kernel has no block barrier.
//
// Whole-word masking (WORDS = true, dtf_mlm_mask_words) changes only the choice of the selected
// positions; continuation[v] = 1 marks id v as a continuation piece (an id past the table is none):
//   candidate j starts a word iff !continuation[t[j]], or j == 0, or j - 1 is no candidate;
//   a word is a start and the candidates up to the next start or non-candidate; nw of them
//   words are visited in ascending (key[start], start); taken = 0; for each word: stop if
//   taken >= T; skip it if taken + len > T; else select all of its tokens and add len to taken
//   T' = taken slots are filled (T' <= T; T == nc selects everything: the same shortcut)
// Each selected token draws its own 80 / 10 / 10 from its own key[j], as above.
// Mapping: per 64-position group the candidates, the starts and the in-word continuations
// (candidates that are no start) are wave-uniform ballot masks.  A start reads its word's length
// off the continuation masks (the run of ones above it), ranks itself among the starts through the
// same LDS pair slice (only starts are staged) and writes the length into a second per-wave LDS
// array indexed by rank.  The greedy fill runs wave-uniformly over the ranks, 64 lengths per LDS
// read and one v_readlane per step, and records the words that fit as one bit per rank.  The
// selected starts are balloted per group and flooded over their words with one 512-bit add:
// adding (starts << 1) to the continuation mask carries through exactly the run above each start.
#include <stdexcept>
#include <string>

#include "launch.h"

namespace {
constexpr int kMlmWaves = 4;                 // rows in flight per block
constexpr int kMlmMaxS = 512;
constexpr int kMlmGroups = kMlmMaxS / 64;    // positions per lane
constexpr int kMlmDefaultBlocks = 2048;

DTF_DEV uint32_t mlm_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

template <typename TokT, bool WORDS>
__global__ void __launch_bounds__(kMlmWaves * 64)
mlm_mask_kernel(const TokT* __restrict__ tokens, const int64_t* __restrict__ idx,
                int64_t* __restrict__ input_ids, int64_t* __restrict__ segment_ids,
                int64_t* __restrict__ input_mask, int64_t* __restrict__ positions,
                int64_t* __restrict__ ids, float* __restrict__ weights, long N, int B, int S, int P,
                uint32_t seed, long ex_stride, long ex_offset, MlmMaskRule r,
                const uint8_t* __restrict__ continuation) {
  __shared__ uint64_t s_pair[kMlmWaves][kMlmMaxS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t* pair = s_pair[wave];
  const int G = (S + 63) >> 6;                                   // groups in use, wave-uniform
  const uint64_t below = (1ull << lane) - 1;                     // the lanes under this one

  for (long b = (long)blockIdx.x * kMlmWaves + wave; b < B; b += (long)gridDim.x * kMlmWaves) {
    const int64_t row = idx[b];
    const bool ok = row >= 0 && row < N;       // a bad index is an all-pad row, never a read past
    const TokT* src = tokens + (ok ? row : 0) * (int64_t)S;      // 64-bit row base
    const uint64_t n = (uint64_t)ex_offset + (uint64_t)row * (uint64_t)ex_stride;
    const uint32_t row_seed =
        mlm_fmix32((uint32_t)n * 0x9E3779B1u + seed) ^ (uint32_t)(n >> 32);

    uint32_t t[kMlmGroups], key[kMlmGroups];
    bool cand[kMlmGroups];
    int first_sep = S, nc = 0;                 // S: no sep in the row
    // WORDS: the candidates, the word starts and the in-word continuations of each group, and the
    // number of words; wave-uniform
    uint64_t cmask[kMlmGroups], smask[kMlmGroups], inner[kMlmGroups];
    uint64_t carry = 0;                        // is the group below's last position a candidate
    int nw = 0;
#pragma unroll
    for (int g = 0; g < kMlmGroups; ++g) {
      t[g] = r.pad_id;
      key[g] = 0;
      cand[g] = false;
      if (g < G) {
        const int j = g * 64 + lane;
        const bool in = j < S;
        if (in && ok) t[g] = (uint32_t)src[j];                   // TokT is unsigned
        key[g] = mlm_fmix32((uint32_t)j * 0x9E3779B1u + row_seed);
        cand[g] = in && t[g] != r.pad_id && t[g] != r.cls_id && t[g] != r.sep_id;
        const uint64_t seps = __ballot(in && t[g] == r.sep_id);
        if (seps != 0 && first_sep == S) first_sep = g * 64 + __builtin_ctzll(seps);
        if constexpr (WORDS) {
          const bool piece = cand[g] && t[g] < r.vocab_size && continuation[t[g]] != 0;
          const uint64_t cm = __ballot(cand[g]), km = __ballot(piece);
          const uint64_t sm = cm & ~(km & ((cm << 1) | carry));
          carry = cm >> 63;
          cmask[g] = cm;
          smask[g] = sm;
          inner[g] = cm & ~sm;
          nc += __popcll(cm);
          nw += __popcll(sm);
          if (in) pair[j] = (sm >> lane) & 1 ? ((uint64_t)key[g] << 32) | (uint32_t)j : ~0ull;
        } else {
          nc += __popcll(__ballot(cand[g]));
          if (in) pair[j] = cand[g] ? ((uint64_t)key[g] << 32) | (uint32_t)j : ~0ull;
        }
      } else if constexpr (WORDS) {
        cmask[g] = smask[g] = inner[g] = 0;
      }
    }
    int T = 0;
    if (nc > 0) {
      T = (int)(((uint32_t)nc * r.prob_q16 + 32768u) >> 16);     // nc <= 512, prob_q16 <= 65536
      T = T < 1 ? 1 : T;
      T = T > nc ? nc : T;
      T = T > P ? P : T;
    }

    // rank of each own candidate among the row's pairs; the slice is this wave's alone, and a
    // wave runs in lockstep, so the LDS writes above are complete once they are waited for
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    int rank[kMlmGroups];
    uint64_t mine[kMlmGroups];
#pragma unroll
    for (int g = 0; g < kMlmGroups; ++g) {
      rank[g] = 0;
      mine[g] = ((uint64_t)key[g] << 32) | (uint32_t)(g * 64 + lane);
    }
    if (T > 0 && T < nc) {
      for (int j = 0; j < S; ++j) {
        const uint64_t other = pair[j];
#pragma unroll
        for (int g = 0; g < kMlmGroups; ++g)
          if (g < G) rank[g] += other < mine[g] ? 1 : 0;
      }
    }                                          // T == nc: every candidate is selected, rank 0 < T
    // every lane is past its reads before the next row's writes to the slice
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    int filled = T;                            // slots in use
    uint64_t wsel[kMlmGroups];                 // WORDS: the selected positions of each group
    if constexpr (WORDS) {
      __shared__ uint16_t s_len[kMlmWaves][kMlmMaxS];
      uint16_t* lens = s_len[wave];            // a word's length, by the rank of its start
#pragma unroll
      for (int g = 0; g < kMlmGroups; ++g) wsel[g] = cmask[g];   // T == nc, or no candidate
      if (T > 0 && T < nc) {
        // the run of in-word continuations above an own start, walked up the groups
#pragma unroll
        for (int g = 0; g < kMlmGroups; ++g) {
          if (g < G && ((smask[g] >> lane) & 1)) {
            int len = 1;
            const uint64_t above = lane == 63 ? 0 : ~inner[g] >> (lane + 1);
            bool open = above == 0;            // the word runs to the end of this group
            len += open ? 63 - lane : __builtin_ctzll(above);
#pragma unroll
            for (int h = g + 1; h < kMlmGroups; ++h) {
              if (open && h < G) {
                open = ~inner[h] == 0;
                len += open ? 64 : __builtin_ctzll(~inner[h]);
              }
            }
            lens[rank[g]] = (uint16_t)len;     // ranks of starts are distinct and below nw
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the greedy fill over the ranks; fit: the words taken, one bit per rank
        int taken = 0;
        uint64_t fit[kMlmGroups];
#pragma unroll
        for (int q = 0; q < kMlmGroups; ++q) {
          uint64_t f = 0;
          if (q * 64 < nw && taken < T) {
            const int left = nw - q * 64 < 64 ? nw - q * 64 : 64;
            const int own = lane < left ? lens[q * 64 + lane] : 0;
            for (int k = 0; k < left && taken < T; ++k) {
              const int len = __builtin_amdgcn_readlane(own, k);
              if (taken + len <= T) {
                taken += len;
                f |= 1ull << k;
              }
            }
          }
          fit[q] = f;
        }
        filled = taken;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the selected starts, flooded over their words: adding (starts << 1) to the in-word
        // continuations flips exactly the run of ones above each selected start
        uint64_t shift_in = 0, add_in = 0;
#pragma unroll
        for (int g = 0; g < kMlmGroups; ++g) {
          bool hit = false;
          if (g < G && ((smask[g] >> lane) & 1)) {
#pragma unroll
            for (int q = 0; q < kMlmGroups; ++q)
              if ((rank[g] >> 6) == q) hit = (fit[q] >> (rank[g] & 63)) & 1;
          }
          const uint64_t ss = g < G ? __ballot(hit) : 0;
          const uint64_t a = (ss << 1) | shift_in;
          shift_in = ss >> 63;
          const uint64_t s1 = inner[g] + a, s2 = s1 + add_in;
          add_in = (s1 < a) | (s2 < s1);
          wsel[g] = ss | ((s2 ^ inner[g]) & inner[g]);
        }
      }
    }

    const int64_t obase = (int64_t)b * S, pbase = (int64_t)b * P;
    int slot_base = 0;
#pragma unroll
    for (int g = 0; g < kMlmGroups; ++g) {
      if (g < G) {
        const int j = g * 64 + lane;
        const bool in = j < S;
        bool sel;
        if constexpr (WORDS) {
          sel = (wsel[g] >> lane) & 1;
        } else {
          sel = cand[g] && rank[g] < T;
        }
        const uint64_t selm = __ballot(sel);
        uint32_t v = t[g];
        if (sel) {
          const uint32_t h2 = mlm_fmix32(key[g] + 0x85EBCA6Bu);
          const uint32_t d = ((h2 & 0xFFFFu) * 10u) >> 16;
          if (d < 8) {
            v = r.mask_id;
          } else if (d == 9) {
            v = r.random_low + __umulhi(mlm_fmix32(h2 + 0x9E3779B1u), r.vocab_size - r.random_low);
          }
          const int slot = slot_base + __popcll(selm & below);   // < T <= P: ranks are distinct
          if (slot < P) {
            positions[pbase + slot] = j;
            ids[pbase + slot] = t[g];
            weights[pbase + slot] = 1.0f;
          }
        }
        if (in) {
          const bool real = t[g] != r.pad_id;
          input_ids[obase + j] = v;
          input_mask[obase + j] = real ? 1 : 0;
          segment_ids[obase + j] = real && j > first_sep ? 1 : 0;
        }
        slot_base += __popcll(selm);
      }
    }
    for (int s = filled + lane; s < P; s += 64) {                // the unused slots
      positions[pbase + s] = 0;
      ids[pbase + s] = 0;
      weights[pbase + s] = 0.0f;
    }
  }
}
}  // namespace

// Shared by both launchers: ``continuation`` == nullptr is the token rule.
static void mlm_mask_launch(const char* name, const void* tokens, int token_bytes,
                            const int64_t* idx, const uint8_t* continuation, int64_t* input_ids,
                            int64_t* segment_ids, int64_t* input_mask, int64_t* positions,
                            int64_t* ids, float* weights, long N, int B, int S, int P,
                            uint32_t seed, long ex_stride, long ex_offset,
                            const MlmMaskRule& rule, int max_blocks, hipStream_t st) {
  const std::string op(name);
  if (token_bytes != 2 && token_bytes != 4)
    throw std::runtime_error(op + ": tokens are 16-bit or 32-bit");
  if (N < 1 || S < 1 || S > kMlmMaxS) throw std::runtime_error(op + ": S in [1, 512]");
  if (B < 0 || P < 1 || P > S) throw std::runtime_error(op + ": P in [1, S]");
  if (rule.prob_q16 > 65536u) throw std::runtime_error(op + ": prob above 1");
  if (rule.vocab_size < 1 || rule.random_low >= rule.vocab_size || rule.pad_id >= rule.vocab_size ||
      rule.cls_id >= rule.vocab_size || rule.sep_id >= rule.vocab_size ||
      rule.mask_id >= rule.vocab_size || (token_bytes == 2 && rule.vocab_size > 65536u))
    throw std::runtime_error(op + ": ids outside the vocabulary");
  if (max_blocks < 0) throw std::runtime_error(op + ": negative max_blocks");
  if (B == 0) return;
  const long want = ((long)B + kMlmWaves - 1) / kMlmWaves;
  const long cap = max_blocks > 0 ? max_blocks : kMlmDefaultBlocks;
  const dim3 grid((unsigned)(want < cap ? want : cap)), block(kMlmWaves * 64);
#define DTF_MLM_LAUNCH(TOK, WORDS)                                                               \
  hipLaunchKernelGGL((mlm_mask_kernel<TOK, WORDS>), grid, block, 0, st,                           \
                     static_cast<const TOK*>(tokens), idx, input_ids, segment_ids, input_mask,   \
                     positions, ids, weights, N, B, S, P, seed, ex_stride, ex_offset, rule,      \
                     continuation)
  if (continuation == nullptr) {
    if (token_bytes == 2) DTF_MLM_LAUNCH(uint16_t, false);
    else DTF_MLM_LAUNCH(uint32_t, false);
  } else {
    if (token_bytes == 2) DTF_MLM_LAUNCH(uint16_t, true);
    else DTF_MLM_LAUNCH(uint32_t, true);
  }
#undef DTF_MLM_LAUNCH
}

void dtf_mlm_mask_tokens(const void* tokens, int token_bytes, const int64_t* idx,
                         int64_t* input_ids, int64_t* segment_ids, int64_t* input_mask,
                         int64_t* positions, int64_t* ids, float* weights, long N, int B, int S,
                         int P, uint32_t seed, long ex_stride, long ex_offset,
                         const MlmMaskRule& rule, int max_blocks, hipStream_t st) {
  mlm_mask_launch("mlm_mask_tokens", tokens, token_bytes, idx, nullptr, input_ids, segment_ids,
                  input_mask, positions, ids, weights, N, B, S, P, seed, ex_stride, ex_offset, rule,
                  max_blocks, st);
}

void dtf_mlm_mask_words(const void* tokens, int token_bytes, const int64_t* idx,
                        const uint8_t* continuation, int64_t* input_ids, int64_t* segment_ids,
                        int64_t* input_mask, int64_t* positions, int64_t* ids, float* weights,
                        long N, int B, int S, int P, uint32_t seed, long ex_stride, long ex_offset,
                        const MlmMaskRule& rule, int max_blocks, hipStream_t st) {
  if (continuation == nullptr)
    throw std::runtime_error("mlm_mask_words: needs the continuation table");
  mlm_mask_launch("mlm_mask_words", tokens, token_bytes, idx, continuation, input_ids, segment_ids,
                  input_mask, positions, ids, weights, N, B, S, P, seed, ex_stride, ex_offset, rule,
                  max_blocks, st);
}
