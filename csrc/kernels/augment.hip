// Fused on-device image augmentation for HBM-resident uint8 image sets (data/images.py): one
// launch turns a batch of example indices into the model's input,
//   gather -> crop box (random-resized-crop / pad-crop / centre) -> bilinear resize -> flip ->
//   per-channel normalisation -> bf16 / fp32 NHWC.
//
// The sampling rule is integer arithmetic (ops/reference.py augment_images is the same rule in
// torch and the tests' oracle; the two agree to the bit).  For output pixel (b, oy, ox):
//   ox' = flip[b] ? Wo - 1 - ox : ox
//   per axis, half-pixel centres with 8 fractional bits:
//     pos = floor((2 o + 1) * side * 256 / (2 O)) - 128, clamped to [0, (side - 1) * 256]
//     i0 = pos >> 8, f = pos & 255, i1 = min(i0 + 1, side - 1)
//   taps (y0 + iy, x0 + ix); a tap outside the image reads `fill`
//   v = ((256 - fy) * ((256 - fx) * p00 + fx * p01) + fy * ((256 - fx) * p10 + fx * p11)
//        + 32768) >> 16
//   out = lut[c][v]          (the host builds (v / 255 - mean_c) / std_c in the output dtype)
//
// Mapping: a block takes one (example, tile of 16 output rows, chunk of 256 output columns) at a
// time and grid-strides over those.  It first fills two small LDS tables -- per output column of
// the chunk and per output row of the tile: the two tap offsets, the weight and whether each tap
// is inside the image -- so the divisions of the rule are paid once per row / column, not once
// per pixel.  Its threads then each produce G consecutive elements of one output row: where
// Wo * C % 8 == 0, 8 whole pixels (G = 8 C, written as 16-B stores; each tap is one load of the
// pixel's C bytes), otherwise G = 1 (the scalar tail path, one byte per tap).  Consecutive lanes
// take consecutive groups of a row, so a wave's stores are one contiguous run and its taps fall
// in the same two source rows.  The example is uniform over
// the block, so taps are 32-bit offsets from one scalar image base.  The normalisation table
// (<= 3 KB) is staged in LDS once per block.
#include <stdexcept>

#include "launch.h"

namespace {
constexpr int kAugThreads = 256;
constexpr int kAugRows = 16;             // output rows per tile
constexpr int kAugCols = 256;            // output columns per chunk (a multiple of 8)
constexpr int kAugDefaultBlocks = 2048;
constexpr int kAugTap0 = 256, kAugTap1 = 512;     // table flags: tap 0 / tap 1 inside the image

struct AugAxis {
  int i0, i1, f;
};

// pos of output coordinate o of O over a box side of `side` source pixels
DTF_DEV AugAxis aug_axis(int o, int O, int side) {
  const uint64_t num = (uint64_t)(2 * o + 1) * (uint64_t)(side > 0 ? side : 0) * 256u;
  const uint32_t den = 2u * (uint32_t)O;
  // the 32-bit divide covers every practical shape; the 64-bit one keeps huge boxes exact
  const int64_t q = (num >> 32) == 0 ? (int64_t)((uint32_t)num / den) : (int64_t)(num / den);
  const int64_t hi = ((int64_t)side - 1) * 256;
  int64_t pos = q - 128;
  pos = pos < 0 ? 0 : pos;
  pos = pos > hi ? hi : pos;
  AugAxis a;
  a.i0 = (int)(pos >> 8);
  a.f = (int)(pos & 255);
  a.i1 = a.i0 + 1 < side ? a.i0 + 1 : side - 1;
  return a;
}

// One table entry of an axis: taps at (origin + i0, origin + i1) of an axis of `extent` source
// pixels, `stride` bytes apart -> byte offsets (0 for a tap outside) and weight | flags.
DTF_DEV void aug_entry(int o, int O, int side, int origin, int extent, int stride, int* off0,
                       int* off1, int* wf) {
  const AugAxis a = aug_axis(o, O, side);
  const int64_t t0 = (int64_t)origin + a.i0, t1 = (int64_t)origin + a.i1;
  const bool ok0 = t0 >= 0 && t0 < extent, ok1 = t1 >= 0 && t1 < extent;
  *off0 = ok0 ? (int)t0 * stride : 0;
  *off1 = ok1 ? (int)t1 * stride : 0;
  *wf = a.f | (ok0 ? kAugTap0 : 0) | (ok1 ? kAugTap1 : 0);
}

DTF_DEV int aug_blend(int p00, int p01, int p10, int p11, int fx, int fy) {
  const int top = (256 - fx) * p00 + fx * p01, bot = (256 - fx) * p10 + fx * p11;
  return ((256 - fy) * top + fy * bot + 32768) >> 16;
}

// The C channel bytes of the pixel at byte `off` of an image, in the low bytes of one word.  For
// C = 3 that is one (unaligned) 4-byte load; it reads one byte past the pixel, so at the image's
// last pixel it is taken 1 byte lower (`last4` = image bytes - 4) and shifted back.
template <int C>
DTF_DEV uint32_t aug_tap(const uint8_t* __restrict__ img, uint32_t off, uint32_t last4) {
  if constexpr (C == 1) {
    return img[off];
  } else {
    const uint32_t at = off < last4 ? off : last4;
    uint32_t w;
    __builtin_memcpy(&w, img + at, 4);
    return w >> (8 * (off - at));
  }
}

template <typename OutT, int C, int G>
__global__ void __launch_bounds__(kAugThreads)
augment_kernel(const uint8_t* __restrict__ images, const int64_t* __restrict__ idx,
               const int* __restrict__ boxes, const uint8_t* __restrict__ flip,
               const OutT* __restrict__ lut, OutT* __restrict__ out, long N, int B, int Hs, int Ws,
               int Ho, int Wo, int fill, int tiles, int chunks) {
  __shared__ OutT s_lut[C * 256];
  __shared__ int s_x0[kAugCols], s_x1[kAugCols], s_xf[kAugCols];
  __shared__ int s_y0[kAugRows], s_y1[kAugRows], s_yf[kAugRows];
  const int tid = threadIdx.x;
  for (int i = tid; i < C * 256; i += kAugThreads) s_lut[i] = lut[i];

  const uint32_t per_b = (uint32_t)tiles * (uint32_t)chunks;
  const uint32_t items = (uint32_t)B * per_b;                        // < 2^31: launcher
  const int64_t row_elems = (int64_t)Wo * C;
  const uint32_t last4 = (uint32_t)(Hs * Ws * C - 4);               // vector path: >= 0, launcher
  const uint32_t fillw = (uint32_t)fill * 0x010101u;
  for (uint32_t u = blockIdx.x; u < items; u += gridDim.x) {
    const int b = (int)(u / per_b);
    const int rem = (int)(u - (uint32_t)b * per_b);
    const int tile = rem / chunks, chunk = rem - tile * chunks;
    const int oy0 = tile * kAugRows, px0 = chunk * kAugCols;
    const int rows = Ho - oy0 < kAugRows ? Ho - oy0 : kAugRows;
    const int cols = Wo - px0 < kAugCols ? Wo - px0 : kAugCols;
    const int y0 = boxes[4 * b], x0 = boxes[4 * b + 1], bh = boxes[4 * b + 2],
              bw = boxes[4 * b + 3];
    const bool fl = flip[b] != 0;
    const int64_t n = idx[b];
    const bool img_ok = n >= 0 && n < N;           // a bad index reads as fill, never past the set
    const uint8_t* img = images + (img_ok ? n : 0) * ((int64_t)Hs * Ws * C);   // block-uniform

    __syncthreads();                 // the previous item's table reads (and the LUT staging)
    if (tid < cols) {
      const int ox = px0 + tid;
      aug_entry(fl ? Wo - 1 - ox : ox, Wo, bw, x0, Ws, C, &s_x0[tid], &s_x1[tid], &s_xf[tid]);
    }
    if (tid < rows) {
      int wf;
      aug_entry(oy0 + tid, Ho, bh, y0, Hs, Ws * C, &s_y0[tid], &s_y1[tid], &wf);
      s_yf[tid] = img_ok ? wf : (wf & 255);
    }
    __syncthreads();

    const int g0 = px0 * C / G, gpc = cols * C / G;       // this chunk's groups of a row
    const float inv_gpc = 1.0f / (float)gpc;
    for (int k = tid; k < rows * gpc; k += kAugThreads) {
      int r = (int)(((float)k + 0.5f) * inv_gpc);          // k / gpc, r < 16: fixed up below
      r = r * gpc > k ? r - 1 : r;
      r = (r + 1) * gpc <= k ? r + 1 : r;
      const int g = k - r * gpc;
      const uint32_t ro0 = (uint32_t)s_y0[r], ro1 = (uint32_t)s_y1[r];
      const int yf = s_yf[r], fy = yf & 255;
      const bool r0_ok = (yf & kAugTap0) != 0, r1_ok = (yf & kAugTap1) != 0;

      OutT res[G];
      if constexpr (G == 1) {
        // tail path: one element; offsets of taps outside the image are 0, so every load is
        // inside the image
        const int pi = g / C, c = g - pi * C, xf = s_xf[pi], fx = xf & 255;
        const uint32_t o0 = (uint32_t)s_x0[pi], o1 = (uint32_t)s_x1[pi];
        const bool c0_ok = (xf & kAugTap0) != 0, c1_ok = (xf & kAugTap1) != 0;
        const int v00 = img[ro0 + o0 + c], v01 = img[ro0 + o1 + c];
        const int v10 = img[ro1 + o0 + c], v11 = img[ro1 + o1 + c];
        const int p00 = r0_ok && c0_ok ? v00 : fill, p01 = r0_ok && c1_ok ? v01 : fill;
        const int p10 = r1_ok && c0_ok ? v10 : fill, p11 = r1_ok && c1_ok ? v11 : fill;
        res[0] = s_lut[c * 256 + aug_blend(p00, p01, p10, p11, fx, fy)];
      } else {
        // vector path: 8 whole pixels; each tap is ONE load of the pixel's channels
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          const int pi = g * 8 + p, xf = s_xf[pi], fx = xf & 255;
          const uint32_t o0 = (uint32_t)s_x0[pi], o1 = (uint32_t)s_x1[pi];
          const bool c0_ok = (xf & kAugTap0) != 0, c1_ok = (xf & kAugTap1) != 0;
          const uint32_t w00 = r0_ok && c0_ok ? aug_tap<C>(img, ro0 + o0, last4) : fillw;
          const uint32_t w01 = r0_ok && c1_ok ? aug_tap<C>(img, ro0 + o1, last4) : fillw;
          const uint32_t w10 = r1_ok && c0_ok ? aug_tap<C>(img, ro1 + o0, last4) : fillw;
          const uint32_t w11 = r1_ok && c1_ok ? aug_tap<C>(img, ro1 + o1, last4) : fillw;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const int v = aug_blend((w00 >> (8 * c)) & 255, (w01 >> (8 * c)) & 255,
                                    (w10 >> (8 * c)) & 255, (w11 >> (8 * c)) & 255, fx, fy);
            res[p * C + c] = s_lut[c * 256 + v];
          }
        }
      }

      OutT* dst = out + ((int64_t)b * Ho + oy0 + r) * row_elems + (int64_t)(g0 + g) * G;
      if constexpr (G == 1) {
        dst[0] = res[0];
      } else if constexpr (sizeof(OutT) == 2) {
#pragma unroll
        for (int q = 0; q < G / 8; ++q) {
          const OutT* h = res + 8 * q;
          uint4 w;                     // the table already holds bf16 bits: pack them as they are
          w.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
          w.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
          w.z = (uint32_t)h[4] | ((uint32_t)h[5] << 16);
          w.w = (uint32_t)h[6] | ((uint32_t)h[7] << 16);
          reinterpret_cast<uint4*>(dst)[q] = w;
        }
      } else {
#pragma unroll
        for (int q = 0; q < G / 4; ++q)
          reinterpret_cast<float4*>(dst)[q] =
              make_float4(res[4 * q], res[4 * q + 1], res[4 * q + 2], res[4 * q + 3]);
      }
    }
  }
}

template <typename OutT, int C>
void launch_augment(const uint8_t* images, const int64_t* idx, const int* boxes,
                    const uint8_t* flip, const void* lut, void* out, long N, int B, int Hs, int Ws,
                    int Ho, int Wo, int fill, int max_blocks, hipStream_t st) {
  // vector path: Wo % 8 == 0 (what Wo * C % 8 == 0 means for C in {1, 3}), so a chunk holds whole
  // groups of 8 pixels; an image of under 4 bytes has no room for the 4-byte tap load
  const bool vec = (Wo * C) % 8 == 0 && (long)Hs * Ws * C >= 4;
  const int tiles = (Ho + kAugRows - 1) / kAugRows, chunks = (Wo + kAugCols - 1) / kAugCols;
  const long items = (long)B * tiles * chunks;
  if (items >= 2147483647L) throw std::runtime_error("augment_images: batch too large");
  const long cap = max_blocks > 0 ? max_blocks : kAugDefaultBlocks;
  const dim3 grid((unsigned)(items < cap ? items : cap)), block(kAugThreads);
  if (vec)
    hipLaunchKernelGGL((augment_kernel<OutT, C, 8 * C>), grid, block, 0, st, images, idx, boxes, flip,
                       static_cast<const OutT*>(lut), static_cast<OutT*>(out), N, B, Hs, Ws, Ho,
                       Wo, fill, tiles, chunks);
  else
    hipLaunchKernelGGL((augment_kernel<OutT, C, 1>), grid, block, 0, st, images, idx, boxes, flip,
                       static_cast<const OutT*>(lut), static_cast<OutT*>(out), N, B, Hs, Ws, Ho,
                       Wo, fill, tiles, chunks);
}

// ---- sample mixing (Mixup / CutMix) inside the same launch: dtf_augment_mix_images
//
// Row b is mixed with row p = partner[b] of the SAME batch, in the 8-bit pixel domain (the table
// is affine and the weights sum to 1, so mixing before it equals mixing after it at the source's
// precision).  With vA the rule above for row b and vB the rule for row p (its own idx, box and
// flip) at the same output pixel, q = clamp(lam_q[b], 0, 65536) and the cut box
// (oy0, ox0, h, w) of row b clipped to the output:
//   v   = vB                                             inside the box
//       = (q vA + (65536 - q) vB + 32768) >> 16          outside     (<= 65536 * 255 + 32768: int)
//   out = lut[c][v]
// A partner outside [0, B) or equal to b leaves the row unmixed (q = 65536, no box).
//
// The mapping is augment_kernel's, with a second set of axis tables and a second scalar image
// base for the partner.  Taps are issued only where their value is used: an item that no box
// reaches and whose q is 65536 fills no partner tables; a thread's group of 8 pixels reads the
// partner only if q < 65536 or the box reaches the group, and itself only if q > 0 and the box
// does not cover the group.  A group that the box edge crosses selects per pixel.
struct AugTables {
  int x0[kAugCols], x1[kAugCols], xf[kAugCols];
  int y0[kAugRows], y1[kAugRows], yf[kAugRows];
};

struct AugRow {                      // one side's row entry, read once per thread
  uint32_t ro0, ro1;
  int fy;
  bool r0_ok, r1_ok;
};

DTF_DEV AugRow aug_row(const AugTables& t, int r) {
  AugRow a;
  const int yf = t.yf[r];
  a.ro0 = (uint32_t)t.y0[r];
  a.ro1 = (uint32_t)t.y1[r];
  a.fy = yf & 255;
  a.r0_ok = (yf & kAugTap0) != 0;
  a.r1_ok = (yf & kAugTap1) != 0;
  return a;
}

// One side's tables of an item: the columns of the chunk and the rows of the tile.
DTF_DEV void aug_fill_tables(AugTables& t, int tid, int rows, int cols, int oy0, int px0,
                             const int* __restrict__ box, bool fl, bool img_ok, int Hs, int Ws,
                             int C, int Ho, int Wo) {
  if (tid < cols) {
    const int ox = px0 + tid;
    aug_entry(fl ? Wo - 1 - ox : ox, Wo, box[3], box[1], Ws, C, &t.x0[tid], &t.x1[tid],
              &t.xf[tid]);
  }
  if (tid < rows) {
    int wf;
    aug_entry(oy0 + tid, Ho, box[2], box[0], Hs, Ws * C, &t.y0[tid], &t.y1[tid], &wf);
    t.yf[tid] = img_ok ? wf : (wf & 255);
  }
}

// v of the C channels of pixel `pi` of the chunk (vector path: each tap is one load)
template <int C>
DTF_DEV void aug_pixel(const uint8_t* __restrict__ img, const AugTables& t, const AugRow& a,
                       int pi, uint32_t last4, uint32_t fillw, int* v) {
  const int xf = t.xf[pi], fx = xf & 255;
  const uint32_t o0 = (uint32_t)t.x0[pi], o1 = (uint32_t)t.x1[pi];
  const bool c0_ok = (xf & kAugTap0) != 0, c1_ok = (xf & kAugTap1) != 0;
  const uint32_t w00 = a.r0_ok && c0_ok ? aug_tap<C>(img, a.ro0 + o0, last4) : fillw;
  const uint32_t w01 = a.r0_ok && c1_ok ? aug_tap<C>(img, a.ro0 + o1, last4) : fillw;
  const uint32_t w10 = a.r1_ok && c0_ok ? aug_tap<C>(img, a.ro1 + o0, last4) : fillw;
  const uint32_t w11 = a.r1_ok && c1_ok ? aug_tap<C>(img, a.ro1 + o1, last4) : fillw;
#pragma unroll
  for (int c = 0; c < C; ++c)
    v[c] = aug_blend((w00 >> (8 * c)) & 255, (w01 >> (8 * c)) & 255, (w10 >> (8 * c)) & 255,
                     (w11 >> (8 * c)) & 255, fx, a.fy);
}

// v of channel c of pixel `pi` (tail path: one byte per tap; offsets of taps outside are 0)
DTF_DEV int aug_elem(const uint8_t* __restrict__ img, const AugTables& t, const AugRow& a, int pi,
                     int c, int fill) {
  const int xf = t.xf[pi], fx = xf & 255;
  const uint32_t o0 = (uint32_t)t.x0[pi], o1 = (uint32_t)t.x1[pi];
  const bool c0_ok = (xf & kAugTap0) != 0, c1_ok = (xf & kAugTap1) != 0;
  const int v00 = img[a.ro0 + o0 + c], v01 = img[a.ro0 + o1 + c];
  const int v10 = img[a.ro1 + o0 + c], v11 = img[a.ro1 + o1 + c];
  const int p00 = a.r0_ok && c0_ok ? v00 : fill, p01 = a.r0_ok && c1_ok ? v01 : fill;
  const int p10 = a.r1_ok && c0_ok ? v10 : fill, p11 = a.r1_ok && c1_ok ? v11 : fill;
  return aug_blend(p00, p01, p10, p11, fx, a.fy);
}

DTF_DEV int aug_mix(int va, int vb, int q, bool inside) {
  return inside ? vb : (q * va + (65536 - q) * vb + 32768) >> 16;
}

template <typename OutT, int C, int G>
__global__ void __launch_bounds__(kAugThreads)
augment_mix_kernel(const uint8_t* __restrict__ images, const int64_t* __restrict__ idx,
                   const int* __restrict__ boxes, const uint8_t* __restrict__ flip,
                   const OutT* __restrict__ lut, const int* __restrict__ partner,
                   const int* __restrict__ lam_q, const int* __restrict__ cut,
                   OutT* __restrict__ out, long N, int B, int Hs, int Ws, int Ho, int Wo, int fill,
                   int tiles, int chunks) {
  __shared__ OutT s_lut[C * 256];
  __shared__ AugTables s_a, s_b;                 // row b's and its partner's
  const int tid = threadIdx.x;
  for (int i = tid; i < C * 256; i += kAugThreads) s_lut[i] = lut[i];

  const uint32_t per_b = (uint32_t)tiles * (uint32_t)chunks;
  const uint32_t items = (uint32_t)B * per_b;                        // < 2^31: launcher
  const int64_t row_elems = (int64_t)Wo * C;
  const int64_t img_bytes = (int64_t)Hs * Ws * C;
  const uint32_t last4 = (uint32_t)(Hs * Ws * C - 4);               // vector path: >= 0, launcher
  const uint32_t fillw = (uint32_t)fill * 0x010101u;
  for (uint32_t u = blockIdx.x; u < items; u += gridDim.x) {
    const int b = (int)(u / per_b);
    const int rem = (int)(u - (uint32_t)b * per_b);
    const int tile = rem / chunks, chunk = rem - tile * chunks;
    const int oy0 = tile * kAugRows, px0 = chunk * kAugCols;
    const int rows = Ho - oy0 < kAugRows ? Ho - oy0 : kAugRows;
    const int cols = Wo - px0 < kAugCols ? Wo - px0 : kAugCols;

    // the plan of row b, block-uniform: a partner outside the batch, or itself, is no partner
    const int pr = partner[b];
    const bool mixed = pr >= 0 && pr < B && pr != b;
    const int p = mixed ? pr : b;
    int q = lam_q[b];
    q = !mixed || q > 65536 ? 65536 : (q < 0 ? 0 : q);
    // the cut box clipped to the output, [cy0, cy1) x [cx0, cx1); empty: cy1 <= cy0
    int cy0 = 0, cy1 = 0, cx0 = 0, cx1 = 0;
    if (mixed && cut[4 * b + 2] > 0 && cut[4 * b + 3] > 0) {
      const int64_t y = cut[4 * b], x = cut[4 * b + 1];
      const int64_t ye = y + cut[4 * b + 2], xe = x + cut[4 * b + 3];
      cy0 = (int)(y < 0 ? 0 : (y > Ho ? Ho : y));
      cx0 = (int)(x < 0 ? 0 : (x > Wo ? Wo : x));
      cy1 = (int)(ye < 0 ? 0 : (ye > Ho ? Ho : ye));
      cx1 = (int)(xe < 0 ? 0 : (xe > Wo ? Wo : xe));
      if (cx1 <= cx0) cy1 = cy0;
    }
    const bool box_here = cy0 < oy0 + rows && cy1 > oy0 && cx0 < px0 + cols && cx1 > px0 &&
                          cy1 > cy0;
    const bool need_b = q < 65536 || box_here;   // block-uniform

    // the partner's index hangs on partner[b]: a second load latency, paid only where it is used
    const int64_t na = idx[b], nb = need_b ? idx[p] : na;
    const bool a_ok = na >= 0 && na < N, b_ok = nb >= 0 && nb < N;   // a bad index reads as fill
    const uint8_t* img_a = images + (a_ok ? na : 0) * img_bytes;     // block-uniform
    const uint8_t* img_b = images + (b_ok ? nb : 0) * img_bytes;

    __syncthreads();                 // the previous item's table reads (and the LUT staging)
    aug_fill_tables(s_a, tid, rows, cols, oy0, px0, boxes + 4 * b, flip[b] != 0, a_ok, Hs, Ws, C,
                    Ho, Wo);
    if (need_b)
      aug_fill_tables(s_b, tid, rows, cols, oy0, px0, boxes + 4 * p, flip[p] != 0, b_ok, Hs, Ws,
                      C, Ho, Wo);
    __syncthreads();

    const int g0 = px0 * C / G, gpc = cols * C / G;       // this chunk's groups of a row
    const float inv_gpc = 1.0f / (float)gpc;
    for (int k = tid; k < rows * gpc; k += kAugThreads) {
      int r = (int)(((float)k + 0.5f) * inv_gpc);          // k / gpc, r < 16: fixed up below
      r = r * gpc > k ? r - 1 : r;
      r = (r + 1) * gpc <= k ? r + 1 : r;
      const int g = k - r * gpc;
      const int oy = oy0 + r;
      const bool in_y = oy >= cy0 && oy < cy1;
      const AugRow ra = aug_row(s_a, r);
      AugRow rb = ra;
      if (need_b) rb = aug_row(s_b, r);

      OutT res[G];
      if constexpr (G == 1) {
        const int pi = g / C, c = g - pi * C, ox = px0 + pi;
        const bool inside = in_y && ox >= cx0 && ox < cx1;
        const bool use_a = !inside && q > 0, use_b = inside || q < 65536;
        const int va = use_a ? aug_elem(img_a, s_a, ra, pi, c, fill) : 0;
        const int vb = use_b ? aug_elem(img_b, s_b, rb, pi, c, fill) : 0;
        res[0] = s_lut[c * 256 + aug_mix(va, vb, q, inside)];
      } else {
        // the box's columns inside this group of 8 pixels: [lo, hi)
        const int gx = px0 + g * 8;
        const int lo = cx0 > gx ? cx0 : gx, hi = cx1 < gx + 8 ? cx1 : gx + 8;
        const int n_in = in_y && hi > lo ? hi - lo : 0;
        const bool use_a = n_in < 8 && q > 0, use_b = n_in > 0 || q < 65536;
#pragma unroll
        for (int px = 0; px < 8; ++px) {
          const int pi = g * 8 + px;
          const bool inside = n_in > 0 && gx + px >= lo && gx + px < hi;
          int va[C], vb[C];
#pragma unroll
          for (int c = 0; c < C; ++c) va[c] = vb[c] = 0;
          if (use_a) aug_pixel<C>(img_a, s_a, ra, pi, last4, fillw, va);
          if (use_b) aug_pixel<C>(img_b, s_b, rb, pi, last4, fillw, vb);
#pragma unroll
          for (int c = 0; c < C; ++c)
            res[px * C + c] = s_lut[c * 256 + aug_mix(va[c], vb[c], q, inside)];
        }
      }

      OutT* dst = out + ((int64_t)b * Ho + oy) * row_elems + (int64_t)(g0 + g) * G;
      if constexpr (G == 1) {
        dst[0] = res[0];
      } else if constexpr (sizeof(OutT) == 2) {
#pragma unroll
        for (int w4 = 0; w4 < G / 8; ++w4) {
          const OutT* h = res + 8 * w4;
          uint4 w;                     // the table already holds bf16 bits: pack them as they are
          w.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
          w.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
          w.z = (uint32_t)h[4] | ((uint32_t)h[5] << 16);
          w.w = (uint32_t)h[6] | ((uint32_t)h[7] << 16);
          reinterpret_cast<uint4*>(dst)[w4] = w;
        }
      } else {
#pragma unroll
        for (int w4 = 0; w4 < G / 4; ++w4)
          reinterpret_cast<float4*>(dst)[w4] =
              make_float4(res[4 * w4], res[4 * w4 + 1], res[4 * w4 + 2], res[4 * w4 + 3]);
      }
    }
  }
}

template <typename OutT, int C>
void launch_augment_mix(const uint8_t* images, const int64_t* idx, const int* boxes,
                        const uint8_t* flip, const void* lut, const int* partner,
                        const int* lam_q, const int* cut, void* out, long N, int B, int Hs, int Ws,
                        int Ho, int Wo, int fill, int max_blocks, hipStream_t st) {
  const bool vec = (Wo * C) % 8 == 0 && (long)Hs * Ws * C >= 4;      // as launch_augment
  const int tiles = (Ho + kAugRows - 1) / kAugRows, chunks = (Wo + kAugCols - 1) / kAugCols;
  const long items = (long)B * tiles * chunks;
  if (items >= 2147483647L) throw std::runtime_error("augment_mix_images: batch too large");
  const long cap = max_blocks > 0 ? max_blocks : kAugDefaultBlocks;
  const dim3 grid((unsigned)(items < cap ? items : cap)), block(kAugThreads);
  if (vec)
    hipLaunchKernelGGL((augment_mix_kernel<OutT, C, 8 * C>), grid, block, 0, st, images, idx,
                       boxes, flip, static_cast<const OutT*>(lut), partner, lam_q, cut,
                       static_cast<OutT*>(out), N, B, Hs, Ws, Ho, Wo, fill, tiles, chunks);
  else
    hipLaunchKernelGGL((augment_mix_kernel<OutT, C, 1>), grid, block, 0, st, images, idx, boxes,
                       flip, static_cast<const OutT*>(lut), partner, lam_q, cut,
                       static_cast<OutT*>(out), N, B, Hs, Ws, Ho, Wo, fill, tiles, chunks);
}
// ---- RandAugment inside the same launch: dtf_augment_rand_images
//
// Each row carries an output -> input affine map in Q16, aff = (a, b, c, d, e, f), and a chain of
// L <= 4 pointwise ops (pops, ppar).  With V_b(v, u) the rule above for row b at output pixel
// (oy = v, ox = u) (the row's "virtual image"), output pixel (b, oy, ox) is
//   U = a (2 ox + 1) + b (2 oy + 1) + 2 c,  W = d (2 ox + 1) + e (2 oy + 1) + 2 f      (int64)
//   u = U >> 17, v = W >> 17                           (PIL's nearest neighbour on pixel centres)
//   x = V_b(v, u) if 0 <= u < Wo and 0 <= v < Ho else ra_fill
//   x = op_k(x) for k = 0 .. L - 1:  1 Invert 255 - x;  2 Solarize x < m ? x : 255 - x;
//       3 SolarizeAdd x < 128 ? min(255, x + m) : x;  4 Posterize x & m;
//       5 Brightness clamp((x m) >> 16);  6 Color (C = 3) clamp((65536 g + m (x - g)) >> 16) with
//       g = (19595 x0 + 38470 x1 + 7471 x2 + 32768) >> 16;  any other code: x
// then the mix of augment_mix_kernel (the partner's row under its OWN map and chain), then lut.
// ops/reference.py augment_rand_images is the same rule and the tests' oracle.
//
// A pixel's (u, v) is its own, so the axis tables cover ALL Wo columns and ALL Ho rows of the
// virtual image (Ho, Wo <= 1024: 16 KB per side, an entry packed into two words), refilled per
// item: the rule's divisions are still paid per row and column, and a pixel looks up x[u], y[v].
// A row whose map is the identity fills only its chunk's columns and its tile's rows and skips
// the map (the separable path).  As in augment_mix_kernel a side that is not used issues no
// taps, and neither does a pixel that the map sends outside the virtual image.  The chain's
// branches are block-uniform.  Parameters are clamped to their ranges when the plan is read, so
// every value stays a byte whatever the plan holds.  The tail path makes one whole pixel per
// thread (Color needs the three channels).
constexpr int kRandMax = 1024;                    // Ho, Wo limit: the tables' length
constexpr int kRandLayers = 4;
constexpr int kAugStep = 1024;                    // table flag: tap 1 lies one stride after tap 0

struct RandTables {                               // .x: tap 0's byte offset, .y: weight | flags
  int2 x[kRandMax], y[kRandMax];
};

DTF_DEV int2 rand_entry(int o, int O, int side, int origin, int extent, int stride) {
  const AugAxis a = aug_axis(o, O, side);
  const int64_t t0 = (int64_t)origin + a.i0, t1 = (int64_t)origin + a.i1;
  const bool ok0 = t0 >= 0 && t0 < extent, ok1 = t1 >= 0 && t1 < extent;
  int2 e;
  // tap 1 is tap 0 or the next pixel; where only tap 1 is inside it is pixel 0, offset 0
  e.x = ok0 ? (int)t0 * stride : 0;
  e.y = a.f | (ok0 ? kAugTap0 : 0) | (ok1 ? kAugTap1 : 0) |
        (ok0 && ok1 && t1 != t0 ? kAugStep : 0);
  return e;
}

// One side's tables: columns [c_lo, c_lo + c_n) and rows [r_lo, r_lo + r_n) of the virtual image.
DTF_DEV void rand_fill_tables(RandTables& t, int tid, int r_lo, int r_n, int c_lo, int c_n,
                              const int* __restrict__ box, bool fl, bool img_ok, int Hs, int Ws,
                              int C, int Ho, int Wo) {
  for (int i = tid; i < c_n; i += kAugThreads) {
    const int ox = c_lo + i;
    t.x[ox] = rand_entry(fl ? Wo - 1 - ox : ox, Wo, box[3], box[1], Ws, C);
  }
  for (int i = tid; i < r_n; i += kAugThreads) {
    const int oy = r_lo + i;
    int2 e = rand_entry(oy, Ho, box[2], box[0], Hs, Ws * C);
    if (!img_ok) e.y &= 255;
    t.y[oy] = e;
  }
}

struct RandPlan {                                 // one row's plan, block-uniform
  int a, b, c, d, e, f;
  int code[kRandLayers], par[kRandLayers];
  int n;                                          // layers up to the last that does something
  bool ident;
};

DTF_DEV RandPlan rand_plan(const int* __restrict__ aff, const int* __restrict__ pops,
                           const int* __restrict__ ppar, int L) {
  RandPlan p;
  p.a = aff[0]; p.b = aff[1]; p.c = aff[2]; p.d = aff[3]; p.e = aff[4]; p.f = aff[5];
  p.ident = p.a == 65536 && p.b == 0 && p.c == 0 && p.d == 0 && p.e == 65536 && p.f == 0;
  p.n = 0;
#pragma unroll
  for (int k = 0; k < kRandLayers; ++k) {
    const int code = k < L ? pops[k] : 0;
    int m = k < L ? ppar[k] : 0;
    const int hi = code == 2 ? 256 : (code == 3 ? 128 : (1 << 18));
    if (code != 4) m = m < 0 ? 0 : (m > hi ? hi : m);
    p.code[k] = code;
    p.par[k] = m;
    if (code >= 1 && code <= 6) p.n = k + 1;
  }
  return p;
}

DTF_DEV int rand_pick(const int (&a)[kRandLayers], int k) {
  return k == 0 ? a[0] : (k == 1 ? a[1] : (k == 2 ? a[2] : a[3]));
}

DTF_DEV int rand_byte(int t) { return t < 0 ? 0 : (t > 255 ? 255 : t); }

// The pointwise chain on NP pixels of C channels.
template <int C, int NP>
DTF_DEV void rand_chain(const RandPlan& p, int (*x)[C]) {
  for (int k = 0; k < p.n; ++k) {
    const int code = rand_pick(p.code, k), m = rand_pick(p.par, k);
    if (code == 1) {
#pragma unroll
      for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) x[i][c] = 255 - x[i][c];
    } else if (code == 2) {
#pragma unroll
      for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) x[i][c] = x[i][c] < m ? x[i][c] : 255 - x[i][c];
    } else if (code == 3) {
#pragma unroll
      for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int t = x[i][c] + m;
          x[i][c] = x[i][c] < 128 ? (t > 255 ? 255 : t) : x[i][c];
        }
    } else if (code == 4) {
#pragma unroll
      for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) x[i][c] &= m;
    } else if (code == 5) {
#pragma unroll
      for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) x[i][c] = rand_byte((x[i][c] * m) >> 16);   // <= 255 * 2^18
    } else if (code == 6) {
      if constexpr (C == 3) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int g = (19595 * x[i][0] + 38470 * x[i][1] + 7471 * x[i][2] + 32768) >> 16;
#pragma unroll
          for (int c = 0; c < C; ++c)
            x[i][c] = rand_byte((65536 * g + m * (x[i][c] - g)) >> 16);         // |.| < 2^27
        }
      }
    }
  }
}

// V(v, u) of the C channels, (u, v) inside the virtual image.  VEC: each tap is one load of the
// pixel's channels; otherwise one byte per tap and channel (offsets of taps outside are inside
// the image, so every load is).
template <int C, bool VEC>
DTF_DEV void rand_fetch(const uint8_t* __restrict__ img, const RandTables& t, int u, int v,
                        int ystride, uint32_t last4, uint32_t fillw, int fill, int* x) {
  const int2 ex = t.x[u], ey = t.y[v];
  const int fx = ex.y & 255, fy = ey.y & 255;
  const bool c0_ok = (ex.y & kAugTap0) != 0, c1_ok = (ex.y & kAugTap1) != 0;
  const bool r0_ok = (ey.y & kAugTap0) != 0, r1_ok = (ey.y & kAugTap1) != 0;
  const uint32_t o0 = (uint32_t)ex.x, o1 = o0 + ((ex.y & kAugStep) ? (uint32_t)C : 0u);
  const uint32_t ro0 = (uint32_t)ey.x, ro1 = ro0 + ((ey.y & kAugStep) ? (uint32_t)ystride : 0u);
  if constexpr (VEC) {
    const uint32_t w00 = r0_ok && c0_ok ? aug_tap<C>(img, ro0 + o0, last4) : fillw;
    const uint32_t w01 = r0_ok && c1_ok ? aug_tap<C>(img, ro0 + o1, last4) : fillw;
    const uint32_t w10 = r1_ok && c0_ok ? aug_tap<C>(img, ro1 + o0, last4) : fillw;
    const uint32_t w11 = r1_ok && c1_ok ? aug_tap<C>(img, ro1 + o1, last4) : fillw;
#pragma unroll
    for (int c = 0; c < C; ++c)
      x[c] = aug_blend((w00 >> (8 * c)) & 255, (w01 >> (8 * c)) & 255, (w10 >> (8 * c)) & 255,
                       (w11 >> (8 * c)) & 255, fx, fy);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int v00 = img[ro0 + o0 + c], v01 = img[ro0 + o1 + c];
      const int v10 = img[ro1 + o0 + c], v11 = img[ro1 + o1 + c];
      const int p00 = r0_ok && c0_ok ? v00 : fill, p01 = r0_ok && c1_ok ? v01 : fill;
      const int p10 = r1_ok && c0_ok ? v10 : fill, p11 = r1_ok && c1_ok ? v11 : fill;
      x[c] = aug_blend(p00, p01, p10, p11, fx, fy);
    }
  }
}

// One side's values after the map and the chain, for the NP output pixels (oy, ox .. ox + NP).
template <int C, bool VEC, int NP>
DTF_DEV void rand_side(const RandPlan& p, const uint8_t* __restrict__ img, const RandTables& t,
                       int ox, int oy, int Ho, int Wo, int ystride, uint32_t last4,
                       uint32_t fillw, int fill, int ra_fill, int (*x)[C]) {
  if (p.ident) {
#pragma unroll
    for (int i = 0; i < NP; ++i)
      rand_fetch<C, VEC>(img, t, ox + i, oy, ystride, last4, fillw, fill, x[i]);
  } else {
    // |a (2 ox + 1)| < 2^31 * 2^11: int64 holds the sums
    const int64_t X = 2 * ox + 1, Y = 2 * oy + 1;
    int64_t U = (int64_t)p.a * X + (int64_t)p.b * Y + 2 * (int64_t)p.c;
    int64_t W = (int64_t)p.d * X + (int64_t)p.e * Y + 2 * (int64_t)p.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int64_t u = U >> 17, v = W >> 17;
      if (u >= 0 && u < Wo && v >= 0 && v < Ho) {
        rand_fetch<C, VEC>(img, t, (int)u, (int)v, ystride, last4, fillw, fill, x[i]);
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) x[i][c] = ra_fill;
      }
      U += 2 * (int64_t)p.a;
      W += 2 * (int64_t)p.d;
    }
  }
  rand_chain<C, NP>(p, x);
}

template <typename OutT, int C, bool VEC, bool MIX>
__global__ void __launch_bounds__(kAugThreads)
augment_rand_kernel(const uint8_t* __restrict__ images, const int64_t* __restrict__ idx,
                    const int* __restrict__ boxes, const uint8_t* __restrict__ flip,
                    const OutT* __restrict__ lut, const int* __restrict__ aff,
                    const int* __restrict__ pops, const int* __restrict__ ppar,
                    const int* __restrict__ partner, const int* __restrict__ lam_q,
                    const int* __restrict__ cut, OutT* __restrict__ out, long N, int B, int Hs,
                    int Ws, int Ho, int Wo, int L, int fill, int ra_fill, int tiles, int chunks) {
  constexpr int NP = VEC ? 8 : 1;                // pixels per thread
  __shared__ OutT s_lut[C * 256];
  __shared__ RandTables s_t[MIX ? 2 : 1];        // row b's and, under a mix, its partner's
  RandTables& s_a = s_t[0];
  RandTables& s_b = s_t[MIX ? 1 : 0];
  const int tid = threadIdx.x;
  for (int i = tid; i < C * 256; i += kAugThreads) s_lut[i] = lut[i];

  const uint32_t per_b = (uint32_t)tiles * (uint32_t)chunks;
  const uint32_t items = (uint32_t)B * per_b;                        // < 2^31: launcher
  const int64_t row_elems = (int64_t)Wo * C;
  const int64_t img_bytes = (int64_t)Hs * Ws * C;
  const int ystride = Ws * C;
  const uint32_t last4 = (uint32_t)(Hs * Ws * C - 4);               // vector path: >= 0, launcher
  const uint32_t fillw = (uint32_t)fill * 0x010101u;
  for (uint32_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int b = (int)(it / per_b);
    const int rem = (int)(it - (uint32_t)b * per_b);
    const int tile = rem / chunks, chunk = rem - tile * chunks;
    const int oy0 = tile * kAugRows, px0 = chunk * kAugCols;
    const int rows = Ho - oy0 < kAugRows ? Ho - oy0 : kAugRows;
    const int cols = Wo - px0 < kAugCols ? Wo - px0 : kAugCols;

    // the mixing plan of row b, block-uniform, as in augment_mix_kernel
    int p = b, q = 65536;
    int cy0 = 0, cy1 = 0, cx0 = 0, cx1 = 0;
    bool need_b = false;
    if constexpr (MIX) {
      const int pr = partner[b];
      const bool mixed = pr >= 0 && pr < B && pr != b;
      p = mixed ? pr : b;
      q = lam_q[b];
      q = !mixed || q > 65536 ? 65536 : (q < 0 ? 0 : q);
      if (mixed && cut[4 * b + 2] > 0 && cut[4 * b + 3] > 0) {
        const int64_t y = cut[4 * b], x = cut[4 * b + 1];
        const int64_t ye = y + cut[4 * b + 2], xe = x + cut[4 * b + 3];
        cy0 = (int)(y < 0 ? 0 : (y > Ho ? Ho : y));
        cx0 = (int)(x < 0 ? 0 : (x > Wo ? Wo : x));
        cy1 = (int)(ye < 0 ? 0 : (ye > Ho ? Ho : ye));
        cx1 = (int)(xe < 0 ? 0 : (xe > Wo ? Wo : xe));
        if (cx1 <= cx0) cy1 = cy0;
      }
      const bool box_here = cy0 < oy0 + rows && cy1 > oy0 && cx0 < px0 + cols && cx1 > px0 &&
                            cy1 > cy0;
      need_b = q < 65536 || box_here;
    }

    const RandPlan pa = rand_plan(aff + 6 * b, pops + (int64_t)L * b, ppar + (int64_t)L * b, L);
    RandPlan pb = pa;
    if (need_b) pb = rand_plan(aff + 6 * p, pops + (int64_t)L * p, ppar + (int64_t)L * p, L);
    const int64_t na = idx[b], nb = need_b ? idx[p] : na;
    const bool a_ok = na >= 0 && na < N, b_ok = nb >= 0 && nb < N;   // a bad index reads as fill
    const uint8_t* img_a = images + (a_ok ? na : 0) * img_bytes;     // block-uniform
    const uint8_t* img_b = images + (b_ok ? nb : 0) * img_bytes;

    __syncthreads();                 // the previous item's table reads (and the LUT staging)
    rand_fill_tables(s_a, tid, pa.ident ? oy0 : 0, pa.ident ? rows : Ho, pa.ident ? px0 : 0,
                     pa.ident ? cols : Wo, boxes + 4 * b, flip[b] != 0, a_ok, Hs, Ws, C, Ho, Wo);
    if (need_b)
      rand_fill_tables(s_b, tid, pb.ident ? oy0 : 0, pb.ident ? rows : Ho, pb.ident ? px0 : 0,
                       pb.ident ? cols : Wo, boxes + 4 * p, flip[p] != 0, b_ok, Hs, Ws, C, Ho,
                       Wo);
    __syncthreads();

    const int gpc = cols / NP;                            // this chunk's groups of a row
    const float inv_gpc = 1.0f / (float)gpc;
    for (int k = tid; k < rows * gpc; k += kAugThreads) {
      int r = (int)(((float)k + 0.5f) * inv_gpc);          // k / gpc, r < 16: fixed up below
      r = r * gpc > k ? r - 1 : r;
      r = (r + 1) * gpc <= k ? r + 1 : r;
      const int g = k - r * gpc;
      const int oy = oy0 + r, gx = px0 + g * NP;
      // the box's columns inside this group of pixels: [lo, hi)
      const int lo = cx0 > gx ? cx0 : gx, hi = cx1 < gx + NP ? cx1 : gx + NP;
      const int n_in = oy >= cy0 && oy < cy1 && hi > lo ? hi - lo : 0;
      const bool use_a = n_in < NP && q > 0, use_b = n_in > 0 || q < 65536;

      int xa[NP][C], xb[NP][C];
#pragma unroll
      for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int c = 0; c < C; ++c) xa[i][c] = xb[i][c] = 0;
      if (use_a)
        rand_side<C, VEC, NP>(pa, img_a, s_a, gx, oy, Ho, Wo, ystride, last4, fillw, fill,
                              ra_fill, xa);
      if (MIX && use_b)
        rand_side<C, VEC, NP>(pb, img_b, s_b, gx, oy, Ho, Wo, ystride, last4, fillw, fill,
                              ra_fill, xb);

      OutT res[NP * C];
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const bool inside = n_in > 0 && gx + i >= lo && gx + i < hi;
#pragma unroll
        for (int c = 0; c < C; ++c)
          res[i * C + c] = s_lut[c * 256 + (MIX ? aug_mix(xa[i][c], xb[i][c], q, inside)
                                                : xa[i][c])];
      }

      OutT* dst = out + ((int64_t)b * Ho + oy) * row_elems + (int64_t)gx * C;
      if constexpr (!VEC) {
#pragma unroll
        for (int c = 0; c < C; ++c) dst[c] = res[c];
      } else if constexpr (sizeof(OutT) == 2) {
#pragma unroll
        for (int w4 = 0; w4 < C; ++w4) {
          const OutT* h = res + 8 * w4;
          uint4 w;                     // the table already holds bf16 bits: pack them as they are
          w.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
          w.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
          w.z = (uint32_t)h[4] | ((uint32_t)h[5] << 16);
          w.w = (uint32_t)h[6] | ((uint32_t)h[7] << 16);
          reinterpret_cast<uint4*>(dst)[w4] = w;
        }
      } else {
#pragma unroll
        for (int w4 = 0; w4 < 2 * C; ++w4)
          reinterpret_cast<float4*>(dst)[w4] =
              make_float4(res[4 * w4], res[4 * w4 + 1], res[4 * w4 + 2], res[4 * w4 + 3]);
      }
    }
  }
}

template <typename OutT, int C>
void launch_augment_rand(const uint8_t* images, const int64_t* idx, const int* boxes,
                         const uint8_t* flip, const void* lut, const int* aff, const int* pops,
                         const int* ppar, int L, const int* partner, const int* lam_q,
                         const int* cut, void* out, long N, int B, int Hs, int Ws, int Ho, int Wo,
                         int fill, int ra_fill, int max_blocks, hipStream_t st) {
  const bool vec = (Wo * C) % 8 == 0 && (long)Hs * Ws * C >= 4;      // as launch_augment
  const int tiles = (Ho + kAugRows - 1) / kAugRows, chunks = (Wo + kAugCols - 1) / kAugCols;
  const long items = (long)B * tiles * chunks;
  if (items >= 2147483647L) throw std::runtime_error("augment_rand_images: batch too large");
  const long cap = max_blocks > 0 ? max_blocks : kAugDefaultBlocks;
  const dim3 grid((unsigned)(items < cap ? items : cap)), block(kAugThreads);
#define DTF_RAND(VEC, MIX)                                                                      \
  hipLaunchKernelGGL((augment_rand_kernel<OutT, C, VEC, MIX>), grid, block, 0, st, images, idx, \
                     boxes, flip, static_cast<const OutT*>(lut), aff, pops, ppar, partner,      \
                     lam_q, cut, static_cast<OutT*>(out), N, B, Hs, Ws, Ho, Wo, L, fill,        \
                     ra_fill, tiles, chunks)
  if (partner != nullptr) {
    if (vec) DTF_RAND(true, true); else DTF_RAND(false, true);
  } else {
    if (vec) DTF_RAND(true, false); else DTF_RAND(false, false);
  }
#undef DTF_RAND
}
}  // namespace

void dtf_augment_images(const uint8_t* images, const int64_t* idx, const int* boxes,
                        const uint8_t* flip, const void* lut, void* out, long N, int B, int Hs,
                        int Ws, int C, int Ho, int Wo, int fill, int out_bf16, int max_blocks,
                        hipStream_t st) {
  if (C != 1 && C != 3) throw std::runtime_error("augment_images: C must be 1 or 3");
  if (N < 1 || Hs < 1 || Ws < 1) throw std::runtime_error("augment_images: empty image set");
  if (B < 0 || Ho < 1 || Wo < 1) throw std::runtime_error("augment_images: bad output shape");
  // tap offsets within one image are 32-bit (the set itself may be far larger), and 2 * o + 1
  // stays inside int
  if ((long)Hs * Ws * C > 2147483647L || Ho > (1 << 20) || Wo > (1 << 20))
    throw std::runtime_error("augment_images: one image must stay below 2 GiB");
  if (fill < 0 || fill > 255) throw std::runtime_error("augment_images: fill must be one byte");
  if (max_blocks < 0) throw std::runtime_error("augment_images: negative max_blocks");
  if (B == 0) return;
#define DTF_AUG(T, CC)                                                                          \
  launch_augment<T, CC>(images, idx, boxes, flip, lut, out, N, B, Hs, Ws, Ho, Wo, fill,         \
                        max_blocks, st)
  if (out_bf16) {
    if (C == 3) DTF_AUG(bf16_t, 3); else DTF_AUG(bf16_t, 1);
  } else {
    if (C == 3) DTF_AUG(float, 3); else DTF_AUG(float, 1);
  }
#undef DTF_AUG
}

void dtf_augment_mix_images(const uint8_t* images, const int64_t* idx, const int* boxes,
                            const uint8_t* flip, const void* lut, const int* partner,
                            const int* lam_q, const int* cut, void* out, long N, int B, int Hs,
                            int Ws, int C, int Ho, int Wo, int fill, int out_bf16, int max_blocks,
                            hipStream_t st) {
  // the same limits as dtf_augment_images
  if (C != 1 && C != 3) throw std::runtime_error("augment_mix_images: C must be 1 or 3");
  if (N < 1 || Hs < 1 || Ws < 1) throw std::runtime_error("augment_mix_images: empty image set");
  if (B < 0 || Ho < 1 || Wo < 1) throw std::runtime_error("augment_mix_images: bad output shape");
  if ((long)Hs * Ws * C > 2147483647L || Ho > (1 << 20) || Wo > (1 << 20))
    throw std::runtime_error("augment_mix_images: one image must stay below 2 GiB");
  if (fill < 0 || fill > 255) throw std::runtime_error("augment_mix_images: fill must be one byte");
  if (max_blocks < 0) throw std::runtime_error("augment_mix_images: negative max_blocks");
  if (B == 0) return;
#define DTF_AUG(T, CC)                                                                          \
  launch_augment_mix<T, CC>(images, idx, boxes, flip, lut, partner, lam_q, cut, out, N, B, Hs,  \
                            Ws, Ho, Wo, fill, max_blocks, st)
  if (out_bf16) {
    if (C == 3) DTF_AUG(bf16_t, 3); else DTF_AUG(bf16_t, 1);
  } else {
    if (C == 3) DTF_AUG(float, 3); else DTF_AUG(float, 1);
  }
#undef DTF_AUG
}

void dtf_augment_rand_images(const uint8_t* images, const int64_t* idx, const int* boxes,
                             const uint8_t* flip, const void* lut, const int* aff,
                             const int* pops, const int* ppar, int L, const int* partner,
                             const int* lam_q, const int* cut, void* out, long N, int B, int Hs,
                             int Ws, int C, int Ho, int Wo, int fill, int ra_fill, int out_bf16,
                             int max_blocks, hipStream_t st) {
  if (C != 1 && C != 3) throw std::runtime_error("augment_rand_images: C must be 1 or 3");
  if (N < 1 || Hs < 1 || Ws < 1) throw std::runtime_error("augment_rand_images: empty image set");
  if (B < 0 || Ho < 1 || Wo < 1) throw std::runtime_error("augment_rand_images: bad output shape");
  // the axis tables hold every column and row of the output
  if (Ho > kRandMax || Wo > kRandMax)
    throw std::runtime_error("augment_rand_images: output sides are at most 1024");
  if ((long)Hs * Ws * C > 2147483647L)
    throw std::runtime_error("augment_rand_images: one image must stay below 2 GiB");
  if (L < 1 || L > kRandLayers)
    throw std::runtime_error("augment_rand_images: 1 to 4 pointwise layers");
  if (fill < 0 || fill > 255 || ra_fill < 0 || ra_fill > 255)
    throw std::runtime_error("augment_rand_images: fill and ra_fill must be one byte");
  if ((partner == nullptr) != (lam_q == nullptr) || (partner == nullptr) != (cut == nullptr))
    throw std::runtime_error("augment_rand_images: partner, lam_q and cut go together");
  if (max_blocks < 0) throw std::runtime_error("augment_rand_images: negative max_blocks");
  if (B == 0) return;
#define DTF_AUG(T, CC)                                                                          \
  launch_augment_rand<T, CC>(images, idx, boxes, flip, lut, aff, pops, ppar, L, partner, lam_q, \
                             cut, out, N, B, Hs, Ws, Ho, Wo, fill, ra_fill, max_blocks, st)
  if (out_bf16) {
    if (C == 3) DTF_AUG(bf16_t, 3); else DTF_AUG(bf16_t, 1);
  } else {
    if (C == 3) DTF_AUG(float, 3); else DTF_AUG(float, 1);
  }
#undef DTF_AUG
}
