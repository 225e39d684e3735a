// Guided-filter matte edge of uint8 RGB crops (Cropper(refine=R)): the hard mask of the label
// map filtered with the crop's own gray as the guide (He, Sun, Tang), so that the alpha stays the parser's over flat
// regions and follows the image's edges where there are any.  In integers throughout; n = (2 r + 1)^2, 1 <= r <= 16:
//
//   I(y,x)  = (9798 R + 19235 G + 3735 B + 16384) >> 15            the gray of min_sharpness (fcp_sharpness.hip's gray_of)
//   p(y,x)  = m(y,x), the hard mask of fcp_feather.h (0 / 255)
//   box(v)  = sum of v over the (2 r + 1)^2 window, indices through reflect101 (fcp_feather.h), so n terms at every pixel
//   S_I, S_p, S_II, S_Ip = box(I), box(p), box(I I), box(I p)
//   cov = n S_Ip - S_I S_p       var = n S_II - S_I S_I (>= 0)       den = var + eps n n,  1 <= eps <= 4096
//   rdiv(u, d) = sign(u) ((|u| + d / 2) / d)                       nearest, ties away from zero
//   A = rdiv(4096 cov, den)                                        Q12 slope
//   B = rdiv(4096 S_p - A S_I, n)                                  Q12 offset
//   q = ((box(A) I + box(B) + 2048 n) >> 12) div n                 arithmetic shift, floor division
//   alpha = min(255, max(0, q))
//
// Widths (r = 16, n = 1089).  A row sum of 33 terms: I and the count of mask pixels fit 14 and 6 bits, I I 22 bits, and
// I p = 255 (I where p) needs only the 14-bit sum of I over the mask pixels: 56 bits, one uint2 in LDS.  Window sums:
// S_I, S_p <= 277 695 and S_II, S_Ip <= 70 812 225 are unsigned 32 bits.  With S_p = 255 k and S_Ip = 255 J (k the count, J
// the sum of I over the mask pixels of the window), cov = 255 (n J - S_I k): both products are <= 302 409 855, so the
// bracket is a signed 32-bit number and cov (|cov| < 7.8e10) a 64-bit one, as are var (< 7.8e10), den (< 1.6e11) and
// 4096 |cov| (< 3.2e14): one unsigned 64-bit division a pixel, skipped where cov == 0 (A = 0: a window inside the subject
// or inside the background).  |a| <= 127.5 / (2 sqrt(eps)) by Cauchy-Schwarz and AM-GM, so |A| <= 261 121: 32 bits.
// 4096 S_p - A S_I is 64 bits (|A S_I| < 7.3e10 < 2^37), divided by n < 2^11 as two unsigned 32-bit divisions (div_small);
// |B| < 6.8e7: 32 bits.  The pair (A, B) is one int2 of the workspace.  Second pass: a row sum of A is < 8.7e6 (25 bits
// with its sign); a row sum of B reaches 2.2e9, past 31 bits, and is a 64-bit number (34 bits with its sign): the two travel
// through LDS as one int64, rowB 2^26 + rowA, and are taken apart again before they are added up.  |box(A)| < 2.9e8 is 32
// bits, |box(B)| < 7.5e10 and box(A) I + box(B) + 2048 n are 64; after the shift the numerator is below 3.7e7 in magnitude:
// 32 bits, negative means alpha 0, otherwise one unsigned 32-bit division.  No float, no atomics.
//
// Two launches and a workspace of 8 bytes per pixel (the caller's: nothing is allocated here), both over (tile, face)
// workgroups of 256 lanes, a tile 64 x 32 pixels:
//
//   refine_ab_kernel stages (I, p) of the tile and its r-pixel halo as 16 bits a position (I, and p as one bit), the
//   reflected indices resolved while staging; runs the horizontal pass as a sliding window, a lane per (staged row, 16
//   columns), into packed row sums; then the vertical pass, a lane per (column, 8 rows), sliding too; divides and writes
//   (A, B).  LDS: (32 + 2 r) rows of ((64 + 2 r) / 2 | 1) dwords of (I, p) and of 65 x 8 B of row sums: 45 824 B at r = 16
//   (3 workgroups of the 160 KiB of a CU, 12 of 32 wave slots), 32 832 B at r = 8 (4 workgroups), 23 760 B at r = 2 (6).
//   The pitches keep the lanes of a pass, which run down the rows, on different banks: an odd number of dwords for the
//   16-bit reads, 65 x 8 B for the 8-byte stores.
//
//   refine_alpha_kernel stages (A, B) of the tile and its halo (reflected likewise) and runs the same two sliding passes.
//   A lane of the horizontal pass keeps its 16 row sums in registers until every lane has read its window, then they go
//   where the (A, B) of the same positions were, so the tile needs no second array.  Then the vertical pass, the pixel's
//   own three crop bytes, shift, divide, clamp, and the alpha byte.  LDS: (32 + 2 r) rows of ((64 + 2 r) | 1) x 8 B:
//   49 664 B at r = 16 (3 workgroups a CU), 31 104 B at r = 8 (5), 19 872 B at r = 2 (8).
//
// Bytes per pixel at r = 8: the first launch reads 4 x (80 x 48) / (64 x 32) = 7.5 (crop and label, with the halo) and
// writes 8; the second reads 8 x 1.875 = 15 of (A, B) and 3 of crop and writes 1: 34.5, against the 55.5 of the background
// blur at sigma 8.  At r = 16 the halo factor is 3: 12 + 8 + 24 + 3 + 1 = 48.
//
// The result is the same from run to run: integer sums in a fixed order, one writer per byte.  crops, labels and alpha
// may start at any byte (they are read and written as bytes here); no byte outside the arrays is touched.
//
// The composite that goes with it is in fcp_matte.hip (fcp_matte_alpha_u8) and fcp_matte_blur.hip
// (fcp_matte_blur_alpha_u8): the same kernels with the alpha read from a plane.
#include "fcp_common.h"
#include "fcp_crop_checks.h"
#include "fcp_feather.h"
#include "fcp_gray.h"
#include "fcp_hip.h"

namespace {

using namespace fcp_crop_checks;
using namespace fcp_feather;

constexpr int kThreads = 256;
constexpr int kTileW = 64;
constexpr int kTileH = 32;
constexpr int kSegW = 16;               // columns a lane of a horizontal pass slides over
constexpr int kSegH = 8;                // rows a lane of a vertical pass slides over
constexpr int kMinRadius = 1;
constexpr int kMaxRadius = 16;
constexpr int kMaxEps = 4096;
constexpr int kSumPitch = kTileW + 1;   // 8-byte row sums of a staged row

using fcp_gray::gray_of;                // the gray of min_sharpness (fcp_sharpness.hip states it itself)

// u / n for u < 2^48 and 1 <= n < 2^16, as two unsigned 32-bit divisions
__device__ __forceinline__ uint64_t div_small(uint64_t u, uint32_t n) {
  const uint32_t hi = (uint32_t)(u >> 16);
  const uint32_t q1 = hi / n, r1 = hi - q1 * n;
  const uint32_t lo = (r1 << 16) | (uint32_t)(u & 0xffffu);     // < n 2^16
  return ((uint64_t)q1 << 16) + lo / n;
}

__host__ __device__ constexpr int ab_stage_pitch(int radius) { return ((kTileW + 2 * radius) / 2) | 1; }   // dwords
__host__ __device__ constexpr int alpha_stage_pitch(int radius) { return (kTileW + 2 * radius) | 1; }      // int2

constexpr size_t ab_lds_bytes(int radius) {
  return (size_t)(kTileH + 2 * radius) * (ab_stage_pitch(radius) * sizeof(uint32_t) + kSumPitch * sizeof(uint2));
}
constexpr size_t alpha_lds_bytes(int radius) { return (size_t)(kTileH + 2 * radius) * alpha_stage_pitch(radius) * sizeof(int2); }
static_assert((kTileH + 2 * kMaxRadius) * (kTileW / kSegW) <= kThreads, "one (row, segment) of the horizontal pass a lane");
static_assert(ab_lds_bytes(kMaxRadius) == 45824 && alpha_lds_bytes(kMaxRadius) == 49664, "the LDS figures of the header");
static_assert(ab_lds_bytes(8) == 32832 && alpha_lds_bytes(8) == 31104, "the LDS figures of the header");
static_assert(ab_lds_bytes(2) == 23760 && alpha_lds_bytes(2) == 19872, "the LDS figures of the header");

// the four row sums of a window of 2 r + 1 staged positions: I (14 bits), I over the mask (14), I I (22), the mask count (6)
struct RowSums {
  uint32_t i, j, ii, k;
  __device__ __forceinline__ void add(uint32_t v) {
    const uint32_t g = v & 255u, m = v >> 8;
    i += g; j += m * g; ii += g * g; k += m;
  }
  __device__ __forceinline__ void sub(uint32_t v) {
    const uint32_t g = v & 255u, m = v >> 8;
    i -= g; j -= m * g; ii -= g * g; k -= m;
  }
  __device__ __forceinline__ uint2 pack() const { return make_uint2(i | (j << 14), ii | (k << 22)); }
};

// the window sums: S_I, J, S_II, k
struct BoxSums {
  uint32_t i, j, ii, k;
  __device__ __forceinline__ void add(uint2 v) {
    i += v.x & 0x3fffu; j += v.x >> 14; ii += v.y & 0x3fffffu; k += v.y >> 22;
  }
  __device__ __forceinline__ void sub(uint2 v) {
    i -= v.x & 0x3fffu; j -= v.x >> 14; ii -= v.y & 0x3fffffu; k -= v.y >> 22;
  }
};

__global__ void __launch_bounds__(kThreads) refine_ab_kernel(const uint8_t* __restrict__ crops, const uint8_t* __restrict__ labels,
                                                             int h, int w, int tiles_x, uint32_t bits, int radius,
                                                             unsigned long long eps_nn, int2* __restrict__ ab) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int sp = ab_stage_pitch(radius);                                     // dwords of a staged row
  uint32_t* stage32 = reinterpret_cast<uint32_t*>(smem);
  const uint16_t* stage16 = reinterpret_cast<const uint16_t*>(smem);
  uint2* hs = reinterpret_cast<uint2*>(stage32 + (kTileH + 2 * radius) * sp);   // 8-byte aligned: the row count is even
  const int f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const int nrows = min(kTileH, h - y0), ncols = min(kTileW, w - x0);
  const int srows = nrows + 2 * radius, scols = ncols + 2 * radius;
  const size_t face = (size_t)f * h * w;

  // (I, p) of rows y0 - r .. y0 + nrows + r - 1, columns x0 - r .. x0 + ncols + r - 1: two positions a dword
  const int sdw = (scols + 1) >> 1;
  for (int i = threadIdx.x; i < srows * sdw; i += kThreads) {
    const int tr = i / sdw, d = i - tr * sdw;
    const size_t row = face + (size_t)reflect101(y0 - radius + tr, h) * w;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (2 * d + j < scols) {
        const size_t pixel = row + reflect101(x0 - radius + 2 * d + j, w);
        const uint8_t* c = crops + pixel * 3;
        v |= (gray_of(c[0], c[1], c[2]) | ((mask_of(labels[pixel], bits) & 1u) << 8)) << (16 * j);
      }
    }
    stage32[tr * sp + d] = v;
  }
  __syncthreads();

  // horizontal pass: a lane per (staged row, kSegW columns); output column c sums staged columns c .. c + 2 r
  const int segs = (ncols + kSegW - 1) / kSegW;
  for (int i = threadIdx.x; i < srows * segs; i += kThreads) {
    const int seg = i / srows, tr = i - seg * srows;
    const int c0 = seg * kSegW, nout = min(kSegW, ncols - c0);
    const uint16_t* s = stage16 + tr * (2 * sp) + c0;
    RowSums sum = {0u, 0u, 0u, 0u};
    for (int k = 0; k <= 2 * radius; ++k) sum.add(s[k]);
    uint2* o = hs + tr * kSumPitch + c0;
    for (int j = 0; j < nout; ++j) {
      o[j] = sum.pack();
      if (j + 1 < nout) {
        sum.add(s[j + 1 + 2 * radius]);
        sum.sub(s[j]);
      }
    }
  }
  __syncthreads();

  // vertical pass: a lane per (column, kSegH rows); output row y sums staged rows y .. y + 2 r; then the division
  const uint32_t side = 2u * radius + 1u, n = side * side;
  for (int i = threadIdx.x; i < ncols * (kTileH / kSegH); i += kThreads) {
    const int rs = i / ncols, c = i - rs * ncols;
    const int r0 = rs * kSegH;
    if (r0 >= nrows) continue;
    const int nout = min(kSegH, nrows - r0);
    const uint2* s = hs + r0 * kSumPitch + c;
    BoxSums sum = {0u, 0u, 0u, 0u};
    for (int k = 0; k <= 2 * radius; ++k) sum.add(s[k * kSumPitch]);
    for (int j = 0; j < nout; ++j) {
      const int32_t d1 = (int32_t)(n * sum.j) - (int32_t)(sum.i * sum.k);    // cov / 255: both products <= 302 409 855
      int32_t a = 0;
      if (d1 != 0) {
        const uint64_t den = (uint64_t)n * sum.ii - (uint64_t)sum.i * sum.i + eps_nn;
        const uint64_t mag = (uint64_t)(uint32_t)(d1 < 0 ? -d1 : d1) * (255u * 4096u);
        const int32_t qa = (int32_t)((mag + (den >> 1)) / den);
        a = d1 < 0 ? -qa : qa;
      }
      const int64_t nb = (int64_t)(sum.k * (255u * 4096u)) - (int64_t)a * (int64_t)sum.i;
      const int32_t qb = (int32_t)div_small((uint64_t)(nb < 0 ? -nb : nb) + (n >> 1), n);
      ab[face + (size_t)(y0 + r0 + j) * w + (x0 + c)] = make_int2(a, nb < 0 ? -qb : qb);
      if (j + 1 < nout) {
        sum.add(s[(j + 1 + 2 * radius) * kSumPitch]);
        sum.sub(s[j * kSumPitch]);
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads) refine_alpha_kernel(const uint8_t* __restrict__ crops, const int2* __restrict__ ab,
                                                                int h, int w, int tiles_x, int radius,
                                                                uint8_t* __restrict__ alpha) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int sp = alpha_stage_pitch(radius);                                  // int2 of a staged row
  int2* stage = reinterpret_cast<int2*>(smem);
  long long* hs = reinterpret_cast<long long*>(smem);                        // the row sums, over the (A, B) they replace
  const int f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const int nrows = min(kTileH, h - y0), ncols = min(kTileW, w - x0);
  const int srows = nrows + 2 * radius, scols = ncols + 2 * radius;
  const size_t face = (size_t)f * h * w;

  for (int i = threadIdx.x; i < srows * scols; i += kThreads) {
    const int tr = i / scols, d = i - tr * scols;
    stage[tr * sp + d] = ab[face + (size_t)reflect101(y0 - radius + tr, h) * w + reflect101(x0 - radius + d, w)];
  }
  __syncthreads();

  // horizontal pass, one (staged row, kSegW columns) a lane: the row sums of A (below 2^24 in magnitude) and of B (below
  // 2^32) as rowB 2^26 + rowA, kept in registers until every window has been read
  const int segs = (ncols + kSegW - 1) / kSegW;
  const bool active = (int)threadIdx.x < srows * segs;
  const int seg = threadIdx.x / srows, tr = threadIdx.x - seg * srows;
  const int c0 = seg * kSegW, nout = active ? min(kSegW, ncols - c0) : 0;
  long long o[kSegW];
  if (active) {
    const int2* s = stage + tr * sp + c0;
    int32_t sa = 0;
    long long sb = 0;
    for (int k = 0; k <= 2 * radius; ++k) {
      const int2 v = s[k];
      sa += v.x;
      sb += v.y;
    }
#pragma unroll
    for (int j = 0; j < kSegW; ++j) {
      o[j] = sb * (1ll << 26) + sa;
      if (j + 1 < nout) {
        const int2 in = s[j + 1 + 2 * radius], out = s[j];
        sa += in.x - out.x;
        sb += (long long)in.y - out.y;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kSegW; ++j)
    if (j < nout) hs[tr * sp + c0 + j] = o[j];
  __syncthreads();

  const uint32_t side = 2u * radius + 1u, n = side * side;
  for (int i = threadIdx.x; i < ncols * (kTileH / kSegH); i += kThreads) {
    const int rs = i / ncols, c = i - rs * ncols;
    const int r0 = rs * kSegH;
    if (r0 >= nrows) continue;
    const int nout = min(kSegH, nrows - r0);
    const long long* s = hs + r0 * sp + c;
    int32_t box_a = 0;                                                       // |box(A)| < 2.9e8
    long long box_b = 0;
    auto take = [&](long long v, int sign) {
      const int32_t ra = (int32_t)((long long)((unsigned long long)v << 38) >> 38);                        // the low 26 bits with their sign
      const long long rb = (v - ra) >> 26;                                   // exact: v - ra is rowB 2^26
      box_a += sign * ra;
      box_b += sign * rb;
    };
    for (int k = 0; k <= 2 * radius; ++k) take(s[k * sp], 1);
    for (int j = 0; j < nout; ++j) {
      const size_t pixel = face + (size_t)(y0 + r0 + j) * w + (x0 + c);
      const uint8_t* cp = crops + pixel * 3;
      const long long t = (long long)box_a * (long long)gray_of(cp[0], cp[1], cp[2]) + box_b + (long long)(n * 2048u);
      const int32_t sh = (int32_t)(t >> 12);                                 // |t| < 1.5e11, so below 3.7e7 after the shift
      const uint32_t q = sh < 0 ? 0u : (uint32_t)sh / n;
      alpha[pixel] = (uint8_t)min(q, 255u);
      if (j + 1 < nout) {
        take(s[(j + 1 + 2 * radius) * sp], 1);
        take(s[j * sp], -1);
      }
    }
  }
}

}  // namespace

extern "C" int64_t fcp_matte_refine_workspace_bytes(int f, int h, int w) { return workspace_bytes(f, h, w, sizeof(int2)); }

extern "C" int fcp_matte_refine_u8(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int radius,
                                   int eps, uint8_t* alpha_out, void* workspace, int64_t workspace_bytes, fcp_stream_t stream) {
  const char* who = "matte_refine";
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_REQUIRE(radius >= kMinRadius && radius <= kMaxRadius, "matte_refine: radius must be %d..%d (got %d)", kMinRadius, kMaxRadius,
              radius);
  FCP_REQUIRE(eps >= 1 && eps <= kMaxEps, "matte_refine: eps must be 1..%d (got %d)", kMaxEps, eps);
  FCP_CHECK(check_class_bits(who, class_bits));
  if (f == 0) return 0;
  FCP_REQUIRE(crops && labels && alpha_out, "matte_refine: null pointer");
  FCP_CHECK(check_workspace(who, workspace, workspace_bytes, fcp_matte_refine_workspace_bytes(f, h, w)));
  hipStream_t s = (hipStream_t)stream;
  int2* ab = static_cast<int2*>(workspace);
  const int tiles_x = fcp_cdiv(w, kTileW), tiles_y = fcp_cdiv(h, kTileH);
  const unsigned long long n = (unsigned long long)(2 * radius + 1) * (2 * radius + 1);
  hipLaunchKernelGGL(refine_ab_kernel, dim3(tiles_x * tiles_y, f), dim3(kThreads), ab_lds_bytes(radius), s, crops, labels, h, w,
                     tiles_x, class_bits, radius, (unsigned long long)eps * n * n, ab);
  FCP_LAUNCH_OK();
  hipLaunchKernelGGL(refine_alpha_kernel, dim3(tiles_x * tiles_y, f), dim3(kThreads), alpha_lds_bytes(radius), s, crops, ab, h, w,
                     tiles_x, radius, alpha_out);
  FCP_LAUNCH_OK();
  return 0;
}
