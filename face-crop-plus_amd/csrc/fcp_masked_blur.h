// The mask-normalised Gaussian of uint8 RGB crops, once for fcp_matte_blur.hip (one side: the background of the hard
// mask) and fcp_cutout.hip (two sides: alpha == 255 and alpha == 0).  A side is an indicator s(p) in {0, 1}; a pixel is
// on at most one side:
//
//   t[0..r]   : all >= 1, t[0] + 2 sum(t[1..r]) == 4096, 3 <= r <= 48; made on the host from sigma, data here
//   D(y,x)    = sum_j sum_i t|j| t|i| s(y+j, x+i)                                          taps inside the image only
//   N_ch(y,x) = sum_j sum_i t|j| t|i| s(y+j, x+i) c_ch(y+j, x+i)                           the same taps
//   B_ch(y,x) = D > 0 ? (N_ch + D / 2) / D : c_ch(y,x)                                     integer division: normalised()
//
// Positions outside the image contribute to neither N nor D: the normalisation is the border rule.  Bounds, all in
// unsigned 32 bits: a horizontal sum is at most 255 * 4096 < 2^20; N <= 255 * 4096^2 = 4 278 190 080 < 2^32 and
// N + D / 2 <= 4 286 578 688 < 2^32, only just, which is why load_taps refuses taps that do not sum to 4096; N <= 255 D,
// so B <= 255.  Every tap is >= 1, so D > 0 wherever the window holds a pixel of the side.
//
// Two passes through a workspace of Sides x 16 bytes per pixel, side 0 first, workgroups of kThreads lanes:
//
//   rows_pass, (kRowTileH rows x kRowTileW columns, face): stages Sides dwords per pixel of its rows and an r-pixel
//   margin, (s, s c_r, s c_g, s c_b) as four bytes, zero off the side and outside the image, so the border rule and the
//   indicator cost nothing in the loop; then a lane per output pixel runs the 2 r + 1 taps over consecutive entries
//   (consecutive lanes, consecutive banks) and stores Sides x (H_s, H_r, H_g, H_b) as 16-byte stores.  The tap table is
//   mirrored to 2 r + 1 entries, so the loop has no |k|.
//
//   stage_cols / cols_taps, the pieces of a columns pass whose tile, LDS plan and epilogue are its file's: the 16-byte
//   sums of TileW columns for rows y0 - r .. y0 + nrows + r - 1 at a pitch of the caller's, zero outside the image; then
//   the 2 r + 1 taps down the four pixels of a lane's group into dn[pixel][4 side + (0: D, 1..3: N)].
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "fcp_common.h"

namespace fcp_masked_blur {

constexpr int kThreads = 256;
constexpr int kMinRadius = 3;
constexpr int kMaxRadius = 48;
constexpr uint32_t kTapSum = 4096;
constexpr int kRowTileW = 256;
constexpr int kRowTileH = 4;
constexpr int kRowPitch = kRowTileW + 2 * kMaxRadius;   // entries of a staged row
constexpr size_t kTapBytes = (2 * kMaxRadius + 1) * sizeof(uint32_t);   // of LDS: the mirrored tap table

struct Taps {
  uint16_t t[kMaxRadius + 1];           // 49 x 16 bit in the kernel argument block
};

// taps[0..radius] of an entry point `who`, kMinRadius <= radius <= kMaxRadius: the 32-bit sums above hold because of this.
inline int load_taps(const char* who, const uint16_t* taps, int radius, Taps* t) {
  FCP_REQUIRE(taps != nullptr, "%s: null taps", who);
  uint32_t total = 0;
  for (int k = 0; k <= radius; ++k) {
    FCP_REQUIRE(taps[k] >= 1, "%s: tap %d is 0: every tap must be at least 1", who, k);
    t->t[k] = taps[k];
    total += (k == 0 ? 1u : 2u) * taps[k];
  }
  FCP_REQUIRE(total == kTapSum, "%s: the taps must sum to %u over the window (got %u)", who, kTapSum, total);
  return 0;
}

// the mirrored tap table, 2 r + 1 dwords: entry k is t|k - r|
__device__ __forceinline__ void stage_taps(uint32_t* tl, const Taps& taps, int radius) {
  const int k = threadIdx.x;
  if (k <= 2 * radius) tl[k] = taps.t[k < radius ? radius - k : k - radius];
}

// B of one channel: the normalised sum, the crop's colour where the window saw no pixel of the side
__device__ __forceinline__ uint32_t normalised(uint32_t n, uint32_t d, uint32_t c) { return d > 0u ? (n + (d >> 1)) / d : c; }

// a staged pixel: (s, s c_r, s c_g, s c_b) as four bytes, one dword per side
template <int Sides>
using Staged = std::conditional_t<Sides == 1, uint32_t, uint2>;
__device__ __forceinline__ uint32_t side0(uint32_t v) { return v; }
__device__ __forceinline__ uint32_t side0(uint2 v) { return v.x; }

// the four horizontal sums of one side, each <= 255 * 4096
struct SideSums {
  uint32_t s = 0u, r = 0u, g = 0u, b = 0u;
  __device__ __forceinline__ void add(uint32_t t, uint32_t v) {
    s += t * (v & 255u);
    r += t * ((v >> 8) & 255u);
    g += t * ((v >> 16) & 255u);
    b += t * (v >> 24);
  }
  __device__ __forceinline__ uint4 sums() const { return make_uint4(s, r, g, b); }
};

template <int Sides>
constexpr size_t rows_lds_bytes() {
  return (size_t)kRowTileH * kRowPitch * sizeof(Staged<Sides>) + kTapBytes;
}

// The rows pass of a kernel launched over (cdiv(w, kRowTileW) * cdiv(h, kRowTileH), f) with rows_lds_bytes<Sides>() of
// dynamic LDS.  side_of(byte of plane) is the pixel's side, 0 .. Sides - 1, or negative for none.
template <int Sides, class SideOf>
__device__ __forceinline__ void rows_pass(const uint8_t* __restrict__ crops, const uint8_t* __restrict__ plane, int h, int w,
                                          int tiles_x, const Taps& taps, int radius, uint4* __restrict__ sums, SideOf side_of) {
  static_assert(Sides == 1 || Sides == 2, "one side or two");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  Staged<Sides>* stage = reinterpret_cast<Staged<Sides>*>(smem);   // kRowTileH rows of kRowPitch entries
  uint32_t* tl = reinterpret_cast<uint32_t*>(stage + kRowTileH * kRowPitch);
  const int f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kRowTileW, y0 = ty * kRowTileH;
  const int nrows = min(kRowTileH, h - y0), ncols = min(kRowTileW, w - x0);
  const int span = ncols + 2 * radius;

  stage_taps(tl, taps, radius);
  for (int i = threadIdx.x; i < nrows * span; i += kThreads) {
    const int tr = i / span, d = i - tr * span;
    const int x = x0 - radius + d;
    Staged<Sides> v = Staged<Sides>();
    if (x >= 0 && x < w) {
      const size_t pixel = ((size_t)f * h + (y0 + tr)) * w + x;
      const int side = side_of((uint32_t)plane[pixel]);
      if (side >= 0) {
        const uint8_t* c = crops + pixel * 3;
        const uint32_t e = 1u | ((uint32_t)c[0] << 8) | ((uint32_t)c[1] << 16) | ((uint32_t)c[2] << 24);
        if constexpr (Sides == 1) v = e;
        else v = side == 0 ? make_uint2(e, 0u) : make_uint2(0u, e);
      }
    }
    stage[tr * kRowPitch + d] = v;
  }
  __syncthreads();

  for (int i = threadIdx.x; i < nrows * ncols; i += kThreads) {
    const int tr = i / ncols, cx = i - tr * ncols;
    const Staged<Sides>* s = stage + tr * kRowPitch + cx;   // output x sums staged x .. x + 2 r
    SideSums a, b;                                          // side 0, side 1
    for (int k = 0; k <= 2 * radius; ++k) {
      const Staged<Sides> v = s[k];
      const uint32_t t = tl[k];
      a.add(t, side0(v));
      if constexpr (Sides == 2) b.add(t, v.y);
    }
    uint4* o = sums + Sides * (((size_t)f * h + (y0 + tr)) * w + (x0 + cx));
    o[0] = a.sums();
    if constexpr (Sides == 2) o[1] = b.sums();
  }
}

// The sums of rows y0 - r .. y0 + nrows + r - 1, TileW columns from x0, into col at Pitch uint4 a staged row
// (Pitch >= Sides * TileW): zero outside the image.  All lanes of the workgroup call it.
template <int Sides, int TileW, int Pitch>
__device__ __forceinline__ void stage_cols(uint4* col, const uint4* __restrict__ sums, int f, int h, int w, int x0, int y0,
                                           int nrows, int radius) {
  constexpr int kRow = Sides * TileW;
  for (int i = threadIdx.x; i < (nrows + 2 * radius) * kRow; i += kThreads) {
    const int tr = i / kRow, q = i - tr * kRow;
    const int y = y0 - radius + tr, x = x0 + q / Sides;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (y >= 0 && y < h && x < w) v = sums[Sides * (((size_t)f * h + y) * w + x) + q % Sides];
    col[tr * Pitch + q] = v;
  }
}

// D and N of the four pixels of group g of tile row r, every side, from col as stage_cols left it (a group's entries
// start at 4 Sides g of a staged row); dn is zero on entry.  N + D / 2 < 2^32.
template <int Sides, int Pitch>
__device__ __forceinline__ void cols_taps(const uint4* col, const uint32_t* tl, int radius, int r, int g, uint32_t dn[4][4 * Sides]) {
  for (int k = 0; k <= 2 * radius; ++k) {
    const uint32_t t = tl[k];
    const uint4* p = col + (r + k) * Pitch + 4 * Sides * g;
#pragma unroll
    for (int j = 0; j < 4 * Sides; ++j) {       // pixel j / Sides, side j % Sides
      const uint4 v = p[j];
      uint32_t* d = dn[j / Sides] + 4 * (j % Sides);
      d[0] += t * v.x;
      d[1] += t * v.y;
      d[2] += t * v.z;
      d[3] += t * v.w;
    }
  }
}

}  // namespace fcp_masked_blur
