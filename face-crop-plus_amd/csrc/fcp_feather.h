// Label map to soft alpha: the mask and its feather, once for fcp_matte.hip and fcp_matte_blur.hip, whose alphas are
// equal byte for byte because both are this code:
//
//   m(y,x)  = 255 if l(y,x) < 32 and bit l(y,x) of class_bits is set, else 0
//   k       = feather 3: (64,128,64)   5: (16,64,96,64,16)   7: (8,28,56,72,56,28,8)      each sums to 256
//   H(y,x)  = sum_i k[i] m(y, R(x+i-r, w))            r = feather / 2;  H <= 65280: 16 bits, no rounding
//   alpha   = (sum_j k[j] H(R(y+j-r, h), x) + 32768) >> 16                    feather 0: alpha = m
//   over255 = (c alpha + b (255 - alpha) + 127) / 255                          round to nearest, no ties: 255 is odd
//
// R is BORDER_REFLECT_101 iterated until the index is inside (crops smaller than the radius); the two passes restate
// cv2.GaussianBlur(m, (K,K), 0) for CV_8U.  The division is u = t + 128; (u + (u >> 8)) >> 8, equal to (t + 127) / 255 for
// every t in 0 .. 65025.
//
// Tile<R, TileW, TileH> is the feather of one TileW x TileH tile of a workgroup, four pixels of a row (a group) per lane,
// in LDS: TileH + 2 R rows of H, TileW / 4 groups of 8 bytes (four 16-bit sums) each, then as many mask rows of
// TileW + 8 bytes (TileW + 2 * 3 halo, rounded up to dwords).  stage() puts the mask bytes of the tile and its R-pixel
// halo there, the reflected indices resolved here, four bytes and one aligned dword store per lane; then, after a
// barrier, runs the horizontal pass: three dword reads, four sums, one 8-byte store per lane.  The caller places the
// barrier between stage() and alpha(), which runs the vertical pass of one group in registers (2 R + 1 reads of 8
// bytes).  R == 0 has no LDS, no barrier and no stage(): alpha() reads the group's labels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "fcp_crop_bytes.h"

namespace fcp_feather {

constexpr int kClasses = 19;
constexpr int kMaxSide = 8192;

__host__ __device__ constexpr int tap(int r, int i) {
  return r == 1 ? (i == 1 ? 128 : 64)
       : r == 2 ? (i == 2 ? 96 : (i == 1 || i == 3) ? 64 : 16)
                : (i == 3 ? 72 : (i == 2 || i == 4) ? 56 : (i == 1 || i == 5) ? 28 : 8);
}
static_assert(tap(1, 0) + tap(1, 1) + tap(1, 2) == 256, "taps sum to 256");
static_assert(2 * (tap(2, 0) + tap(2, 1)) + tap(2, 2) == 256, "taps sum to 256");
static_assert(2 * (tap(3, 0) + tap(3, 1) + tap(3, 2)) + tap(3, 3) == 256, "taps sum to 256");

// BORDER_REFLECT_101, iterated: the triangle wave of period 2 (n - 1); a dimension of size 1 maps everything to 0.
__device__ __forceinline__ int reflect101(int p, int n) {
  if (p >= 0 && p < n) return p;
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  p %= period;
  if (p < 0) p += period;
  return p < n ? p : period - p;
}

__device__ __forceinline__ uint32_t mask_of(uint32_t label, uint32_t bits) {
  return (label < 32u && ((bits >> (label & 31u)) & 1u)) ? 255u : 0u;
}

__device__ __forceinline__ uint32_t over255(uint32_t c, uint32_t a, uint32_t b) {
  const uint32_t u = c * a + b * (255u - a) + 128u;
  return (u + (u >> 8)) >> 8;
}

// A checked feather (0, 3, 5 or 7) as Tile's R = feather / 2: calls fn(std::integral_constant<int, R>), on the host.
template <class Fn>
inline void with_feather(int feather, Fn&& fn) {
  switch (feather) {
    case 0: fn(std::integral_constant<int, 0>{}); break;
    case 3: fn(std::integral_constant<int, 1>{}); break;
    case 5: fn(std::integral_constant<int, 2>{}); break;
    default: fn(std::integral_constant<int, 3>{}); break;
  }
}

template <int R, int TileW, int TileH>
struct Tile {
  static_assert(R >= 0 && R <= 3 && TileW % 4 == 0, "feather 0, 3, 5 or 7; whole groups");
  static constexpr int kGroups = TileW / 4;
  static constexpr int kMaskPitch = TileW + 8;
  static constexpr int kRows = TileH + 2 * R;
  static constexpr size_t kBytes = R > 0 ? (size_t)kRows * (kGroups * sizeof(uint2) + kMaskPitch) : 0;   // of LDS, at hsum

  // The tile at (x0, y0) of the label map lab (h, w): nrows rows and groups groups of it are inside the map.  All lanes
  // of the workgroup (threads of them) call it.
  static __device__ __forceinline__ void stage(uint2* hsum, const uint8_t* lab, int h, int w, int x0, int y0, int nrows,
                                               int groups, uint32_t bits, int threads) {
    uint32_t* mask32 = reinterpret_cast<uint32_t*>(hsum + kRows * kGroups);
    // mask bytes of rows y0 - R .. y0 + nrows + R - 1, columns x0 - R .. x0 + 4 groups + R - 1 (to the next dword)
    const int mdw = (4 * groups + 2 * R + 3) >> 2;
    for (int i = threadIdx.x; i < (nrows + 2 * R) * mdw; i += threads) {
      const int tr = i / mdw, d = i - tr * mdw;
      const uint8_t* row = lab + (size_t)reflect101(y0 - R + tr, h) * w;
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) v |= mask_of(row[reflect101(x0 - R + 4 * d + j, w)], bits) << (8 * j);
      mask32[tr * (kMaskPitch / 4) + d] = v;
    }
    __syncthreads();
    // H of the same rows: output x of the tile sums mask bytes x .. x + 2 R
    for (int i = threadIdx.x; i < (nrows + 2 * R) * groups; i += threads) {
      const int tr = i / groups, g = i - tr * groups;
      const uint32_t* m = mask32 + tr * (kMaskPitch / 4) + g;
      const uint32_t d[3] = {m[0], m[1], R == 3 ? m[2] : 0u};
      uint32_t s[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int t = 0; t <= 2 * R; ++t) s[j] += (uint32_t)tap(R, t) * ((d[(j + t) >> 2] >> (8 * ((j + t) & 3))) & 255u);
      }
      hsum[tr * kGroups + g] = make_uint2(s[0] | (s[1] << 16), s[2] | (s[3] << 16));
    }
  }

  // a[0..npx-1] of group g of tile row r; lp points at the group's npx labels (read when R == 0 only).
  static __device__ __forceinline__ void alpha(const uint2* hsum, int r, int g, const uint8_t* lp, int npx, uint32_t bits,
                                               uint32_t a[4]) {
    if constexpr (R > 0) {
      uint32_t s[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int t = 0; t <= 2 * R; ++t) {
        const uint2 v = hsum[(r + t) * kGroups + g];
        s[0] += (uint32_t)tap(R, t) * (v.x & 0xffffu);
        s[1] += (uint32_t)tap(R, t) * (v.x >> 16);
        s[2] += (uint32_t)tap(R, t) * (v.y & 0xffffu);
        s[3] += (uint32_t)tap(R, t) * (v.y >> 16);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = (s[j] + 32768u) >> 16;
    } else {
      uint32_t l[4];
      fcp_crop_bytes::load_u8(lp, npx, l);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = mask_of(l[j], bits);
    }
  }
};

}  // namespace fcp_feather
