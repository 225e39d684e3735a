// Unsharp-mask sharpening of uint8 RGB crops (Cropper(sharpen=A)), in integers: the gray's
// difference from its own Gaussian blur, cored and scaled, is added to all three channels alike, so there are no colour
// fringes.  For one crop (h,w,3), taps t[0..r], an amount A_q and a threshold T (tests/sharpen_ref.py is the numpy
// restatement):
//
//   t[0..r]  : integer taps, t[0] + 2 sum(t[1..r]) == 4096, 1 <= r <= 48; a tap may be 0
//   g        = gray_of(R, G, B)                                   the gray of min_sharpness (fcp_gray.h)
//   coordinates outside the crop are clamped to its edge          BORDER_REPLICATE: any h, w >= 1
//   Hs(y,x)  = sum_i t|i| g(y, clamp(x + i))                      <= 255 * 4096
//   B(y,x)   = sum_j t|j| Hs(clamp(y + j), x)                     <= 255 * 2^24 < 2^32, unsigned
//   b8       = (B + 32768) >> 16                                  the blurred gray with 8 fraction bits
//   d        = (g << 8) - b8                                      |d| <= 65280
//   e        = sign(d) * max(|d| - (T << 8), 0)                   soft threshold (coring), T = 0..255 gray levels
//   v_c      = (c << 16) + A_q * e + 32768                        c = R, G, B; |A_q e| <= 1024 * 65280: signed 32 bits
//   out_c    = v_c < 0 ? 0 : min(255, v_c >> 16)
//
// Integer sums commute: the bytes do not depend on the tile or on the launch geometry.
//
// One launch, no workspace, no float and no atomics.  A workgroup of 256 lanes owns a TileH x 64 tile of one crop, and a
// lane works on groups of four consecutive pixels of a row throughout:
//   stage    the gray of the tile and an r-pixel halo as bytes, the clamp applied here (read from the crop as bytes: rows
//            are 3 w bytes and start at any byte, and no byte outside the crop is touched), and the taps, mirrored to
//            2 r + 1 dwords with zeros on both sides, so that the loops below have neither |k| nor an edge case;
//   rows     a group's four horizontal sums of one staged row: the row's gray a dword (four pixels) at a time, each with
//            the seven taps that its bytes meet in the four sums, stored as 16 bytes;
//   columns  a group's four vertical sums, 16 bytes per tap, then the delta of each pixel and the group's 12 RGB bytes
//            (fcp_crop_bytes.h).
// Consecutive lanes are consecutive groups, so they read consecutive dwords of the gray and consecutive 16 bytes of the
// sums; a staged row of gray is 192 bytes, which puts the two rows of 16 groups that 32 lanes read on disjoint banks.
// Two tile shapes, chosen on the host by the radius alone: r <= 8 (sigma up to 2.67) runs 32 x 64 tiles with LDS for a
// halo of 8 (21.1 KiB: seven workgroups a CU; a halo of 5 adds 31 % to the rows pass), r > 8 runs 48 x 64 tiles with LDS
// for a halo of 48 (63.4 KiB: two workgroups a CU).  A tile's pixels past the crop's edge are never computed or stored.
#include "fcp_common.h"
#include "fcp_crop_bytes.h"
#include "fcp_crop_checks.h"
#include "fcp_gray.h"
#include "fcp_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxRadius = 48;
constexpr int kSmallRadius = 8;                         // up to here the small tile
constexpr uint32_t kTapSum = 4096;
constexpr int kMaxAmount = 1024;
constexpr int kTileW = 64;
constexpr int kGroups = kTileW / 4;                     // groups of four pixels in a tile row
constexpr int kGrayPitch = 192;                         // bytes of a staged row of gray: 48 dwords, 16 banks past 32

struct Taps {
  uint16_t t[kMaxRadius + 1];                           // 49 x 16 bit in the kernel argument block
};

template <int TileH, int MaxR>
__global__ void __launch_bounds__(kThreads) unsharp_kernel(const uint8_t* __restrict__ crops, int h, int w, Taps taps, int radius,
                                                           int amount, int threshold8, int tiles_x, uint8_t* __restrict__ out) {
  constexpr int kRows = TileH + 2 * MaxR;               // staged rows
  constexpr int kTapSlots = 2 * MaxR + 12;              // 3 zeros, the 2 r + 1 mirrored taps, zeros
  static_assert(kGrayPitch >= kTileW + 2 * MaxR + 4 && kGrayPitch % 128 == 64, "a dword past the last tap; rows 16 banks apart");
  static_assert(kRows * kGrayPitch + kRows * kGroups * 16 + kTapSlots * 4 <= 65536, "static LDS");
  static_assert(255u * kTapSum * (uint64_t)kTapSum < (1ull << 32) && kMaxAmount * 65280 + (255 << 16) + 32768 < (1ll << 31), "32-bit sums");
  __shared__ uint32_t gray32[kRows * kGrayPitch / 4];
  __shared__ uint4 hs[kRows * kGroups];
  __shared__ __attribute__((aligned(16))) uint32_t tl[kTapSlots];
  const int t = threadIdx.x, f = blockIdx.y;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int y0 = tile_y * TileH, x0 = tile_x * kTileW;
  const int nrows = min(TileH, h - y0), ngroups = (min(kTileW, w - x0) + 3) >> 2;
  const int srows = nrows + 2 * radius, scols = 4 * ngroups + 2 * radius;
  const uint8_t* crop = crops + (size_t)f * h * w * 3;
  uint8_t* gray = reinterpret_cast<uint8_t*>(gray32);

  // staged (sr, sc) is the gray of pixel (clamp(y0 - r + sr), clamp(x0 - r + sc)); tl[k + 3] = t|k - r| for k in 0 .. 2 r
  for (int i = t; i < kTapSlots; i += kThreads) {
    const int k = i - 3;
    tl[i] = k >= 0 && k <= 2 * radius ? (uint32_t)taps.t[k < radius ? radius - k : k - radius] : 0u;
  }
  // four pixels a lane at a time, so that their twelve loads are in flight together; past the end the last pixel again,
  // which puts the same byte in the same place
  const int staged = srows * scols;
  for (int i0 = t; i0 < staged; i0 += 4 * kThreads) {
    uint32_t px[4][3];
    int at[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = min(i0 + u * kThreads, staged - 1);
      const int sr = i / scols, sc = i - sr * scols;
      const int y = min(max(y0 - radius + sr, 0), h - 1), x = min(max(x0 - radius + sc, 0), w - 1);
      const uint8_t* p = crop + ((size_t)y * w + x) * 3;
      px[u][0] = p[0], px[u][1] = p[1], px[u][2] = p[2];
      at[u] = sr * kGrayPitch + sc;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) gray[at[u]] = (uint8_t)fcp_gray::gray_of(px[u][0], px[u][1], px[u][2]);
  }
  __syncthreads();

  // rows: sum i of a group takes byte b of the group's dwords with tap k = b - i, that is tl[b - i + 3]; the bytes past the
  // last tap (up to three of them never staged) meet zeros
  const int ndwords = (2 * radius + 7) >> 2;
  for (int i = t; i < srows * ngroups; i += kThreads) {
    const int sr = i / ngroups, g = i - sr * ngroups;
    const uint32_t* src = gray32 + sr * (kGrayPitch / 4) + g;
    uint32_t a[4] = {0u, 0u, 0u, 0u};
    for (int m = 0; m < ndwords; ++m) {
      const uint32_t d = src[m];
      const uint32_t* tp = tl + 4 * m;
      const uint32_t tap[7] = {tp[0], tp[1], tp[2], tp[3], tp[4], tp[5], tp[6]};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t v = (d >> (8 * j)) & 255u;
#pragma unroll
        for (int s = 0; s < 4; ++s) a[s] += tap[j - s + 3] * v;
      }
    }
    hs[sr * kGroups + g] = make_uint4(a[0], a[1], a[2], a[3]);
  }
  __syncthreads();

  // columns, then the delta: pixel (y0 + ty, x0 + 4 g + s)
  for (int i = t; i < nrows * ngroups; i += kThreads) {
    const int ty = i / ngroups, g = i - ty * ngroups;
    const int y = y0 + ty, x = x0 + 4 * g;
    const int npx = min(4, w - x);
    const size_t at = ((size_t)y * w + x) * 3;
    uint32_t c[3], o[3] = {0u, 0u, 0u};
    fcp_crop_bytes::load_rgb_together(crop + at, npx, c);   // asked for here, needed after the taps
    const uint4* col = hs + ty * kGroups + g;
    uint32_t b[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k <= 2 * radius; ++k) {
      const uint32_t tap = tl[k + 3];
      const uint4 v = col[k * kGroups];
      b[0] += tap * v.x;
      b[1] += tap * v.y;
      b[2] += tap * v.z;
      b[3] += tap * v.w;
    }
    const uint8_t* own = gray + (ty + radius) * kGrayPitch + 4 * g + radius;
    int add[4];                                          // A_q e + 32768
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int d = ((int)own[s] << 8) - (int)((b[s] + 32768u) >> 16);
      const int over = max(abs(d) - threshold8, 0);
      add[s] = amount * (d < 0 ? -over : over) + 32768;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {                       // byte k of the group: pixel k / 3
      const int v = (int)(((c[k >> 2] >> (8 * (k & 3))) & 255u) << 16) + add[k / 3];
      o[k >> 2] |= (uint32_t)(v < 0 ? 0 : min(255, v >> 16)) << (8 * (k & 3));
    }
    fcp_crop_bytes::store_rgb(out + (size_t)f * h * w * 3 + at, npx, o);
  }
}

template <int TileH, int MaxR>
void launch(const uint8_t* crops, int f, int h, int w, const Taps& taps, int radius, int amount, int threshold, uint8_t* out,
            hipStream_t stream) {
  const int tiles_x = fcp_cdiv(w, kTileW), tiles_y = fcp_cdiv(h, TileH);
  hipLaunchKernelGGL((unsharp_kernel<TileH, MaxR>), dim3(tiles_x * tiles_y, f), dim3(kThreads), 0, stream, crops, h, w, taps, radius,
                     amount, threshold << 8, tiles_x, out);
}

}  // namespace

extern "C" int fcp_unsharp_u8(const uint8_t* crops, int f, int h, int w, const uint16_t* taps, int radius, int amount_q8, int threshold,
                              uint8_t* out, fcp_stream_t stream) {
  const char* who = "unsharp";
  FCP_CHECK(fcp_crop_checks::check_sizes(who, f, h, w));
  FCP_REQUIRE(radius >= 1 && radius <= kMaxRadius, "%s: radius must be 1..%d (got %d)", who, kMaxRadius, radius);
  FCP_REQUIRE(amount_q8 >= 1 && amount_q8 <= kMaxAmount, "%s: amount_q8 must be 1..%d (got %d)", who, kMaxAmount, amount_q8);
  FCP_REQUIRE(threshold >= 0 && threshold <= 255, "%s: threshold must be 0..255 (got %d)", who, threshold);
  FCP_REQUIRE(taps != nullptr, "%s: null pointer (taps)", who);
  FCP_REQUIRE((reinterpret_cast<uintptr_t>(taps) & 1) == 0, "%s: the taps must be 2-byte aligned", who);
  Taps t = {};
  uint32_t total = 0;
  for (int k = 0; k <= radius; ++k) {
    t.t[k] = taps[k];
    total += (k == 0 ? 1u : 2u) * taps[k];
  }
  FCP_REQUIRE(total == kTapSum, "%s: the taps must sum to %u over the window (got %u)", who, kTapSum, total);
  if (f == 0) return 0;
  FCP_REQUIRE(crops && out, "%s: null pointer", who);
  const uintptr_t bytes = (uintptr_t)f * h * w * 3, from = reinterpret_cast<uintptr_t>(crops), to = reinterpret_cast<uintptr_t>(out);
  FCP_REQUIRE(to + bytes <= from || from + bytes <= to,
              "%s: out must not overlap crops (out == crops included): a workgroup reads its neighbours' pixels", who);
  // two tile shapes, by the radius alone: a small halo does not pay for the LDS and the rows of the largest one
  if (radius <= kSmallRadius)
    launch<32, kSmallRadius>(crops, f, h, w, t, radius, amount_q8, threshold, out, (hipStream_t)stream);
  else
    launch<48, kMaxRadius>(crops, f, h, w, t, radius, amount_q8, threshold, out, (hipStream_t)stream);
  FCP_LAUNCH_OK();
  return 0;
}
