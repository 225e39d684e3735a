// Non-local-means noise removal of uint8 RGB crops (Cropper(denoise=H)), in integers.  For
// one crop (h,w,3), a weight table lut[0..n-1] of uint16 and a shift (tests/denoise_ref.py is the numpy restatement):
//
//   P = 3 (a 7 x 7 patch), S = 10 (a 21 x 21 search window), ONE = 4096; every coordinate outside the crop is reflected,
//   BORDER_REFLECT_101, which wants h, w >= P + S + 1 = 14.
//   g       = (9798 R + 19235 G + 3735 B + 16384) >> 15                       the gray of min_sharpness (fcp_gray.h)
//   d(p,o)  = sum over t in [-P,P]^2 of (g(p + t) - g(p + o + t))^2           for every o in [-S,S]^2; d <= 49 255^2 < 2^22
//   k       = d >> shift;   w(p,o) = min(lut[k], ONE) if k < n, else 0
//   W       = sum over o of w(p,o)                                            <= 441 ONE < 2^21
//   out_c(p) = (sum over o of w(p,o) c(p + o) + (W >> 1)) / W                 c = R, G, B; floor division; numerator < 2^29
//   W == 0: the pixel is copied.
//
// The weights come from the gray alone and the three channels are averaged with them.  Integer sums commute: the bytes do
// not depend on the tile, on the order of the offsets or on the launch geometry.
//
// One launch, no workspace, no float and no atomics.  A workgroup of 256 lanes owns a 32 x 64 tile of one crop and
// stages, once: the gray of the tile with a halo of P + S = 13 as bytes, the RGB of the tile with a halo of S as one
// dword a pixel (both reflected at the crop's edge, read from the crop as bytes: rows are 3 w bytes and start at any
// byte, and no byte outside the crop is touched), and the table, clamped at ONE, with a 0 behind its last entry so that
// k >= n needs no branch.  Then, per offset o, the box sum d is made in two passes through a double-buffered LDS plane,
// which costs one barrier per offset:
//   columns  210 lanes, one per (column of the tile plus a rim of P, run of 11 rows): 17 squared differences down the
//            column (the lane's own 17 gray bytes stay in registers for all 441 offsets, the partner's are 17 LDS bytes),
//            summed as they come, 11 vertical 7-sums as differences of those running sums, stored to the plane (lanes of
//            a wave store consecutive dwords);
//   rows     every lane, 8 consecutive pixels of one tile row: 14 plane dwords (16-byte reads) slid into 8 horizontal
//            7-sums = d, the table lookup, and w, w R, w G, w B added into 32 registers.
// The three divisions per pixel happen once, after the last offset.  Pixels of a tile past the crop's edge are computed
// from clamped coordinates and never stored.
// LDS 5.4 (gray) + 17.5 (RGB) + 18 (two planes) + 8 (table) = 49 KiB: three workgroups per CU, so that one workgroup's
// barrier waits behind another's arithmetic.
#include "fcp_common.h"
#include "fcp_crop_bytes.h"
#include "fcp_crop_checks.h"
#include "fcp_gray.h"
#include "fcp_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kP = 3;                                   // patch radius
constexpr int kS = 10;                                  // search radius
constexpr int kHalo = kP + kS;
constexpr int kMinSide = kHalo + 1;                     // one reflection reaches every coordinate a crop pixel needs
constexpr uint32_t kOne = 4096;
constexpr int kMaxLut = 4096;
constexpr int kMaxShift = 10;
constexpr int kTileH = 32;
constexpr int kTileW = 64;
constexpr int kGroup = 8;                               // pixels of a lane in the row pass: 32 rows x 8 groups = 256 lanes
constexpr int kRun = 11;                                // rows of a lane in the column pass
constexpr int kRuns = (kTileH + kRun - 1) / kRun;       // 3: the last run ends one row past the tile
constexpr int kDiffs = kRun + 2 * kP;                   // 17 squared differences make the 11 sums of a run
constexpr int kSumCols = kTileW + 2 * kP;               // 70 columns of vertical sums
constexpr int kSumPitch = 72;                           // dwords: rows of the plane start at 16 bytes
constexpr int kGrayCols = kTileW + 2 * kHalo;           // 90
constexpr int kGrayRows = kRuns * kRun + 2 * kHalo;     // 59: one more than the tile needs, the last run reads it
constexpr int kGrayPitch = 92;                          // bytes
constexpr int kRgbCols = kTileW + 2 * kS;               // 84
constexpr int kRgbRows = kTileH + 2 * kS;               // 52
constexpr int kRgbPitch = 86;                           // dwords: the four rows of a 32-lane group start 22 banks apart

static_assert(kThreads == kTileH * (kTileW / kGroup) && kRuns * kSumCols <= kThreads, "lanes of the two passes");
static_assert(kGroup + 2 * kP == 14 && kSumPitch >= kSumCols && kSumPitch % 4 == 0, "the row pass reads 3 x 16 + 8 bytes");
static_assert(kGrayPitch >= kGrayCols && kGrayPitch % 4 == 0 && kRgbPitch >= kRgbCols, "tile pitches");
static_assert(49u * 255u * 255u < (1u << 22) && 441u * kOne * 255u + 441u * kOne / 2 < (1u << 29), "32-bit sums suffice");

// BORDER_REFLECT_101 of v into 0..n-1; past one reflection (only pixels of a tile outside the crop, never stored) clamped
__device__ __forceinline__ int reflect(int v, int n) {
  v = v < 0 ? -v : v;
  v = v >= n ? 2 * (n - 1) - v : v;
  return min(max(v, 0), n - 1);
}

__global__ void __launch_bounds__(kThreads) nlm_denoise_kernel(const uint8_t* __restrict__ crops, int h, int w,
                                                               const uint16_t* __restrict__ lut, int n, int shift, int tiles_x,
                                                               uint8_t* __restrict__ out) {
  __shared__ uint32_t gray32[kGrayRows * kGrayPitch / 4];
  __shared__ uint32_t rgb[kRgbRows * kRgbPitch];
  __shared__ uint4 plane4[2][kTileH * kSumPitch / 4];
  __shared__ uint16_t weight[kMaxLut + 2];
  const int t = threadIdx.x, f = blockIdx.y;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int y0 = tile_y * kTileH, x0 = tile_x * kTileW;
  const uint8_t* crop = crops + (size_t)f * h * w * 3;
  uint8_t* gray = reinterpret_cast<uint8_t*>(gray32);

  for (int i = t; i < kGrayRows * kGrayCols; i += kThreads) {
    const int r = i / kGrayCols, c = i - r * kGrayCols;
    const uint8_t* p = crop + ((size_t)reflect(y0 - kHalo + r, h) * w + reflect(x0 - kHalo + c, w)) * 3;
    const uint32_t cr = p[0], cg = p[1], cb = p[2];
    gray[r * kGrayPitch + c] = (uint8_t)fcp_gray::gray_of(cr, cg, cb);
    const int rr = r - kP, cc = c - kP;
    if (rr >= 0 && rr < kRgbRows && cc >= 0 && cc < kRgbCols) rgb[rr * kRgbPitch + cc] = cr | (cg << 8) | (cb << 16);
  }
  for (int i = t; i <= n; i += kThreads) weight[i] = i < n ? (uint16_t)min((uint32_t)lut[i], kOne) : (uint16_t)0;
  __syncthreads();

  // the column pass: vertical sums for plane rows run * kRun .., column col (pixel x0 + col - kP)
  const bool summing = t < kRuns * kSumCols;
  const int run = t / kSumCols, col = t - run * kSumCols;
  const int own = (run * kRun + kS) * kGrayPitch + col + kS;     // gray of pixel (run * kRun - kP, col - kP) of the tile
  int g1[kDiffs];
  if (summing) {
#pragma unroll
    for (int i = 0; i < kDiffs; ++i) g1[i] = gray[own + i * kGrayPitch];
  }
  // the row pass: pixels (py, px .. px + 7) of the tile
  const int py = t >> 3, px = (t & 7) * kGroup;
  uint32_t acc[kGroup][4];
#pragma unroll
  for (int k = 0; k < kGroup; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0u;

  int buf = 0;
  for (int oy = -kS; oy <= kS; ++oy) {
    for (int ox = -kS; ox <= kS; ++ox) {
      uint32_t* plane = reinterpret_cast<uint32_t*>(plane4[buf]);
      if (summing) {
        const uint8_t* g2 = gray + own + oy * kGrayPitch + ox;
        int below[kDiffs];                               // below[i]: the squared differences of rows 0 .. i of the run, summed
#pragma unroll
        for (int i = 0; i < kDiffs; ++i) {
          const int diff = g1[i] - (int)g2[i * kGrayPitch];
          below[i] = diff * diff + (i > 0 ? below[i - 1] : 0);
          if (i >= 2 * kP) {
            const int row = run * kRun + i - 2 * kP;
            const int sum = below[i] - (i > 2 * kP ? below[i - 2 * kP - 1] : 0);
            if (row < kTileH) plane[row * kSumPitch + col] = (uint32_t)sum;
          }
        }
      }
      __syncthreads();                                   // the plane of this offset is whole; the other one is free
      const uint4* v4 = plane4[buf] + (py * kSumPitch + px) / 4;
      const uint4 a = v4[0], b = v4[1], c = v4[2];
      const uint2 e = *reinterpret_cast<const uint2*>(v4 + 3);
      const uint32_t v[kGroup + 2 * kP] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, e.x, e.y};
      const uint32_t* src = rgb + (py + kS + oy) * kRgbPitch + px + kS + ox;
      uint32_t dist = v[0] + v[1] + v[2] + v[3] + v[4] + v[5] + v[6];
#pragma unroll
      for (int k = 0; k < kGroup; ++k) {
        if (k > 0) dist += v[k + 2 * kP] - v[k - 1];
        const uint32_t wgt = weight[min(dist >> shift, (uint32_t)n)];
        const uint32_t pixel = src[k];
        acc[k][0] += wgt * (pixel & 255u);
        acc[k][1] += wgt * ((pixel >> 8) & 255u);
        acc[k][2] += wgt * (pixel >> 16);
        acc[k][3] += wgt;
      }
      buf ^= 1;
    }
  }

  const int y = y0 + py, x = x0 + px;
  if (y >= h || x >= w) return;
  const uint32_t* centre = rgb + (py + kS) * kRgbPitch + px + kS;
  uint8_t* op = out + (((size_t)f * h + y) * w + x) * 3;
#pragma unroll
  for (int g = 0; g < kGroup / 4; ++g) {
    const int npx = min(4, w - (x + 4 * g));
    if (npx <= 0) break;
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 4 * g + j;
      const uint32_t total = acc[k][3], half = total >> 1, pixel = centre[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint32_t value = total != 0u ? (acc[k][c] + half) / total : (pixel >> (8 * c)) & 255u;
        const int byte = 3 * j + c;                          // byte of the group
        o[byte >> 2] |= value << (8 * (byte & 3));
      }
    }
    fcp_crop_bytes::store_rgb(op + 12 * g, npx, o);
  }
}

}  // namespace

extern "C" int fcp_nlm_denoise_u8(const uint8_t* crops, int f, int h, int w, const uint16_t* lut, int lut_len, int shift,
                                  uint8_t* out, fcp_stream_t stream) {
  const char* who = "nlm_denoise";
  FCP_CHECK(fcp_crop_checks::check_sizes(who, f, h, w));
  FCP_REQUIRE(h >= kMinSide && w >= kMinSide, "%s: crops of at least %d x %d px (got h %d, w %d): the reflected window", who, kMinSide,
              kMinSide, h, w);
  FCP_REQUIRE(lut_len >= 1 && lut_len <= kMaxLut, "%s: lut_len must be 1..%d (got %d)", who, kMaxLut, lut_len);
  FCP_REQUIRE(shift >= 0 && shift <= kMaxShift, "%s: shift must be 0..%d (got %d)", who, kMaxShift, shift);
  if (f == 0) return 0;
  FCP_REQUIRE(crops && lut && out, "%s: null pointer", who);
  FCP_REQUIRE((reinterpret_cast<uintptr_t>(lut) & 1) == 0, "%s: the table must be 2-byte aligned", who);
  const uintptr_t bytes = (uintptr_t)f * h * w * 3, from = reinterpret_cast<uintptr_t>(crops), to = reinterpret_cast<uintptr_t>(out);
  FCP_REQUIRE(to + bytes <= from || from + bytes <= to, "%s: out must not overlap crops (out == crops included): a pixel reads its window",
              who);
  const int tiles_x = fcp_cdiv(w, kTileW), tiles_y = fcp_cdiv(h, kTileH);
  hipLaunchKernelGGL(nlm_denoise_kernel, dim3(tiles_x * tiles_y, f), dim3(kThreads), 0, (hipStream_t)stream, crops, h, w, lut, lut_len,
                     shift, tiles_x, out);
  FCP_LAUNCH_OK();
  return 0;
}
