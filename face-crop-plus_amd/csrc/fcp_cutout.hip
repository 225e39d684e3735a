// RGBA cut-outs and the subject's own edge colours (Cropper(background="transparent"), Cropper(decontaminate=sigma),
// INTEGRATION.md section 2n).  In the soft edge of a matte the crop's colour is already alpha F + (1 - alpha) B_old:
// shipping (c, alpha), or compositing c over a new fill, carries the old background along as a halo.  The subject's
// colour F is estimated by "blur fusion": two mask-normalised Gaussians, one over the pixels that are certainly
// subject and one over those that are certainly background, and one integer correction.  tests/cutout_ref.py states
// the same in numpy; the kernels are held to it byte for byte.
//
//   c (F,H,W,3) u8, a (F,H,W) u8: the alpha the mode already has (fcp_feather_alpha_u8's, or fcp_matte_refine_u8's)
//   t[0..r]   : the taps of fcp_masked_blur.h, made on the host from sigma (matte.blur_taps)
//   sF(p)     = 1 where a(p) == 255 else 0                                              "certainly subject"
//   sB(p)     = 1 where a(p) == 0   else 0                                              "certainly background"
//   F^_ch, B^_ch = the mask-normalised Gaussians B_ch of fcp_masked_blur.h over the sides sF (side 0) and sB (side 1)
//   R_ch      = 255 c_ch - (a F^_ch + (255 - a) B^_ch)                                  in [-65025, 65025]
//   E_ch      = clamp(floor((65025 F^_ch + a R_ch + 32512) / 65025), 0, 255)
//   F_ch      = c_ch where a == 255;  E_ch where 0 < a < 255;  (unused) where a == 0
//
//   RGBA, radius 0 : (c_r, c_g, c_b, a) where a > 0, (0,0,0,0) where a == 0             hidden colours do not ship
//   RGBA, radius r : (F_r, F_g, F_b, a) where a > 0, (0,0,0,0) where a == 0
//   fill, radius r : (F_ch a + fill_ch (255 - a) + 127) / 255, three channels           fcp_feather.h's over255
//   fill, radius 0 : refused: that is fcp_matte_alpha_u8, which stays the one statement of it
//   picture, radius r : the fill composite with P_ch, the face's picture of a bank, as fill_ch (fcp_cutout_image_u8,
//                    Cropper(background_image=...), section 2r): the same kernels with fcp_fill.h's Picture as the fill
//                    source of the columns pass; radius 0 is refused likewise: that is fcp_matte_image_alpha_u8
//
// Bounds.  The sums and their unsigned 32-bit bounds are fcp_masked_blur.h's; F^, B^ <= 255.  The correction is signed
// 32 bits: |a R| <= 254 * 65025 and 65025 F^ <= 255 * 65025, so the numerator lies in (-255 * 65025, 2^25); the floor
// division adds 255 * 65025 (the numerator is then positive), divides and takes 255 off again.
//
// The alpha plane comes from fcp_feather_alpha_u8 (fcp_matte.hip) or fcp_matte_refine_u8.
//
// fcp_cutout_u8 with a radius: two launches and a workspace of 32 bytes per pixel (the caller's).
//
//   cutout_rows_kernel, workgroups of 256 lanes over (4 rows x 256 columns, face): fcp_masked_blur.h's rows_pass with
//   two staged dwords per pixel, the subject side first.  LDS per workgroup: 4 x (256 + 96) x 8 B + 97 taps x 4 B =
//   11652 B: 14 workgroups would fit a CU, the 32 wave slots allow 8.
//
//   cutout_cols_kernel, workgroups of 256 lanes over (128 rows x 8 columns, face), four pixels of a row per lane, one
//   group per lane.  Two sets of sums double the 16 bytes per staged pixel of blur_cols_kernel: its 64 x 16 tile would
//   need (64 + 96) x 16 x 32 B = 81920 B at r = 48, and two of those do not fit beside their tap tables.  The tile here
//   is half as wide and twice as tall, which also reads each staged row for twice as many outputs: rows
//   y0 - r .. y0 + 127 + r of 8 pixels x 32 B plus one 16-byte pad (a pitch of 272 B: the 16-byte reads of the eight
//   rows and two groups that one LDS cycle serves fall into 16 different 16-byte slots of the 256-byte bank line;
//   with a pitch of 256 B the eight rows would meet in one).  LDS per workgroup at r = 48: 224 x 272 B = 60928 B of
//   sums + 388 B of taps + 256 B of static LDS behind __syncthreads_or = 61572 B: 2 workgroups per CU (160 KiB; the
//   third misses), below the 64 KiB that need no opt-in; at r = 12 (sigma 4) 152 x 272 + 388 + 256 = 41988 B: 3
//   workgroups.
//   A lane first reads the four alpha bytes of its group.  A workgroup whose tile holds no pixel with 0 < a < 255
//   stages nothing and runs no tap (a uniform branch after one __syncthreads_or): E is needed nowhere there, the
//   bytes do not depend on the branch.  Inside an edge tile a lane without such a pixel skips its taps too.
//
// Bytes per pixel of an edge tile: the rows pass reads 4 (crop + alpha) and writes 32; the columns pass reads
// 32 x (128 + 2 r) / 128 of sums (38 at r = 12, 56 at r = 48), 1 of alpha and 3 of crop and writes 4 or 3.  A tile
// without a soft pixel reads 4 and writes 4 or 3.
//
// out is its own array: it never aliases crops (RGBA pixels are wider than the crop's).  crops, alpha and labels
// start at any byte and move by the rules of fcp_crop_bytes.h; the fill composite is written by those rules too; RGBA
// pixels are one aligned dword store each, so an RGBA out must be 4-byte aligned.  No byte outside the arrays is
// written, and no dword is read that does not hold a byte of them.  Integer sums in a fixed order, one writer per
// byte: the same bytes from run to run.
#include "fcp_common.h"
#include "fcp_crop_bytes.h"
#include "fcp_crop_checks.h"
#include "fcp_feather.h"
#include "fcp_fill.h"
#include "fcp_hip.h"
#include "fcp_masked_blur.h"

namespace {

using namespace fcp_crop_bytes;
using namespace fcp_crop_checks;
using namespace fcp_feather;
using namespace fcp_masked_blur;
using fcp_fill::Colour;
using fcp_fill::Picture;

// columns pass
constexpr int kTileW = 8;               // output pixels of a tile row: 2 groups of four
constexpr int kTileH = 128;
constexpr int kGroups = kTileW / 4;
constexpr int kColPitch = 2 * kTileW + 1;   // uint4 of a staged row: (subject, background) per pixel and the pad
static_assert(kTileH * kGroups == kThreads, "one group per lane");

// byte k of an RGB group (pixel k / 3, channel k % 3)
__device__ __forceinline__ uint32_t rgb_byte(const uint32_t c[3], int k) { return (c[k >> 2] >> (8 * (k & 3))) & 255u; }

// One RGBA pixel: the colour under its alpha, nothing where the alpha is 0.
__device__ __forceinline__ uint32_t rgba(uint32_t r, uint32_t g, uint32_t b, uint32_t a) {
  return a == 0u ? 0u : (r | (g << 8) | (b << 16) | (a << 24));
}

// RGBA without an estimate: a lane per group of four pixels.
__global__ void __launch_bounds__(kThreads) cutout_plain_kernel(const uint8_t* __restrict__ crops, const uint8_t* __restrict__ alpha,
                                                                int w, int groups_x, size_t groups, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= groups) return;
  const size_t row = i / groups_x;       // face * h + y
  const int x = 4 * (int)(i - row * groups_x);
  const int npx = min(4, w - x);
  const size_t pixel = row * w + x;
  uint32_t a[4], c[3];
  load_u8(alpha + pixel, npx, a);
  load_rgb(crops + pixel * 3, npx, c);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < npx) out[pixel + j] = rgba(rgb_byte(c, 3 * j), rgb_byte(c, 3 * j + 1), rgb_byte(c, 3 * j + 2), a[j]);
}

__global__ void __launch_bounds__(kThreads) cutout_rows_kernel(const uint8_t* __restrict__ crops, const uint8_t* __restrict__ alpha,
                                                               int h, int w, int tiles_x, Taps taps, int radius,
                                                               uint4* __restrict__ sums) {
  rows_pass<2>(crops, alpha, h, w, tiles_x, taps, radius, sums, [](uint32_t a) { return a == 255u ? 0 : a == 0u ? 1 : -1; });
}

// E of one channel, 0 < a < 255
__device__ __forceinline__ uint32_t corrected(uint32_t c, uint32_t a, uint32_t fh, uint32_t bh) {
  const int32_t r = 255 * (int32_t)c - (int32_t)(a * fh + (255u - a) * bh);
  const int32_t num = 65025 * (int32_t)fh + (int32_t)a * r + 32512;
  const int32_t e = (num + 255 * 65025) / 65025 - 255;   // floor: the numerator is above -255 * 65025
  return (uint32_t)min(255, max(0, e));
}

constexpr size_t cols_lds_bytes(int radius) {
  return (size_t)(kTileH + 2 * radius) * kColPitch * sizeof(uint4) + kTapBytes;
}

// Rgba: out is (f,h,w) dwords; else (f,h,w,3) bytes over `fill`, fcp_fill.h's Colour or Picture.
template <bool Rgba, class Fill = Colour>
__global__ void __launch_bounds__(kThreads) cutout_cols_kernel(const uint8_t* __restrict__ crops, const uint8_t* __restrict__ alpha,
                                                               const uint4* __restrict__ sums, int h, int w, int tiles_x,
                                                               Fill fill, Taps taps, int radius, uint8_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* col = reinterpret_cast<uint4*>(smem);                                   // (kTileH + 2 r) rows of kColPitch
  uint32_t* tl = reinterpret_cast<uint32_t*>(col + (kTileH + 2 * radius) * kColPitch);
  const int f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const int nrows = min(kTileH, h - y0);
  const int groups = (min(kTileW, w - x0) + 3) >> 2;

  // the lane's group, if the tile has one for it
  const int r = threadIdx.x / kGroups, g = threadIdx.x - r * kGroups;
  const bool mine = r < nrows && g < groups;
  const int x = x0 + 4 * g;
  const int npx = mine ? min(4, w - x) : 0;
  const size_t pixel = ((size_t)f * h + (y0 + r)) * w + x;
  uint32_t a[4] = {0u, 0u, 0u, 0u};
  if (mine) load_u8(alpha + pixel, npx, a);
  bool soft = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) soft = soft || (j < npx && a[j] > 0u && a[j] < 255u);

  // D and N of the four pixels, both sides: N + D / 2 < 2^32
  uint32_t dn[4][8] = {};
  if (__syncthreads_or(soft)) {          // the same for every lane of the workgroup
    stage_taps(tl, taps, radius);
    stage_cols<2, kTileW, kColPitch>(col, sums, f, h, w, x0, y0, nrows, radius);
    __syncthreads();
    if (soft) cols_taps<2, kColPitch>(col, tl, radius, r, g, dn);
  }
  if (!mine) return;

  uint32_t c[3];
  load_rgb(crops + pixel * 3, npx, c);
  uint32_t fg[4][3];                     // F of the group's pixels
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const uint32_t cv = rgb_byte(c, 3 * j + ch);
      uint32_t v = cv;
      if (a[j] > 0u && a[j] < 255u)
        v = corrected(cv, a[j], normalised(dn[j][1 + ch], dn[j][0], cv), normalised(dn[j][5 + ch], dn[j][4], cv));
      fg[j][ch] = v;
    }
  }
  if constexpr (Rgba) {
    uint32_t* o = reinterpret_cast<uint32_t*>(out) + pixel;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < npx) o[j] = rgba(fg[j][0], fg[j][1], fg[j][2], a[j]);
  } else {
    const auto b = fill.face(f, h, w).group((size_t)(y0 + r) * w + x, npx);
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 12; ++k)              // byte k of the group: pixel k / 3, channel k % 3
      o[k >> 2] |= over255(fg[k / 3][k % 3], a[k / 3], b.byte(k)) << (8 * (k & 3));
    store_rgb(out + pixel * 3, npx, o);
  }
}

// The two launches of an estimate for the entry point `who`: the rows pass into the caller's workspace, then the columns
// pass to RGBA or over `fill`.
template <bool Rgba, class Fill>
int estimate(const char* who, const uint8_t* crops, const uint8_t* alpha, int f, int h, int w, Fill fill, const Taps& t, int radius,
             uint8_t* out, void* workspace, int64_t workspace_bytes, hipStream_t s) {
  FCP_CHECK(check_workspace(who, workspace, workspace_bytes, fcp_cutout_workspace_bytes(f, h, w)));
  uint4* sums = static_cast<uint4*>(workspace);
  const int row_tiles_x = fcp_cdiv(w, kRowTileW), row_tiles_y = fcp_cdiv(h, kRowTileH);
  hipLaunchKernelGGL(cutout_rows_kernel, dim3(row_tiles_x * row_tiles_y, f), dim3(kThreads), rows_lds_bytes<2>(), s, crops, alpha,
                     h, w, row_tiles_x, t, radius, sums);
  FCP_LAUNCH_OK();
  const int tiles_x = fcp_cdiv(w, kTileW), tiles_y = fcp_cdiv(h, kTileH);
  hipLaunchKernelGGL((cutout_cols_kernel<Rgba, Fill>), dim3(tiles_x * tiles_y, f), dim3(kThreads), cols_lds_bytes(radius), s, crops,
                     alpha, sums, h, w, tiles_x, fill, t, radius, out);
  FCP_LAUNCH_OK();
  return 0;
}

}  // namespace

extern "C" int64_t fcp_cutout_workspace_bytes(int f, int h, int w) { return workspace_bytes(f, h, w, 2 * sizeof(uint4)); }

extern "C" int fcp_cutout_u8(const uint8_t* crops, const uint8_t* alpha, int f, int h, int w, int mode, int bg_r, int bg_g, int bg_b,
                             const uint16_t* taps, int radius, uint8_t* out, void* workspace, int64_t workspace_bytes,
                             fcp_stream_t stream) {
  const char* who = "cutout";
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_REQUIRE(mode == FCP_CUTOUT_RGBA || mode == FCP_CUTOUT_FILL, "cutout: mode must be %d (RGBA) or %d (fill) (got %d)",
              FCP_CUTOUT_RGBA, FCP_CUTOUT_FILL, mode);
  FCP_REQUIRE(radius == 0 || (radius >= kMinRadius && radius <= kMaxRadius), "cutout: radius must be 0 or %d..%d (got %d)",
              kMinRadius, kMaxRadius, radius);
  FCP_REQUIRE(mode == FCP_CUTOUT_RGBA || radius > 0,
              "cutout: the fill mode needs a radius: without an estimate it is fcp_matte_alpha_u8");
  FCP_CHECK(check_fill(who, bg_r, bg_g, bg_b));
  Taps t = {};
  if (radius > 0) FCP_CHECK(load_taps(who, taps, radius, &t));
  if (f == 0) return 0;
  FCP_REQUIRE(crops && alpha && out, "cutout: null pointer");
  FCP_REQUIRE(mode != FCP_CUTOUT_RGBA || (reinterpret_cast<uintptr_t>(out) & 3) == 0, "cutout: an RGBA out must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (radius == 0) {
    const int groups_x = fcp_cdiv(w, 4);
    const size_t groups = (size_t)f * h * groups_x;       // <= 65535 * 8192 * 2048 < 2^40: blocks < 2^32
    FCP_REQUIRE((groups + kThreads - 1) / kThreads <= 0x7fffffffull, "cutout: too many pixels for one launch (f %d, h %d, w %d)",
                f, h, w);
    hipLaunchKernelGGL(cutout_plain_kernel, dim3((unsigned)((groups + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, crops,
                       alpha, w, groups_x, groups, reinterpret_cast<uint32_t*>(out));
    FCP_LAUNCH_OK();
    return 0;
  }
  const Colour fill = {packed_fill(bg_r, bg_g, bg_b)};
  if (mode == FCP_CUTOUT_RGBA) return estimate<true>(who, crops, alpha, f, h, w, fill, t, radius, out, workspace, workspace_bytes, s);
  return estimate<false>(who, crops, alpha, f, h, w, fill, t, radius, out, workspace, workspace_bytes, s);
}

extern "C" int fcp_cutout_image_u8(const uint8_t* crops, const uint8_t* alpha, int f, int h, int w, const uint8_t* pictures, int k,
                                   const int32_t* picks, const uint16_t* taps, int radius, uint8_t* out, void* workspace,
                                   int64_t workspace_bytes, fcp_stream_t stream) {
  const char* who = "cutout_image";
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_REQUIRE(radius != 0, "%s: the composite needs a radius: without an estimate it is fcp_matte_image_alpha_u8", who);
  FCP_REQUIRE(radius >= kMinRadius && radius <= kMaxRadius, "%s: radius must be %d..%d (got %d)", who, kMinRadius, kMaxRadius, radius);
  Taps t = {};
  FCP_CHECK(load_taps(who, taps, radius, &t));
  FCP_CHECK(check_pictures(who, k));
  if (f == 0) return 0;
  FCP_REQUIRE(crops && alpha && pictures && picks && out, "%s: null pointer", who);
  return estimate<false>(who, crops, alpha, f, h, w, Picture{pictures, picks, k}, t, radius, out, workspace, workspace_bytes,
                         (hipStream_t)stream);
}
