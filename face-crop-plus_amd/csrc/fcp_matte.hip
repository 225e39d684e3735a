// Background replacement of uint8 RGB crops from a per-pixel label map (Cropper(background=...)):
//
//   alpha   = the feathered mask of the labels that class_bits names (fcp_feather.h: m, H, alpha; feather 0, 3, 5, 7)
//   out_ch  = (c_ch alpha + b_ch (255 - alpha) + 127) / 255                    fcp_feather.h's over255, b the fill
//
// One launch over (tile, face) workgroups of 256 lanes; a tile is 64 x 32 output pixels, four pixels of a row per lane
// and two such groups per lane.  A workgroup stages the mask of its tile and runs the horizontal pass into LDS
// (fcp_feather.h: Tile::stage); then a lane runs the vertical pass of a group in registers, reads the 12 crop bytes of
// the group, composites and writes out (and alpha) once.  feather 0 is its own instantiation with no LDS and no barrier.
// fcp_matte_alpha_u8 is the same composite with an alpha the caller has (the refined one of fcp_matte_refine.hip): the
// feather-0 instantiation once more, a group's four alpha bytes read from the plane where that one reads four labels.
// Every output byte has one writer and depends on its own crop pixel and on labels only, so out may be the crops
// themselves and the result is the same from run to run.
// fcp_feather_alpha_u8 is the alpha plane of fcp_matte_u8 alone (feather_alpha_kernel): the same tile and LDS, no crop.
// fcp_matte_image_u8 and fcp_matte_image_alpha_u8 are fcp_matte_u8 and fcp_matte_alpha_u8 over pictures (Cropper(
// background_image=...)): the same kernel with the fill source fcp_fill.h's Picture in place of
// Colour, so b is byte for byte the face's picture of a bank that stays on the device, read 12 bytes a group beside
// the crop's.  The tiles, the LDS and the one launch are the same; feather 0 and the plane still have no LDS and no barrier.
//
// The tile.  LDS per workgroup at r = 3: mask 38 rows x 72 B = 2736 B, H 38 rows x 128 B = 4864 B, 7600 B together: 21
// workgroups fit the 160 KiB of a CU, so the limit is the 32 wave slots of a CU: 8 workgroups of 4 waves, reached because
// the kernel needs fewer than 64 VGPRs (27 to 32 over a colour, 34 or 35 over pictures: the group's picture dwords and
// their address).  The halo costs (38 x 70) / (32 x 64) = 1.3 label bytes per pixel beside the 6
// crop bytes a pixel moves; a 256 x 256 crop is 32 tiles, so a batch of 8 fills the 256 CUs once.  Banks: the H rows are 128
// B, the 8-byte reads of 32 consecutive lanes (two tile rows of 16 groups) cover 256 contiguous bytes: no conflict.  The
// mask rows are 18 dwords, so the dword reads of a half wave (rows t and t + 1, 16 groups each) meet in two of the 32
// banks: one extra LDS cycle in a read of two, left alone.
//
// Rows are 3 w bytes and start at any byte (odd widths, offset views): crop, out, alpha and the feather-0 labels move by
// the rules of fcp_crop_bytes.h.  No byte outside the arrays is written, and no dword is read that does not hold a byte
// of them.
#include "fcp_common.h"
#include "fcp_crop_bytes.h"
#include "fcp_crop_checks.h"
#include "fcp_feather.h"
#include "fcp_fill.h"
#include "fcp_hip.h"

namespace {

using namespace fcp_crop_bytes;
using namespace fcp_crop_checks;
using namespace fcp_feather;
using fcp_fill::Colour;
using fcp_fill::Picture;

constexpr int kThreads = 256;
constexpr int kTileW = 64;             // output pixels of a tile row: 16 groups of four
constexpr int kTileH = 32;

// crops and out may be the same array: neither is __restrict__.  Plane (with R == 0): labels is an alpha plane, read as it is.
// Fill: fcp_fill.h's Colour or Picture.
template <int R, bool Plane = false, class Fill = Colour>
__global__ void __launch_bounds__(kThreads) matte_kernel(const uint8_t* crops, const uint8_t* __restrict__ labels, int h, int w,
                                                         int tiles_x, uint32_t bits, Fill fill, uint8_t* out,
                                                         uint8_t* alpha) {
  static_assert(!Plane || R == 0, "a given alpha has no feather");
  using Feather = Tile<R, kTileW, kTileH>;
  extern __shared__ uint2 lds[];         // R > 0: the feather's tile; R == 0: none
  const int f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const int nrows = min(kTileH, h - y0);
  const int groups = (min(kTileW, w - x0) + 3) >> 2;
  const auto behind = fill.face(f, h, w);

  if constexpr (R > 0) {
    Feather::stage(lds, labels + (size_t)f * h * w, h, w, x0, y0, nrows, groups, bits, kThreads);
    __syncthreads();
  }

  for (int i = threadIdx.x; i < nrows * groups; i += kThreads) {
    const int r = i / groups, g = i - r * groups;
    const int y = y0 + r, x = x0 + 4 * g;
    const int npx = min(4, w - x);
    const size_t pixel = ((size_t)f * h + y) * w + x;
    uint32_t a[4];
    if constexpr (Plane) {
      load_u8(labels + pixel, npx, a);
    } else {
      Feather::alpha(lds, r, g, labels + pixel, npx, bits, a);
      if (alpha != nullptr) store_u8(alpha + pixel, npx, a);
    }

    uint32_t c[3];
    load_rgb(crops + pixel * 3, npx, c);
    const auto b = behind.group((size_t)y * w + x, npx);
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 12; ++k) {            // byte k of the group: pixel k / 3, channel k % 3
      const uint32_t v = over255((c[k >> 2] >> (8 * (k & 3))) & 255u, a[k / 3], b.byte(k));
      o[k >> 2] |= v << (8 * (k & 3));
    }
    store_rgb(out + pixel * 3, npx, o);
  }
}

// matte_kernel without the composite: the alpha alone (fcp_feather_alpha_u8).  A kernel of its own: as a flag of
// matte_kernel, or with the tile loop of both in one function, the compiler orders the composite's arithmetic differently
// and the feather-0 instantiation needs two more registers.
template <int R>
__global__ void __launch_bounds__(kThreads) feather_alpha_kernel(const uint8_t* __restrict__ labels, int h, int w, int tiles_x,
                                                                 uint32_t bits, uint8_t* __restrict__ alpha) {
  using Feather = Tile<R, kTileW, kTileH>;
  extern __shared__ uint2 lds[];         // R > 0: the feather's tile; R == 0: none
  const int f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const int nrows = min(kTileH, h - y0);
  const int groups = (min(kTileW, w - x0) + 3) >> 2;

  if constexpr (R > 0) {
    Feather::stage(lds, labels + (size_t)f * h * w, h, w, x0, y0, nrows, groups, bits, kThreads);
    __syncthreads();
  }
  for (int i = threadIdx.x; i < nrows * groups; i += kThreads) {
    const int r = i / groups, g = i - r * groups;
    const int x = x0 + 4 * g;
    const int npx = min(4, w - x);
    const size_t pixel = ((size_t)f * h + (y0 + r)) * w + x;
    uint32_t a[4];
    Feather::alpha(lds, r, g, labels + pixel, npx, bits, a);
    store_u8(alpha + pixel, npx, a);
  }
}

// Composite false: feather_alpha_kernel, which takes labels, bits and alpha only.
template <int R, bool Plane = false, bool Composite = true, class Fill = Colour>
void launch(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t bits, Fill fill, uint8_t* out,
            uint8_t* alpha, hipStream_t stream) {
  const int tiles_x = fcp_cdiv(w, kTileW), tiles_y = fcp_cdiv(h, kTileH);
  constexpr size_t lds = Tile<R, kTileW, kTileH>::kBytes;
  const dim3 grid(tiles_x * tiles_y, f);
  if constexpr (Composite) {
    hipLaunchKernelGGL((matte_kernel<R, Plane, Fill>), grid, dim3(kThreads), lds, stream, crops, labels, h, w, tiles_x, bits, fill, out,
                       alpha);
  } else {
    hipLaunchKernelGGL(feather_alpha_kernel<R>, grid, dim3(kThreads), lds, stream, labels, h, w, tiles_x, bits, alpha);
  }
}

}  // namespace

extern "C" int fcp_matte_u8(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int feather,
                            int bg_r, int bg_g, int bg_b, uint8_t* out, uint8_t* alpha, fcp_stream_t stream) {
  const char* who = "matte";
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_CHECK(check_feather(who, feather));
  FCP_CHECK(check_fill(who, bg_r, bg_g, bg_b));
  FCP_CHECK(check_class_bits(who, class_bits));
  if (f == 0) return 0;
  FCP_REQUIRE(crops && labels && out, "%s: null pointer", who);
  with_feather(feather, [&](auto r) {
    launch<decltype(r)::value>(crops, labels, f, h, w, class_bits, Colour{packed_fill(bg_r, bg_g, bg_b)}, out, alpha,
                               (hipStream_t)stream);
  });
  FCP_LAUNCH_OK();
  return 0;
}

extern "C" int fcp_matte_alpha_u8(const uint8_t* crops, const uint8_t* alpha, int f, int h, int w, int bg_r, int bg_g, int bg_b,
                                  uint8_t* out, fcp_stream_t stream) {
  const char* who = "matte_alpha";
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_CHECK(check_fill(who, bg_r, bg_g, bg_b));
  if (f == 0) return 0;
  FCP_REQUIRE(crops && alpha && out, "%s: null pointer", who);
  launch<0, true>(crops, alpha, f, h, w, 0u, Colour{packed_fill(bg_r, bg_g, bg_b)}, out, nullptr, (hipStream_t)stream);
  FCP_LAUNCH_OK();
  return 0;
}

extern "C" int fcp_matte_image_u8(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int feather,
                                  const uint8_t* pictures, int k, const int32_t* picks, uint8_t* out, uint8_t* alpha,
                                  fcp_stream_t stream) {
  const char* who = "matte_image";
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_CHECK(check_feather(who, feather));
  FCP_CHECK(check_class_bits(who, class_bits));
  FCP_CHECK(check_pictures(who, k));
  if (f == 0) return 0;
  FCP_REQUIRE(crops && labels && pictures && picks && out, "%s: null pointer", who);
  with_feather(feather, [&](auto r) {
    launch<decltype(r)::value, false, true>(crops, labels, f, h, w, class_bits, Picture{pictures, picks, k}, out, alpha,
                                            (hipStream_t)stream);
  });
  FCP_LAUNCH_OK();
  return 0;
}

extern "C" int fcp_matte_image_alpha_u8(const uint8_t* crops, const uint8_t* alpha, int f, int h, int w, const uint8_t* pictures, int k,
                                        const int32_t* picks, uint8_t* out, fcp_stream_t stream) {
  const char* who = "matte_image_alpha";
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_CHECK(check_pictures(who, k));
  if (f == 0) return 0;
  FCP_REQUIRE(crops && alpha && pictures && picks && out, "%s: null pointer", who);
  launch<0, true, true>(crops, alpha, f, h, w, 0u, Picture{pictures, picks, k}, out, nullptr, (hipStream_t)stream);
  FCP_LAUNCH_OK();
  return 0;
}

extern "C" int fcp_feather_alpha_u8(const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int feather, uint8_t* alpha,
                                    fcp_stream_t stream) {
  const char* who = "feather_alpha";
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_CHECK(check_feather(who, feather));
  FCP_CHECK(check_class_bits(who, class_bits));
  if (f == 0) return 0;
  FCP_REQUIRE(labels && alpha, "%s: null pointer", who);
  with_feather(feather, [&](auto r) {
    launch<decltype(r)::value, false, false>(nullptr, labels, f, h, w, class_bits, Colour{0u}, nullptr, alpha, (hipStream_t)stream);
  });
  FCP_LAUNCH_OK();
  return 0;
}
