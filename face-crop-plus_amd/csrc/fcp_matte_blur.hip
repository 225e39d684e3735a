// Background blur of uint8 RGB crops from a per-pixel label map (Cropper(background_blur=...)):
// what is behind the subject is kept and blurred, by a wide Gaussian over the BACKGROUND pixels only, divided by the
// Gaussian weight of the background pixels it saw (a plain blur would smear the subject outward into a halo).
//
//   m, alpha  = the mask and the feathered alpha of fcp_feather.h (feather 0, 3, 5, 7): those of fcp_matte_u8
//   b(y,x)    = 1 where m == 0, else 0                                                          from the HARD mask
//   t, D, N, B: the mask-normalised Gaussian of fcp_masked_blur.h with the one side b; its 32-bit bounds are stated there
//   out_ch    = (c_ch alpha + B_ch (255 - alpha) + 127) / 255                                   fcp_feather.h's over255
//
// alpha < 255 needs a hard-background pixel within Chebyshev distance 3 inside the image (reflect-101 revisits in-image
// pixels only), every tap is >= 1 and r >= 3, so D > 0 wherever B shows; the D == 0 branch only defines the bytes nobody
// sees.
//
// Two launches and a workspace of 16 bytes per pixel (the caller's: nothing is allocated here).
//
//   blur_rows_kernel, workgroups of 256 lanes over (4 rows x 256 columns, face): fcp_masked_blur.h's rows_pass, one dword
//   per staged pixel.  LDS per workgroup: 4 x (256 + 96) x 4 B + 97 taps x 4 B = 6020 B.  27 workgroups would fit the
//   160 KiB of a CU; the 32 wave slots allow 8.
//
//   blur_cols_kernel, workgroups of 256 lanes over (64 rows x 16 columns, face), four pixels of a row per lane.  A
//   workgroup stages the 16-byte sums of its columns for rows y0 - r .. y0 + 63 + r (fcp_masked_blur.h: stage_cols), and the
//   feather's tile (fcp_feather.h: Tile::stage); then a lane runs the 2 r + 1 taps down its four columns (cols_taps: four 16-byte
//   LDS reads per tap, 16 accumulators), divides, runs the feather's vertical pass, reads the 12 crop bytes of its
//   group, composites and writes out (and alpha) once.  LDS per workgroup at r = 48 and feather 7:
//   160 x 16 x 16 B = 40960 B of sums + 70 x 32 B + 70 x 24 B of feather + 388 B of taps = 45268 B: 3 workgroups per CU
//   (160 KiB), 12 of 32 wave slots; at r = 24 (sigma 8) it is 28672 + 4308 B: 4 workgroups, the 5th misses by 1 KiB.
//
// Bytes per pixel, the floor of this form: the rows pass reads 4 (crop + label) and writes 16; the columns pass reads
// 16 x (64 + 2 r) / 64 of sums (28 at r = 24, 40 at r = 48), 1.5 of labels and 3 of crop, and writes 3: 55.5 at r = 24,
// 67.5 at r = 48, against the 7.3 of matte_kernel.  A single launch with a 2-D tile and a 48-pixel halo would move
// fewer bytes to and from memory but read its input (64 + 96)^2 / 64^2 = 6.25 times and keep one workgroup per CU.
//
// out MAY BE crops: every read of c that a neighbour needs happens in blur_rows_kernel, which has finished before
// blur_cols_kernel starts on the same stream; blur_cols_kernel reads c at its own pixels only (the centre of the
// composite), and each group of four pixels has one lane that reads, then writes it.  No scratch copy of out is taken.
// The result is the same from run to run: integer sums in a fixed order, one writer per byte.
//
// Rows are 3 w bytes and start at any byte.  The rows pass reads crop and label bytes as bytes.  The columns pass moves
// crop, out, alpha and the feather-0 labels by the rules of fcp_crop_bytes.h.  No byte outside the arrays is written,
// and no dword is read that does not hold a byte of them.
#include "fcp_common.h"
#include "fcp_crop_bytes.h"
#include "fcp_crop_checks.h"
#include "fcp_feather.h"
#include "fcp_hip.h"
#include "fcp_masked_blur.h"

namespace {

using namespace fcp_crop_bytes;
using namespace fcp_crop_checks;
using namespace fcp_feather;
using namespace fcp_masked_blur;

// columns pass
constexpr int kTileW = 16;              // output pixels of a tile row: 4 groups of four
constexpr int kTileH = 64;

__global__ void __launch_bounds__(kThreads) blur_rows_kernel(const uint8_t* __restrict__ crops, const uint8_t* __restrict__ labels,
                                                             int h, int w, int tiles_x, uint32_t bits, Taps taps, int radius,
                                                             uint4* __restrict__ sums) {
  rows_pass<1>(crops, labels, h, w, tiles_x, taps, radius, sums, [bits](uint32_t l) { return mask_of(l, bits) == 0u ? 0 : -1; });
}

// Bytes of dynamic LDS of blur_cols_kernel<R>: the sums, the feather's tile, the taps.
template <int R>
constexpr size_t cols_lds_bytes(int radius) {
  return (size_t)(kTileH + 2 * radius) * kTileW * sizeof(uint4) + Tile<R, kTileW, kTileH>::kBytes + kTapBytes;
}

// crops and out may be the same array: neither is __restrict__.  Plane (with R == 0, fcp_matte_blur_alpha_u8): labels is an
// alpha plane the caller has (the refined one of fcp_matte_refine.hip), read as it is; N and D are those of the rows pass.
template <int R, bool Plane = false>
__global__ void __launch_bounds__(kThreads) blur_cols_kernel(const uint8_t* crops, const uint8_t* __restrict__ labels,
                                                             const uint4* __restrict__ sums, int h, int w, int tiles_x,
                                                             uint32_t bits, Taps taps, int radius, uint8_t* out,
                                                             uint8_t* alpha) {
  static_assert(!Plane || R == 0, "a given alpha has no feather");
  using Feather = Tile<R, kTileW, kTileH>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4* col = reinterpret_cast<uint4*>(smem);                                    // (kTileH + 2 r) rows of kTileW sums
  uint2* hsum = reinterpret_cast<uint2*>(col + (kTileH + 2 * radius) * kTileW);   // R > 0: the feather's tile
  uint32_t* tl = reinterpret_cast<uint32_t*>(hsum) + Feather::kBytes / 4;
  const int f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const int nrows = min(kTileH, h - y0);
  const int groups = (min(kTileW, w - x0) + 3) >> 2;

  stage_taps(tl, taps, radius);
  stage_cols<1, kTileW, kTileW>(col, sums, f, h, w, x0, y0, nrows, radius);
  if constexpr (R > 0) Feather::stage(hsum, labels + (size_t)f * h * w, h, w, x0, y0, nrows, groups, bits, kThreads);
  __syncthreads();

  for (int i = threadIdx.x; i < nrows * groups; i += kThreads) {
    const int r = i / groups, g = i - r * groups;
    const int y = y0 + r, x = x0 + 4 * g;
    const int npx = min(4, w - x);
    const size_t pixel = ((size_t)f * h + y) * w + x;

    uint32_t dn[4][4] = {};
    cols_taps<1, kTileW>(col, tl, radius, r, g, dn);

    uint32_t a[4];
    if constexpr (Plane) {
      load_u8(labels + pixel, npx, a);
    } else {
      Feather::alpha(hsum, r, g, labels + pixel, npx, bits, a);
      if (alpha != nullptr) store_u8(alpha + pixel, npx, a);
    }

    uint32_t c[3];
    load_rgb(crops + pixel * 3, npx, c);
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 12; ++k) {            // byte k of the group: pixel k / 3, channel k % 3
      const uint32_t cv = (c[k >> 2] >> (8 * (k & 3))) & 255u;
      o[k >> 2] |= over255(cv, a[k / 3], normalised(dn[k / 3][1 + k % 3], dn[k / 3][0], cv)) << (8 * (k & 3));
    }
    store_rgb(out + pixel * 3, npx, o);
  }
}

template <int R, bool Plane = false>
void launch_cols(const uint8_t* crops, const uint8_t* labels, const uint4* sums, int f, int h, int w, uint32_t bits,
                 const Taps& taps, int radius, uint8_t* out, uint8_t* alpha, hipStream_t stream) {
  const int tiles_x = fcp_cdiv(w, kTileW), tiles_y = fcp_cdiv(h, kTileH);
  hipLaunchKernelGGL((blur_cols_kernel<R, Plane>), dim3(tiles_x * tiles_y, f), dim3(kThreads), cols_lds_bytes<R>(radius), stream,
                     crops, labels, sums, h, w, tiles_x, bits, taps, radius, out, alpha);
}

}  // namespace

extern "C" int64_t fcp_matte_blur_workspace_bytes(int f, int h, int w) { return workspace_bytes(f, h, w, sizeof(uint4)); }

namespace {

// Both entry points: `alpha_in` null is fcp_matte_blur_u8 (the feathered alpha, written to `alpha` when asked for), else
// fcp_matte_blur_alpha_u8 (the composite through the given plane).
int matte_blur(const char* who, const uint8_t* crops, const uint8_t* labels, const uint8_t* alpha_in, bool given, int f, int h, int w,
               uint32_t class_bits, int feather, const uint16_t* taps, int radius, uint8_t* out, uint8_t* alpha, void* workspace,
               int64_t workspace_bytes, fcp_stream_t stream) {
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_CHECK(check_feather(who, feather));
  FCP_CHECK(check_class_bits(who, class_bits));
  FCP_REQUIRE(radius >= kMinRadius && radius <= kMaxRadius, "%s: radius must be %d..%d (got %d)", who, kMinRadius, kMaxRadius,
              radius);
  Taps t = {};
  FCP_CHECK(load_taps(who, taps, radius, &t));
  if (f == 0) return 0;
  FCP_REQUIRE(crops && labels && out && (!given || alpha_in), "%s: null pointer", who);
  FCP_CHECK(check_workspace(who, workspace, workspace_bytes, fcp_matte_blur_workspace_bytes(f, h, w)));
  hipStream_t s = (hipStream_t)stream;
  uint4* sums = static_cast<uint4*>(workspace);
  const int row_tiles_x = fcp_cdiv(w, kRowTileW), row_tiles_y = fcp_cdiv(h, kRowTileH);
  hipLaunchKernelGGL(blur_rows_kernel, dim3(row_tiles_x * row_tiles_y, f), dim3(kThreads), rows_lds_bytes<1>(), s, crops, labels, h,
                     w, row_tiles_x, class_bits, t, radius, sums);
  FCP_LAUNCH_OK();
  if (given) {
    launch_cols<0, true>(crops, alpha_in, sums, f, h, w, class_bits, t, radius, out, nullptr, s);
  } else {
    with_feather(feather, [&](auto r) {
      launch_cols<decltype(r)::value>(crops, labels, sums, f, h, w, class_bits, t, radius, out, alpha, s);
    });
  }
  FCP_LAUNCH_OK();
  return 0;
}

}  // namespace

extern "C" int fcp_matte_blur_u8(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int feather,
                                 const uint16_t* taps, int radius, uint8_t* out, uint8_t* alpha, void* workspace,
                                 int64_t workspace_bytes, fcp_stream_t stream) {
  return matte_blur("matte_blur", crops, labels, nullptr, false, f, h, w, class_bits, feather, taps, radius, out, alpha, workspace,
                    workspace_bytes, stream);
}

extern "C" int fcp_matte_blur_alpha_u8(const uint8_t* crops, const uint8_t* labels, const uint8_t* alpha, int f, int h, int w,
                                       uint32_t class_bits, const uint16_t* taps, int radius, uint8_t* out, void* workspace,
                                       int64_t workspace_bytes, fcp_stream_t stream) {
  return matte_blur("matte_blur_alpha", crops, labels, alpha, true, f, h, w, class_bits, 0, taps, radius, out, nullptr, workspace,
                    workspace_bytes, stream);
}
