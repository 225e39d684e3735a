// Background blur of uint8 RGB crops from a per-pixel label map (Cropper(background_blur=...)):
// what is behind the subject is kept and blurred, by a wide Gaussian over the BACKGROUND pixels only, divided by the
// Gaussian weight of the background pixels it saw (a plain blur would smear the subject outward into a halo).
//
//   m, alpha  = the mask and the feathered alpha of fcp_feather.h (feather 0, 3, 5, 7): those of fcp_matte_u8
//   b(y,x)    = 1 where m == 0, else 0                                                          from the HARD mask
//   t[0..r]   : all >= 1, t[0] + 2 sum(t[1..r]) == 4096, 3 <= r <= 48; made on the host from sigma, data here
//   D(y,x)    = sum_j sum_i t|j| t|i| b(y+j, x+i)                                               taps inside the image only
//   N_ch(y,x) = sum_j sum_i t|j| t|i| b(y+j, x+i) c_ch(y+j, x+i)                                the same taps
//   B_ch(y,x) = D > 0 ? (N_ch + D / 2) / D : c_ch(y,x)                                          integer division
//   out_ch    = (c_ch alpha + B_ch (255 - alpha) + 127) / 255                                   fcp_feather.h's over255
//
// Positions outside the image contribute to neither N nor D: the normalisation is the border rule.  Bounds, all in
// unsigned 32 bits: a horizontal sum is at most 255 * 4096 < 2^20; N <= 255 * 4096^2 = 4 278 190 080 < 2^32 and
// N + D / 2 <= 4 286 578 688 < 2^32, only just, which is why the entry point refuses taps that do not sum to 4096;
// N <= 255 D, so B <= 255.  alpha < 255 needs a hard-background pixel within Chebyshev distance 3 inside the image
// (reflect-101 revisits in-image pixels only), every tap is >= 1 and r >= 3, so D > 0 wherever B shows; the D == 0
// branch only defines the bytes nobody sees.
//
// Two launches and a workspace of 16 bytes per pixel (the caller's: nothing is allocated here).
//
//   blur_rows_kernel, workgroups of 256 lanes over (4 rows x 256 columns, face).  A workgroup stages one dword per pixel
//   of its rows and an r-pixel margin, (b, b c_r, b c_g, b c_b) as four bytes, zero for a subject pixel and for a
//   position outside the image, so the border rule and the indicator cost nothing in the loop; then a lane per output
//   pixel runs the 2 r + 1 taps over consecutive dwords (consecutive lanes, consecutive banks) and stores the four sums
//   (H_b, H_r, H_g, H_b') as one 16-byte store.  LDS per workgroup: 4 x (256 + 96) x 4 B + 97 taps x 4 B = 6020 B (the
//   tap table is mirrored to 2 r + 1 entries, so the loop has no |k|).  27 workgroups would fit the 160 KiB of a CU; the
//   32 wave slots allow 8.
//
//   blur_cols_kernel, workgroups of 256 lanes over (64 rows x 16 columns, face), four pixels of a row per lane.  A
//   workgroup stages the 16-byte sums of its columns for rows y0 - r .. y0 + 63 + r (zero outside the image), and the
//   feather's tile (fcp_feather.h: Tile::stage); then a lane runs the 2 r + 1 taps down its four columns (four 16-byte
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
#include "fcp_feather.h"
#include "fcp_hip.h"

namespace {

using namespace fcp_crop_bytes;
using namespace fcp_feather;

constexpr int kThreads = 256;
constexpr int kMinRadius = 3;
constexpr int kMaxRadius = 48;
constexpr uint32_t kTapSum = 4096;

// rows pass
constexpr int kRowTileW = 256;
constexpr int kRowTileH = 4;
constexpr int kRowPitch = kRowTileW + 2 * kMaxRadius;   // dwords of a staged row

// columns pass
constexpr int kTileW = 16;              // output pixels of a tile row: 4 groups of four
constexpr int kTileH = 64;

struct BlurTaps {
  uint16_t t[kMaxRadius + 1];           // 49 x 16 bit in the kernel argument block
};

// the mirrored tap table, 2 r + 1 dwords: entry k is t|k - r|
__device__ __forceinline__ void stage_taps(uint32_t* tl, const BlurTaps& taps, int radius) {
  const int k = threadIdx.x;
  if (k <= 2 * radius) tl[k] = taps.t[k < radius ? radius - k : k - radius];
}

__global__ void __launch_bounds__(kThreads) blur_rows_kernel(const uint8_t* __restrict__ crops, const uint8_t* __restrict__ labels,
                                                             int h, int w, int tiles_x, uint32_t bits, BlurTaps taps, int radius,
                                                             uint4* __restrict__ sums) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* stage = reinterpret_cast<uint32_t*>(smem);   // kRowTileH rows of kRowPitch dwords
  uint32_t* tl = stage + kRowTileH * kRowPitch;
  const int f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kRowTileW, y0 = ty * kRowTileH;
  const int nrows = min(kRowTileH, h - y0), ncols = min(kRowTileW, w - x0);
  const int span = ncols + 2 * radius;

  stage_taps(tl, taps, radius);
  for (int i = threadIdx.x; i < nrows * span; i += kThreads) {
    const int tr = i / span, d = i - tr * span;
    const int x = x0 - radius + d;
    uint32_t v = 0;
    if (x >= 0 && x < w) {
      const size_t pixel = ((size_t)f * h + (y0 + tr)) * w + x;
      if (mask_of(labels[pixel], bits) == 0u) {
        const uint8_t* c = crops + pixel * 3;
        v = 1u | ((uint32_t)c[0] << 8) | ((uint32_t)c[1] << 16) | ((uint32_t)c[2] << 24);
      }
    }
    stage[tr * kRowPitch + d] = v;
  }
  __syncthreads();

  for (int i = threadIdx.x; i < nrows * ncols; i += kThreads) {
    const int tr = i / ncols, cx = i - tr * ncols;
    const uint32_t* s = stage + tr * kRowPitch + cx;   // output x sums staged x .. x + 2 r
    uint32_t a0 = 0u, a1 = 0u, a2 = 0u, a3 = 0u;        // each <= 255 * 4096
    for (int k = 0; k <= 2 * radius; ++k) {
      const uint32_t v = s[k], t = tl[k];
      a0 += t * (v & 255u);
      a1 += t * ((v >> 8) & 255u);
      a2 += t * ((v >> 16) & 255u);
      a3 += t * (v >> 24);
    }
    sums[((size_t)f * h + (y0 + tr)) * w + (x0 + cx)] = make_uint4(a0, a1, a2, a3);
  }
}

// Bytes of dynamic LDS of blur_cols_kernel<R>: the sums, the feather's tile, the taps.
template <int R>
constexpr size_t cols_lds_bytes(int radius) {
  return (size_t)(kTileH + 2 * radius) * kTileW * sizeof(uint4) + Tile<R, kTileW, kTileH>::kBytes +
         (2 * kMaxRadius + 1) * sizeof(uint32_t);
}

// crops and out may be the same array: neither is __restrict__.  Plane (with R == 0, fcp_matte_blur_alpha_u8): labels is an
// alpha plane the caller has (the refined one of fcp_matte_refine.hip), read as it is; N and D are those of the rows pass.
template <int R, bool Plane = false>
__global__ void __launch_bounds__(kThreads) blur_cols_kernel(const uint8_t* crops, const uint8_t* __restrict__ labels,
                                                             const uint4* __restrict__ sums, int h, int w, int tiles_x,
                                                             uint32_t bits, BlurTaps taps, int radius, uint8_t* out,
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
  // sums of rows y0 - r .. y0 + nrows + r - 1, all kTileW columns: zero outside the image
  for (int i = threadIdx.x; i < (nrows + 2 * radius) * kTileW; i += kThreads) {
    const int tr = i / kTileW, c = i - tr * kTileW;
    const int y = y0 - radius + tr, x = x0 + c;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (y >= 0 && y < h && x < w) v = sums[((size_t)f * h + y) * w + x];
    col[i] = v;
  }
  if constexpr (R > 0) Feather::stage(hsum, labels + (size_t)f * h * w, h, w, x0, y0, nrows, groups, bits, kThreads);
  __syncthreads();

  for (int i = threadIdx.x; i < nrows * groups; i += kThreads) {
    const int r = i / groups, g = i - r * groups;
    const int y = y0 + r, x = x0 + 4 * g;
    const int npx = min(4, w - x);
    const size_t pixel = ((size_t)f * h + y) * w + x;

    // D and N of the four pixels: N + D / 2 < 2^32
    uint32_t dn[4][4] = {};
    for (int k = 0; k <= 2 * radius; ++k) {
      const uint32_t t = tl[k];
      const uint4* p = col + (r + k) * kTileW + 4 * g;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint4 v = p[j];
        dn[j][0] += t * v.x;
        dn[j][1] += t * v.y;
        dn[j][2] += t * v.z;
        dn[j][3] += t * v.w;
      }
    }

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
      const uint32_t dd = dn[k / 3][0];
      const uint32_t bv = dd > 0u ? (dn[k / 3][1 + k % 3] + (dd >> 1)) / dd : cv;
      o[k >> 2] |= over255(cv, a[k / 3], bv) << (8 * (k & 3));
    }
    store_rgb(out + pixel * 3, npx, o);
  }
}

template <int R, bool Plane = false>
void launch_cols(const uint8_t* crops, const uint8_t* labels, const uint4* sums, int f, int h, int w, uint32_t bits,
                 const BlurTaps& taps, int radius, uint8_t* out, uint8_t* alpha, hipStream_t stream) {
  const int tiles_x = fcp_cdiv(w, kTileW), tiles_y = fcp_cdiv(h, kTileH);
  hipLaunchKernelGGL((blur_cols_kernel<R, Plane>), dim3(tiles_x * tiles_y, f), dim3(kThreads), cols_lds_bytes<R>(radius), stream,
                     crops, labels, sums, h, w, tiles_x, bits, taps, radius, out, alpha);
}

}  // namespace

extern "C" int64_t fcp_matte_blur_workspace_bytes(int f, int h, int w) {
  if (f < 0 || f > 65535 || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide) return -1;
  return (int64_t)f * h * w * (int64_t)sizeof(uint4);
}

namespace {

// Both entry points: `alpha_in` null is fcp_matte_blur_u8 (the feathered alpha, written to `alpha` when asked for), else
// fcp_matte_blur_alpha_u8 (the composite through the given plane).
int matte_blur(const char* who, const uint8_t* crops, const uint8_t* labels, const uint8_t* alpha_in, bool given, int f, int h, int w,
               uint32_t class_bits, int feather, const uint16_t* taps, int radius, uint8_t* out, uint8_t* alpha, void* workspace,
               int64_t workspace_bytes, fcp_stream_t stream) {
  FCP_REQUIRE(f >= 0 && h >= 1 && w >= 1, "%s: bad sizes (f %d, h %d, w %d)", who, f, h, w);
  FCP_REQUIRE(h <= kMaxSide && w <= kMaxSide, "%s: crops of at most %d x %d px (got h %d, w %d)", who, kMaxSide, kMaxSide, h, w);
  FCP_REQUIRE(f <= 65535, "%s: at most 65535 crops per call (got %d)", who, f);
  FCP_REQUIRE(feather == 0 || feather == 3 || feather == 5 || feather == 7, "%s: feather must be 0, 3, 5 or 7 (got %d)", who,
              feather);
  FCP_REQUIRE((class_bits >> kClasses) == 0, "%s: class_bits 0x%x names a class at or above %d", who, class_bits, kClasses);
  FCP_REQUIRE(radius >= kMinRadius && radius <= kMaxRadius, "%s: radius must be %d..%d (got %d)", who, kMinRadius, kMaxRadius,
              radius);
  FCP_REQUIRE(taps != nullptr, "%s: null taps", who);
  // the 32-bit sums of the kernels hold because of this
  BlurTaps t = {};
  uint32_t total = 0;
  for (int k = 0; k <= radius; ++k) {
    FCP_REQUIRE(taps[k] >= 1, "%s: tap %d is 0: every tap must be at least 1", who, k);
    t.t[k] = taps[k];
    total += (k == 0 ? 1u : 2u) * taps[k];
  }
  FCP_REQUIRE(total == kTapSum, "%s: the taps must sum to %u over the window (got %u)", who, kTapSum, total);
  if (f == 0) return 0;
  FCP_REQUIRE(crops && labels && out && (!given || alpha_in), "%s: null pointer", who);
  const int64_t need = fcp_matte_blur_workspace_bytes(f, h, w);
  FCP_REQUIRE(workspace != nullptr && workspace_bytes >= need, "%s: the workspace needs %lld bytes (got %lld)", who,
              (long long)need, (long long)workspace_bytes);
  FCP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  uint4* sums = static_cast<uint4*>(workspace);
  const int row_tiles_x = fcp_cdiv(w, kRowTileW), row_tiles_y = fcp_cdiv(h, kRowTileH);
  hipLaunchKernelGGL(blur_rows_kernel, dim3(row_tiles_x * row_tiles_y, f), dim3(kThreads),
                     (kRowTileH * kRowPitch + 2 * kMaxRadius + 1) * sizeof(uint32_t), s, crops, labels, h, w, row_tiles_x,
                     class_bits, t, radius, sums);
  FCP_LAUNCH_OK();
  if (given) {
    launch_cols<0, true>(crops, alpha_in, sums, f, h, w, class_bits, t, radius, out, nullptr, s);
  } else {
    switch (feather) {
      case 0: launch_cols<0>(crops, labels, sums, f, h, w, class_bits, t, radius, out, alpha, s); break;
      case 3: launch_cols<1>(crops, labels, sums, f, h, w, class_bits, t, radius, out, alpha, s); break;
      case 5: launch_cols<2>(crops, labels, sums, f, h, w, class_bits, t, radius, out, alpha, s); break;
      default: launch_cols<3>(crops, labels, sums, f, h, w, class_bits, t, radius, out, alpha, s); break;
    }
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
