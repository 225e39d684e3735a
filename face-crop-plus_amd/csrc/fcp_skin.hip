// Parser-guided skin smoothing of uint8 RGB crops (Cropper(smooth_skin=S)), in integers: a
// bilateral filter that changes only pixels the label map calls skin and averages only over such pixels.  For one crop c
// (h,w,3), its label map l (h,w), the class bit set `bits`, the taps t[0..r], the range table rng[0..255] of uint16 and
// the amount A (tests/skin_ref.py is the numpy restatement):
//
//   g(p)     = (9798 R + 19235 G + 3735 B + 16384) >> 15                   the gray of min_sharpness (fcp_gray.h)
//   m(p)     = 1 if l(p) < 32 and bit l(p) of bits is set, else 0          fcp_feather::mask_of / 255; 0 outside the crop
//   s(o)     = (t[|oy|] t[|ox|] + 2048) >> 12                              o in [-r, r]^2, 3 <= r <= 24
//   w(p,o)   = m(p + o) ((s(o) min(rng[|g(p + o) - g(p)|], ONE) + 2048) >> 12)             ONE = 4096
//   W(p)     = sum over o of w(p,o)
//   b_c(p)   = (sum over o of w(p,o) c_c(p + o) + (W >> 1)) / W            c = R, G, B; floor division; W == 0: b = c(p)
//   alpha(p) = the feather-7 alpha of m, fcp_feather.h's (reflect-101 borders)
//   e(p)     = max(0, 2 alpha(p) - 255);   E(p) = (e(p) A + 128) >> 8      A = 1..256
//   out_c(p) = over255(b_c(p), E(p), c_c(p)) if m(p) == 1, else c_c(p)
//
// Positions outside the crop carry weight 0 (they are not reflected), so any h, w >= 1 will do.  Every tap is at most
// ONE, so s <= ONE and w <= ONE; a window has at most 49 x 49 = 2401 positions: unsigned 32-bit sums (the static_assert
// below).  Integer sums commute: the bytes do not depend on the tile or on the order of the offsets.
//
// One launch, no workspace, no float and no atomics.  A workgroup of 256 lanes owns a 32 x 64 tile of one crop; a lane
// owns a run of 8 consecutive pixels of one tile row.
//   exit     every lane reads the 8 labels of its run; a tile without a skin pixel (background, hair, clothes: the common
//            case) copies its bytes and returns before anything is staged.
//   stage    the tile and a halo of r, one dword a pixel: R, G, B and the gray in the top byte.  A pixel that is not skin
//            or lies outside the crop carries no weight, so neither its colour nor its gray is ever used: it is staged as
//            kNotSkin, a dword no pixel can have (gray 255 of black), and its crop bytes are not read.  Beside it the
//            range table, clamped at ONE, as 512 entries of which the upper 256 are 0, and the spatial weights s as r + 1
//            rows (one per |oy|) of s(|oy|, d) for d = -r - 8 .. r + 15, 0 where |d| > r.
//   window   per row oy of the window a lane walks the 2 r + 8 staged neighbours its run can see, 8 at a time.  A
//            neighbour is read once (one LDS dword: colour, gray and mask) and serves the 8 centres of the run from
//            registers: per (neighbour, centre) |g - g'| + (256 if the neighbour is not skin) in one v_sad, one table
//            read, the rounded product with s, and four multiply-adds.  The s of the 8 x 8 pairs of a step are 15
//            consecutive entries of the row's table, of which 8 are new per step (two 16-byte reads at a uniform
//            address): positions past the window have s = 0, so the steps need no edge case.  A lane whose run holds no
//            skin pixel skips the window; a wave of such lanes (8 x 64 pixels) costs nothing.
//   blend    after a barrier the feather tile (fcp_feather::Tile<3>) takes the place of the staged pixels, which are
//            spent; a lane divides, reads its 24 crop bytes, blends the skin pixels and writes the run once.
// LDS at radius r: (32 + 2 r) rows of 2 r + 73 dwords (the run's last step reads up to 8 entries past the halo; the odd
// pitch spreads the 8 rows of a wave over the banks), (r + 1) (2 r + 24) dwords of s and 1 KiB of table: 46 KiB at
// r = 24, 21 KiB at r = 9.  The allocation is dynamic, sized by the radius of the call, and leaves room for three
// workgroups a CU at r = 24 and seven at r = 9.  The lanes hold 32 sums, 16 weights, 8 grays and the 8 table reads of a
// neighbour, which are in flight together: 108 VGPRs, nothing spilled, four waves a SIMD.  So three workgroups a CU run
// at r = 24 and four at r = 9, and one workgroup's staging and barriers wait behind another's arithmetic.  The window is
// arithmetic, not memory: 617 vector instructions for the 64 pairs of a step beside 70 LDS reads.
// Addressing into crops, labels and out is size_t.  Rows are 3 w bytes and start at any byte: the run moves through
// fcp_crop_bytes.h, and no byte outside the arrays is touched.
#include "fcp_common.h"
#include "fcp_crop_bytes.h"
#include "fcp_crop_checks.h"
#include "fcp_feather.h"
#include "fcp_gray.h"
#include "fcp_hip.h"

namespace {

using namespace fcp_crop_bytes;
using namespace fcp_crop_checks;

constexpr int kThreads = 256;
constexpr int kTileW = 64;
constexpr int kTileH = 32;
constexpr int kRun = 8;                                 // pixels of a lane: 32 rows x 8 runs = 256 lanes
constexpr int kMinRadius = 3;
constexpr int kMaxRadius = 24;
constexpr uint32_t kOne = 4096;
constexpr int kMaxAmount = 256;
constexpr int kRange = 256;                             // entries of the range table
constexpr uint32_t kNotSkin = 0xff000000u;              // gray 255 of a black pixel: no pixel stages as this
using Feather = fcp_feather::Tile<3, kTileW, kTileH>;

struct Taps {
  uint16_t t[kMaxRadius + 1];                           // 25 x 16 bit in the kernel argument block
};

__host__ __device__ constexpr int pixel_pitch(int r) { return kTileW + 2 * r + kRun + 1; }             // dwords, odd
__host__ __device__ constexpr int pixel_rows(int r) { return kTileH + 2 * r; }
__host__ __device__ constexpr int weight_pitch(int r) { return (2 * r + 3 * kRun + 3) & ~3; }          // dwords
__host__ __device__ constexpr int steps(int r) { return (2 * r + kRun + kRun - 1) / kRun; }            // of 8 neighbours
__host__ __device__ constexpr size_t lds_bytes(int r) {
  return ((size_t)pixel_rows(r) * pixel_pitch(r) + 3) / 4 * 16 + (size_t)(r + 1) * weight_pitch(r) * 4 + 2 * kRange * sizeof(uint16_t);
}

static_assert(kThreads == kTileH * (kTileW / kRun) && kRun == 8, "a lane per run of two groups");
static_assert((2u * kMaxRadius + 1) * (2u * kMaxRadius + 1) == 2401u &&
                  2401ull * kOne * 255ull + 2401ull * kOne / 2 < (1ull << 32), "32-bit sums suffice");
static_assert((kOne * kOne + 2048u) >> 12 == kOne, "s and w stay at most ONE");
static_assert(kRun * steps(kMaxRadius) + kTileW - kRun <= pixel_pitch(kMaxRadius) &&
                  kRun * steps(kMinRadius) + kTileW - kRun <= pixel_pitch(kMinRadius), "the last step stays inside its row");
static_assert(kRun * (steps(kMaxRadius) + 1) <= weight_pitch(kMaxRadius) && kRun * (steps(kMinRadius) + 1) <= weight_pitch(kMinRadius),
              "the last step's weights are in the table");
static_assert(Feather::kBytes <= (size_t)pixel_rows(kMinRadius) * pixel_pitch(kMinRadius) * 4, "the feather fits where the pixels were");
static_assert(lds_bytes(kMaxRadius) <= 160 * 1024 / 3, "three workgroups per CU at the largest radius");

__global__ void __launch_bounds__(kThreads) skin_smooth_kernel(const uint8_t* __restrict__ crops, const uint8_t* __restrict__ labels,
                                                               int h, int w, int tiles_x, uint32_t bits, Taps taps, int radius,
                                                               const uint16_t* __restrict__ range, int amount,
                                                               uint8_t* __restrict__ out) {
  extern __shared__ uint4 smem[];
  const int t = threadIdx.x, f = blockIdx.y;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int y0 = tile_y * kTileH, x0 = tile_x * kTileW;
  const int py = t >> 3, px = (t & 7) * kRun;
  const int y = y0 + py, x = x0 + px;
  const bool inside = y < h && x < w;
  const uint8_t* crop = crops + (size_t)f * h * w * 3;
  const uint8_t* lab = labels + (size_t)f * h * w;
  const size_t first = ((size_t)f * h + (inside ? y : 0)) * w + (inside ? x : 0);      // the run's first pixel, of the batch

  // exit: a tile without a skin pixel is copied
  uint32_t skin = 0u;                                   // bit k: pixel k of the run is skin
  if (inside) {
#pragma unroll
    for (int g = 0; g < kRun / 4; ++g) {
      const int npx = min(4, w - (x + 4 * g));
      if (npx <= 0) break;
      uint32_t l[4];
      load_u8(labels + first + 4 * g, npx, l);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < npx && fcp_feather::mask_of(l[j], bits) != 0u) skin |= 1u << (4 * g + j);
    }
  }
  if (__syncthreads_or(skin != 0u) == 0) {
    if (inside) {
#pragma unroll
      for (int g = 0; g < kRun / 4; ++g) {
        const int npx = min(4, w - (x + 4 * g));
        if (npx <= 0) break;
        uint32_t c[3];
        load_rgb(crops + (first + 4 * g) * 3, npx, c);
        store_rgb(out + (first + 4 * g) * 3, npx, c);
      }
    }
    return;
  }

  // stage
  const int pitch = pixel_pitch(radius), rows = pixel_rows(radius), cols = kTileW + 2 * radius;
  const int wpitch = weight_pitch(radius);
  uint32_t* pixels = reinterpret_cast<uint32_t*>(smem);
  uint32_t* weights = reinterpret_cast<uint32_t*>(smem + ((size_t)rows * pitch + 3) / 4);
  uint16_t* table = reinterpret_cast<uint16_t*>(weights + (radius + 1) * wpitch);
  for (int i = t; i < rows * pitch; i += kThreads) {
    const int r = i / pitch, c = i - r * pitch;
    const int sy = y0 - radius + r, sx = x0 - radius + c;
    uint32_t v = kNotSkin;
    if (c < cols && sy >= 0 && sy < h && sx >= 0 && sx < w) {
      const size_t p = (size_t)sy * w + sx;
      if (fcp_feather::mask_of(lab[p], bits) != 0u) {
        const uint8_t* q = crop + p * 3;
        const uint32_t cr = q[0], cg = q[1], cb = q[2];
        v = cr | (cg << 8) | (cb << 16) | (fcp_gray::gray_of(cr, cg, cb) << 24);
      }
    }
    pixels[i] = v;
  }
  for (int i = t; i < (radius + 1) * wpitch; i += kThreads) {
    const int r = i / wpitch, d = i - r * wpitch - radius - kRun;
    const int ad = d < 0 ? -d : d;
    weights[i] = ad <= radius ? ((uint32_t)taps.t[r] * taps.t[ad] + 2048u) >> 12 : 0u;
  }
  for (int i = t; i < 2 * kRange; i += kThreads) table[i] = i < kRange ? (uint16_t)min((uint32_t)range[i], kOne) : (uint16_t)0;
  __syncthreads();

  // window
  const uint32_t* centre = pixels + (py + radius) * pitch + px + radius;
  uint32_t own[kRun];
#pragma unroll
  for (int k = 0; k < kRun; ++k) own[k] = centre[k];
  uint32_t acc[kRun][4];
#pragma unroll
  for (int k = 0; k < kRun; ++k) acc[k][0] = acc[k][1] = acc[k][2] = acc[k][3] = 0u;
  if (skin != 0u) {
    uint32_t gc[kRun];
#pragma unroll
    for (int k = 0; k < kRun; ++k) gc[k] = own[k] >> 24;
    const int nsteps = steps(radius);
    for (int oy = -radius; oy <= radius; ++oy) {
      const uint32_t* row = pixels + (py + radius + oy) * pitch + px;           // the neighbour at x - r of the run's first pixel
      const uint4* srow = reinterpret_cast<const uint4*>(weights + (oy < 0 ? -oy : oy) * wpitch);
      uint32_t e[2 * kRun];                                 // e[i] = s(oy, j0 - 8 + i), j0 the step's first neighbour
#pragma unroll
      for (int i = 0; i < kRun; ++i) e[kRun + i] = 0u;      // left of the first step: d < -r
      for (int c = 0; c < nsteps; ++c) {
        const uint4 lo = srow[2 * c + 2], hi = srow[2 * c + 3];
#pragma unroll
        for (int i = 0; i < kRun; ++i) e[i] = e[kRun + i];
        e[8] = lo.x, e[9] = lo.y, e[10] = lo.z, e[11] = lo.w, e[12] = hi.x, e[13] = hi.y, e[14] = hi.z, e[15] = hi.w;
#pragma unroll
        for (int jj = 0; jj < kRun; ++jj) {
          const uint32_t v = row[kRun * c + jj];
          const uint32_t gn = v >> 24, off = v == kNotSkin ? (uint32_t)kRange : 0u;
          const uint32_t nr = v & 255u, ng = (v >> 8) & 255u, nb = (v >> 16) & 255u;
          uint32_t rw[kRun];                                                     // the 8 table reads are in flight together
#pragma unroll
          for (int k = 0; k < kRun; ++k) rw[k] = table[__builtin_amdgcn_sad_u16(gn, gc[k], off)];   // |g' - g|, + 256 off the skin: weight 0
#pragma unroll
          for (int k = 0; k < kRun; ++k) {
            // s, the table and w are at most ONE and a colour at most 255: 24-bit multiplies are exact
            const uint32_t wgt = (__umul24(e[jj - k + kRun], rw[k]) + 2048u) >> 12;
            acc[k][0] += __umul24(wgt, nr);
            acc[k][1] += __umul24(wgt, ng);
            acc[k][2] += __umul24(wgt, nb);
            acc[k][3] += wgt;
          }
        }
      }
    }
  }

  // blend
  __syncthreads();                                       // the staged pixels are spent: the feather takes their place
  uint2* feather = reinterpret_cast<uint2*>(smem);
  const int nrows = min(kTileH, h - y0);
  const int groups = (min(kTileW, w - x0) + 3) >> 2;
  Feather::stage(feather, lab, h, w, x0, y0, nrows, groups, bits, kThreads);
  __syncthreads();
  if (!inside) return;
#pragma unroll
  for (int g = 0; g < kRun / 4; ++g) {
    const int npx = min(4, w - (x + 4 * g));
    if (npx <= 0) break;
    uint32_t c[3];
    load_rgb(crops + (first + 4 * g) * 3, npx, c);
    if (((skin >> (4 * g)) & 15u) != 0u) {
      uint32_t a[4];
      Feather::alpha(feather, py, (px >> 2) + g, nullptr, npx, bits, a);
      uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 4 * g + j;
        const uint32_t total = acc[k][3], half = total >> 1;
        const uint32_t ramp = a[j] > 127u ? 2u * a[j] - 255u : 0u;
        const uint32_t blend = (skin >> k) & 1u ? (ramp * (uint32_t)amount + 128u) >> 8 : 0u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int byte = 3 * j + ch;                       // byte of the group
          const uint32_t was = (c[byte >> 2] >> (8 * (byte & 3))) & 255u;
          const uint32_t mean = total != 0u ? (acc[k][ch] + half) / total : was;
          o[byte >> 2] |= fcp_feather::over255(mean, blend, was) << (8 * (byte & 3));
        }
      }
      c[0] = o[0], c[1] = o[1], c[2] = o[2];
    }
    store_rgb(out + (first + 4 * g) * 3, npx, c);
  }
}

}  // namespace

extern "C" int fcp_skin_smooth_u8(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t class_bits,
                                  const uint16_t* taps, int radius, const uint16_t* range_lut, int amount_q8, uint8_t* out,
                                  fcp_stream_t stream) {
  const char* who = "skin_smooth";
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_CHECK(check_class_bits(who, class_bits));
  FCP_REQUIRE(radius >= kMinRadius && radius <= kMaxRadius, "%s: radius must be %d..%d (got %d)", who, kMinRadius, kMaxRadius, radius);
  FCP_REQUIRE(taps != nullptr, "%s: null taps", who);
  Taps t = {};
  for (int k = 0; k <= radius; ++k) {
    FCP_REQUIRE(taps[k] <= kOne, "%s: tap %d is %u: every tap must be at most %u", who, k, (unsigned)taps[k], kOne);
    t.t[k] = taps[k];
  }
  FCP_REQUIRE(amount_q8 >= 1 && amount_q8 <= kMaxAmount, "%s: amount_q8 must be 1..%d (got %d)", who, kMaxAmount, amount_q8);
  if (f == 0) return 0;
  FCP_REQUIRE(crops && labels && range_lut && out, "%s: null pointer", who);
  FCP_REQUIRE((reinterpret_cast<uintptr_t>(range_lut) & 1) == 0, "%s: the range table must be 2-byte aligned", who);
  const uintptr_t pixels = (uintptr_t)f * h * w, bytes = pixels * 3, to = reinterpret_cast<uintptr_t>(out);
  const uintptr_t from = reinterpret_cast<uintptr_t>(crops), lab = reinterpret_cast<uintptr_t>(labels);
  FCP_REQUIRE(to + bytes <= from || from + bytes <= to, "%s: out must not overlap crops (out == crops included): a pixel reads its window",
              who);
  FCP_REQUIRE(to + bytes <= lab || lab + pixels <= to, "%s: out must not overlap labels", who);
  const int tiles_x = fcp_cdiv(w, kTileW), tiles_y = fcp_cdiv(h, kTileH);
  hipLaunchKernelGGL(skin_smooth_kernel, dim3(tiles_x * tiles_y, f), dim3(kThreads), lds_bytes(radius), (hipStream_t)stream, crops,
                     labels, h, w, tiles_x, class_bits, t, radius, range_lut, amount_q8, out);
  FCP_LAUNCH_OK();
  return 0;
}
