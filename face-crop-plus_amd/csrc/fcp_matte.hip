// Background replacement of uint8 RGB crops from a per-pixel label map (Cropper(background=...)):
//
//   m(y,x)  = 255 if l(y,x) < 32 and bit l(y,x) of class_bits is set, else 0
//   k       = feather 3: (64,128,64)   5: (16,64,96,64,16)   7: (8,28,56,72,56,28,8)      each sums to 256
//   H(y,x)  = sum_i k[i] m(y, R(x+i-r, w))            r = feather / 2;  H <= 65280: 16 bits, no rounding
//   alpha   = (sum_j k[j] H(R(y+j-r, h), x) + 32768) >> 16                    feather 0: alpha = m
//   out_ch  = (c_ch alpha + b_ch (255 - alpha) + 127) / 255                    round to nearest, no ties: 255 is odd
//
// R is BORDER_REFLECT_101 iterated until the index is inside (crops smaller than the radius); the two passes restate
// cv2.GaussianBlur(m, (K,K), 0) for CV_8U.  The division is u = t + 128; (u + (u >> 8)) >> 8, equal to (t + 127) / 255 for
// every t in 0 .. 65025.
//
// One launch over (tile, face) workgroups of 256 lanes; a tile is 64 x 32 output pixels, four pixels of a row per lane
// and two such groups per lane.  A workgroup
//   1. stages the mask bytes of its tile and an r-pixel halo in LDS, the reflected indices resolved here, four bytes
//      and one aligned dword store per lane;
//   2. runs the horizontal pass into 16-bit LDS: three dword reads, four sums, one 8-byte store per lane;
//   3. runs the vertical pass in registers (2r + 1 reads of 8 bytes per group), reads the 12 crop bytes of the group,
//      composites and writes out (and alpha) once.
// feather 0 is its own instantiation with no LDS and no barrier.  Every output byte has one writer and depends on its own
// crop pixel and on labels only, so out may be the crops themselves and the result is the same from run to run.
//
// The tile.  LDS per workgroup at r = 3: mask 38 rows x 72 B = 2736 B, H 38 rows x 128 B = 4864 B, 7600 B together: 21
// workgroups fit the 160 KiB of a CU, so the limit is the 32 wave slots of a CU: 8 workgroups of 4 waves, reached because
// the kernel needs fewer than 64 VGPRs.  The halo costs (38 x 70) / (32 x 64) = 1.3 label bytes per pixel beside the 6
// crop bytes a pixel moves; a 256 x 256 crop is 32 tiles, so a batch of 8 fills the 256 CUs once.  Banks: the H rows are 128
// B, the 8-byte reads of 32 consecutive lanes (two tile rows of 16 groups) cover 256 contiguous bytes: no conflict.  The
// mask rows are 18 dwords, so the dword reads of a half wave (rows t and t + 1, 16 groups each) meet in two of the 32
// banks: one extra LDS cycle in a read of two, left alone.
//
// Rows are 3 w bytes and start at any byte (odd widths, offset views).  Crop bytes are read as the aligned dwords that
// hold at least one byte of the group and shifted, as in fcp_sharpness.hip; out, alpha and the feather-0 labels go through
// dwords when the group is whole and its address aligned, through bytes otherwise.  No byte outside the arrays is written,
// and no dword is read that does not hold a byte of them.
#include "fcp_common.h"
#include "fcp_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64;             // output pixels of a tile row: 16 groups of four
constexpr int kTileH = 32;
constexpr int kGroups = kTileW / 4;
constexpr int kMaskPitch = kTileW + 8;  // bytes of a staged mask row: 64 + 2 * 3 halo, rounded up to dwords
constexpr int kMaxSide = 8192;
constexpr int kClasses = 19;

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

__device__ __forceinline__ bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

__device__ __forceinline__ uint32_t over255(uint32_t c, uint32_t a, uint32_t b) {
  const uint32_t u = c * a + b * (255u - a) + 128u;
  return (u + (u >> 8)) >> 8;
}

// crops and out may be the same array: neither is __restrict__.
template <int R>
__global__ void __launch_bounds__(kThreads) matte_kernel(const uint8_t* crops, const uint8_t* __restrict__ labels, int h, int w,
                                                         int tiles_x, uint32_t bits, uint32_t fill, uint8_t* out,
                                                         uint8_t* alpha) {
  extern __shared__ uint2 lds[];         // R > 0: H rows (8 bytes per group), then the mask rows; R == 0: none
  uint2* hsum = lds;
  uint32_t* mask32 = reinterpret_cast<uint32_t*>(lds + (kTileH + 2 * R) * kGroups);
  const int f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const int nrows = min(kTileH, h - y0);
  const int groups = (min(kTileW, w - x0) + 3) >> 2;
  const uint8_t* lab = labels + (size_t)f * h * w;

  if constexpr (R > 0) {
    // mask bytes of rows y0 - R .. y0 + nrows + R - 1, columns x0 - R .. x0 + 4 groups + R - 1 (to the next dword)
    const int mdw = (4 * groups + 2 * R + 3) >> 2;
    for (int i = threadIdx.x; i < (nrows + 2 * R) * mdw; i += kThreads) {
      const int tr = i / mdw, d = i - tr * mdw;
      const uint8_t* row = lab + (size_t)reflect101(y0 - R + tr, h) * w;
      uint32_t v = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) v |= mask_of(row[reflect101(x0 - R + 4 * d + j, w)], bits) << (8 * j);
      mask32[tr * (kMaskPitch / 4) + d] = v;
    }
    __syncthreads();
    // H of the same rows: output x of the tile sums mask bytes x .. x + 2 R
    for (int i = threadIdx.x; i < (nrows + 2 * R) * groups; i += kThreads) {
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
    __syncthreads();
  }

  for (int i = threadIdx.x; i < nrows * groups; i += kThreads) {
    const int r = i / groups, g = i - r * groups;
    const int y = y0 + r, x = x0 + 4 * g;
    const int npx = min(4, w - x);
    const size_t pixel = ((size_t)f * h + y) * w + x;
    uint32_t a[4];
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
      const uint8_t* lp = labels + pixel;
      if (npx == 4 && aligned4(lp)) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(lp);
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = mask_of((v >> (8 * j)) & 255u, bits);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = j < npx ? mask_of(lp[j], bits) : 0u;
      }
    }
    if (alpha != nullptr) {
      uint8_t* ap = alpha + pixel;
      if (npx == 4 && aligned4(ap)) {
        *reinterpret_cast<uint32_t*>(ap) = a[0] | (a[1] << 8) | (a[2] << 16) | (a[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < npx) ap[j] = (uint8_t)a[j];
      }
    }

    // the 3 * npx crop bytes of the group, from the aligned dwords that hold them (every dword read holds at least one)
    const uint8_t* cp = crops + pixel * 3;
    const int skew = (int)(reinterpret_cast<uintptr_t>(cp) & 3), nbytes = skew + 3 * npx;
    const uint32_t* p = reinterpret_cast<const uint32_t*>(cp - skew);
    const uint32_t d0 = p[0];
    const uint32_t d1 = nbytes > 4 ? p[1] : 0u;
    const uint32_t d2 = nbytes > 8 ? p[2] : 0u;
    const uint32_t d3 = nbytes > 12 ? p[3] : 0u;
    const int sh = 8 * skew;
    const uint32_t c[3] = {(uint32_t)((((uint64_t)d1 << 32) | d0) >> sh), (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh),
                           (uint32_t)((((uint64_t)d3 << 32) | d2) >> sh)};
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 12; ++k) {            // byte k of the group: pixel k / 3, channel k % 3
      const uint32_t v = over255((c[k >> 2] >> (8 * (k & 3))) & 255u, a[k / 3], (fill >> (8 * (k % 3))) & 255u);
      o[k >> 2] |= v << (8 * (k & 3));
    }
    uint8_t* op = out + pixel * 3;
    if (npx == 4 && aligned4(op)) {
      uint32_t* q = reinterpret_cast<uint32_t*>(op);
      q[0] = o[0];
      q[1] = o[1];
      q[2] = o[2];
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (k < 3 * npx) op[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
    }
  }
}

template <int R>
void launch(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t bits, uint32_t fill, uint8_t* out,
            uint8_t* alpha, hipStream_t stream) {
  const int tiles_x = fcp_cdiv(w, kTileW), tiles_y = fcp_cdiv(h, kTileH);
  const size_t lds = R > 0 ? (size_t)(kTileH + 2 * R) * (kGroups * sizeof(uint2) + kMaskPitch) : 0;
  hipLaunchKernelGGL(matte_kernel<R>, dim3(tiles_x * tiles_y, f), dim3(kThreads), lds, stream, crops, labels, h, w, tiles_x, bits,
                     fill, out, alpha);
}

}  // namespace

extern "C" int fcp_matte_u8(const uint8_t* crops, const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int feather,
                            int bg_r, int bg_g, int bg_b, uint8_t* out, uint8_t* alpha, fcp_stream_t stream) {
  FCP_REQUIRE(f >= 0 && h >= 1 && w >= 1, "matte: bad sizes (f %d, h %d, w %d)", f, h, w);
  FCP_REQUIRE(h <= kMaxSide && w <= kMaxSide, "matte: crops of at most %d x %d px (got h %d, w %d)", kMaxSide, kMaxSide, h, w);
  FCP_REQUIRE(f <= 65535, "matte: at most 65535 crops per call (got %d)", f);
  FCP_REQUIRE(feather == 0 || feather == 3 || feather == 5 || feather == 7, "matte: feather must be 0, 3, 5 or 7 (got %d)",
              feather);
  FCP_REQUIRE(bg_r >= 0 && bg_r <= 255 && bg_g >= 0 && bg_g <= 255 && bg_b >= 0 && bg_b <= 255,
              "matte: fill components must be 0..255 (got %d, %d, %d)", bg_r, bg_g, bg_b);
  FCP_REQUIRE((class_bits >> kClasses) == 0, "matte: class_bits 0x%x names a class at or above %d", class_bits, kClasses);
  if (f == 0) return 0;
  FCP_REQUIRE(crops && labels && out, "matte: null pointer");
  const uint32_t fill = (uint32_t)bg_r | ((uint32_t)bg_g << 8) | ((uint32_t)bg_b << 16);
  hipStream_t s = (hipStream_t)stream;
  switch (feather) {
    case 0: launch<0>(crops, labels, f, h, w, class_bits, fill, out, alpha, s); break;
    case 3: launch<1>(crops, labels, f, h, w, class_bits, fill, out, alpha, s); break;
    case 5: launch<2>(crops, labels, f, h, w, class_bits, fill, out, alpha, s); break;
    default: launch<3>(crops, labels, f, h, w, class_bits, fill, out, alpha, s); break;
  }
  FCP_LAUNCH_OK();
  return 0;
}
