// Contrast-limited adaptive histogram equalisation of the luma of uint8 RGB crops (Cropper(clahe=...), INTEGRATION.md
// section 2h): cv2.createCLAHE(c, (g, g)).apply(Y) between cv2.cvtColor(COLOR_RGB2YCrCb) and cvtColor(COLOR_YCrCb2RGB),
// restated.  For one crop (h,w,3), grid g and clip limit c (tests/clahe_ref.py is the numpy restatement):
//
//   1. colour   Y  = (4899 R + 9617 G + 1868 B + 8192) >> 14
//               Cr = sat(((R - Y) 11682 + (128 << 14) + 8192) >> 14)      Cb = sat(((B - Y) 9241 + (128 << 14) + 8192) >> 14)
//               and back, from the equalised Y':
//               R  = sat(Y' + (((Cr - 128) 22987 + 8192) >> 14))          B  = sat(Y' + (((Cb - 128) 29049 + 8192) >> 14))
//               G  = sat(Y' + (((Cb - 128) (-5636) + (Cr - 128) (-11698) + 8192) >> 14))
//               sat clamps to 0..255, the shifts are arithmetic (floor) shifts of signed 32-bit values.
//   2. tiles    if h % g == 0 and w % g == 0 the luma plane is used as is; otherwise it is extended at the bottom by
//               g - h % g rows and at the right by g - w % g columns with BORDER_REFLECT_101 (index n + k reads n - 2 - k).
//               A dimension that is divisible already grows by a full g when the other one is not: OpenCV's rule, kept.
//               th, tw = extended size / g;  area = th tw.
//   3. LUT      per tile: hist = its 256-bin histogram;  clip = max(int(c area / 256), 1), in double, truncated (a value
//               of area or more clips nothing and is taken as area);  every bin above clip is cut to it, the excess summed
//               into clipped;  batch = clipped / 256 goes to every bin;  residual = clipped - 256 batch;  if residual > 0,
//               step = max(256 / residual, 1) and bin i gets + 1 iff i % step == 0 and i / step < residual;  s = the
//               inclusive prefix sum;  lut[i] = sat(rint(float(s[i]) * scale)),  scale = 255.0f / float(area): one
//               float32 division, one float32 multiply, round half to even.
//   4. apply    per pixel (y, x) of the crop, in float32, every operation rounded on its own, in this order:
//               inv_th = 1.0f / th;  tyf = y inv_th - 0.5f;  ty1 = floor(tyf);  ya = tyf - ty1;  ya1 = 1.0f - ya;  only then
//               ty2 = min(ty1 + 1, g - 1) and ty1 = max(ty1, 0);  the same in x;
//               res = (L[ty1][tx1][Y] xa1 + L[ty1][tx2][Y] xa) ya1 + (L[ty2][tx1][Y] xa1 + L[ty2][tx2][Y] xa) ya
//               Y'  = sat(rint(res))
//
// The library is built with -ffp-contract=off, so the float steps are not fused; scale, inv_th and inv_tw are computed
// once on the host and handed to the kernels.  Every int that becomes a float is at most 2^24 (h, w <= 4096): exact.
//
// Two launches on the caller's stream.
//
// clahe_lut_kernel, one 256-lane workgroup per (tile, face).  A lane takes four consecutive pixels of a tile row at a
// time, recomputes Y from the RGB bytes (the reflected rows and columns are resolved here: no extended plane exists) and
// counts them into the sub-histogram of its wave with 32-bit LDS atomics, runs of equal values inside the four as one add.
// Four sub-histograms (4 x 1 KiB) keep a flat background from serialising 256 lanes on one bin: at worst the 64 lanes of
// one wave meet, once per four pixels.  Then, one bin per lane: the four sub-histograms are summed, the excess over clip is
// reduced over the workgroup (xor shuffles, four wave totals through LDS), clip / batch / residual are applied, the 256
// bins are scanned (a wave scan by shuffles up, the wave totals through LDS) and the LUT byte is made; four lanes' bytes are
// gathered by shuffles down and every fourth lane stores one dword to luts[f][g][g][256].  Integer atomics commute, so the
// histogram, and with it every byte written, is the same from run to run.
// LDS 4096 + 32 B; it needs fewer than 64 VGPRs, so the limit is the 32 wave slots of a CU: 8 workgroups.  The kernel is
// bound by the LDS atomics, not by the 3 bytes a pixel reads.  With g = 1 one workgroup walks the whole crop: the
// definition of the issue (a tile is a workgroup), slow for crops of several megapixels and correct.
//
// clahe_apply_kernel, workgroups over (block, face).  The pixels with the same floor(tyf) and floor(txf) form a cell: g + 1
// cells in each direction, a tile wide and high, offset by half a tile (the first and last are half cells), and all pixels
// of a cell interpolate between the same four LUTs.  A block is at most 64 x 32 pixels of ONE cell, so a workgroup stages
// exactly four LUTs in LDS (1 KiB, one dword per lane) and every pixel then reads four LDS bytes.  Staging was picked over
// reading the LUT bytes through L2: a pixel needs four gathered bytes, 16 byte loads per lane and group next to its three
// crop dwords, against one coalesced dword per lane and block; the price is that the tiles of a 2 x 2 pixel grid (32 x 32,
// g = 16) give blocks of four pixels, which is a size nobody crops to.  The cell borders are found with the very float
// expression the pixels use (it is monotonic in y), so a lane's floor(tyf) IS the cell index of its block, also where
// y inv_th rounds across a border.  Blocks of cells that the crop does not reach (the extension) leave at once.
// Crop bytes move four pixels per lane, by the rules of fcp_crop_bytes.h.  Rows are 3 w bytes and start at any byte; no
// byte outside the arrays is written, and no dword is read that holds none of their bytes.  Every output pixel depends
// on its own input pixel and on the LUTs only, so out may be the crops.
// LDS 1 KiB, fewer than 64 VGPRs: 8 workgroups per CU (the wave slots).  A 256 x 256 crop at g = 8 is 49 blocks of 32 x 32
// and 32 half or quarter ones; it moves 6 bytes per pixel here and 3 in the LUT kernel, 9 in all.
#include "fcp_common.h"
#include "fcp_crop_bytes.h"
#include "fcp_hip.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBins = 256;
constexpr int kMaxGrid = 16;
constexpr int kMaxSide = 4096;          // area <= 2^24: every int -> float conversion is exact
constexpr int kBlockW = 64;             // pixels of an apply block: 16 groups of four, 32 rows, inside one cell
constexpr int kBlockH = 32;

__device__ __forceinline__ uint32_t luma(uint32_t r, uint32_t g, uint32_t b) {
  return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14;       // at most (16384 * 255 + 8192) >> 14 = 255
}

__device__ __forceinline__ int sat8(int v) { return min(max(v, 0), 255); }

// The npx (1..4) RGB pixels at cp as px[j] = R | G << 8 | B << 16.
__device__ __forceinline__ void load_group(const uint8_t* cp, int npx, uint32_t px[4]) {
  uint32_t c[3];
  fcp_crop_bytes::load_rgb(cp, npx, c);
  px[0] = c[0] & 0xffffffu;
  px[1] = ((c[0] >> 24) | (c[1] << 8)) & 0xffffffu;
  px[2] = ((c[1] >> 16) | (c[2] << 16)) & 0xffffffu;
  px[3] = c[2] >> 8;
}

__global__ void __launch_bounds__(kThreads) clahe_lut_kernel(const uint8_t* __restrict__ crops, int h, int w, int grid, int th,
                                                             int tw, uint32_t clip, float scale, uint32_t* __restrict__ luts) {
  __shared__ uint32_t hist[kWaves][kBins];
  __shared__ uint32_t wsum[2][kWaves];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int f = blockIdx.y, ty = blockIdx.x / grid, tx = blockIdx.x - ty * grid;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) hist[k][t] = 0u;
  __syncthreads();

  const uint8_t* crop = crops + (size_t)f * h * w * 3;
  uint32_t* mine = hist[wave];
  const int groups = (tw + 3) >> 2;                  // groups of four pixels in a tile row
  const int dq = kThreads / groups, dr = kThreads - dq * groups;
  int r = t / groups, g = t - r * groups;
  while (r < th) {
    const int ey = ty * th + r, y = ey < h ? ey : 2 * (h - 1) - ey;
    const int ex = tx * tw + 4 * g, npx = min(4, tw - 4 * g);
    const uint8_t* row = crop + (size_t)y * w * 3;
    uint32_t px[4];
    if (ex + npx <= w) {
      load_group(row + 3 * ex, npx, px);
    } else {                                         // the reflected columns: the right edge of the last tile column
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < npx) {
          const int x = ex + j < w ? ex + j : 2 * (w - 1) - (ex + j);
          const uint8_t* p = row + 3 * x;
          px[j] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        }
      }
    }
    uint32_t cur = 0u, run = 0u;                     // runs of equal luma inside the group are one add
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < npx) {
        const uint32_t v = luma(px[j] & 255u, (px[j] >> 8) & 255u, px[j] >> 16);
        if (run != 0u && v == cur) {
          ++run;
        } else {
          if (run != 0u) atomicAdd(&mine[cur], run);
          cur = v;
          run = 1u;
        }
      }
    }
    atomicAdd(&mine[cur], run);                      // npx >= 1: there is a run
    g += dr;
    r += dq;
    if (g >= groups) {
      g -= groups;
      ++r;
    }
  }
  __syncthreads();

  // one bin per lane from here
  uint32_t n = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
  uint32_t excess = n > clip ? n - clip : 0u;
  n -= excess;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) excess += __shfl_xor(excess, o);
  if (lane == 0) wsum[0][wave] = excess;
  __syncthreads();
  const uint32_t clipped = wsum[0][0] + wsum[0][1] + wsum[0][2] + wsum[0][3];
  const uint32_t batch = clipped >> 8, residual = clipped & 255u;
  n += batch;
  if (residual != 0u) {
    const uint32_t step = 256u / residual;           // residual <= 255: at least 1
    if ((uint32_t)t % step == 0u && (uint32_t)t / step < residual) ++n;
  }
  uint32_t s = n;                                    // inclusive scan: inside the wave, then the totals of the waves before
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(s, o);
    if (lane >= o) s += v;
  }
  if (lane == 63) wsum[1][wave] = s;
  __syncthreads();
  for (int k = 0; k < wave; ++k) s += wsum[1][k];
  const uint32_t b = (uint32_t)fminf(fmaxf(rintf((float)s * scale), 0.0f), 255.0f);
  const uint32_t v = b | (__shfl_down(b, 1) << 8) | (__shfl_down(b, 2) << 16) | (__shfl_down(b, 3) << 24);
  if ((t & 3) == 0) luts[((size_t)(f * grid + ty) * grid + tx) * (kBins / 4) + (t >> 2)] = v;
}

// floor(p * inv - 0.5f): the index of the LUT row (or column) above (left of) pixel p, before it is clamped: -1 .. g - 1
__device__ __forceinline__ int cell_of(int p, float inv) { return (int)floorf((float)p * inv - 0.5f); }

// The first p in 0..n with cell_of(p) >= k: the exact border ceil((k + 0.5) tile), moved to where the float expression puts it.
__device__ __forceinline__ int cell_begin(int k, int tile, float inv, int n) {
  if (k < 0) return 0;
  int c = min(((2 * k + 1) * tile + 1) >> 1, n);
  while (c > 0 && cell_of(c - 1, inv) >= k) --c;
  while (c < n && cell_of(c, inv) < k) ++c;
  return c;
}

// crops and out may be the same array: neither is __restrict__.
__global__ void __launch_bounds__(kThreads) clahe_apply_kernel(const uint8_t* crops, const uint32_t* __restrict__ luts, int h, int w,
                                                               int grid, int th, int tw, float inv_th, float inv_tw, int subs_x,
                                                               int subs, uint8_t* out) {
  __shared__ uint32_t lut32[4 * kBins / 4];          // [ty1][tx1], [ty1][tx2], [ty2][tx1], [ty2][tx2]
  const int t = threadIdx.x, f = blockIdx.y;
  const int cell = blockIdx.x / subs, sub = blockIdx.x - cell * subs;
  const int cy = cell / (grid + 1) - 1, cx = cell - (cy + 1) * (grid + 1) - 1;
  const int sy = sub / subs_x, sx = sub - sy * subs_x;
  const int y0 = cell_begin(cy, th, inv_th, h) + sy * kBlockH, x0 = cell_begin(cx, tw, inv_tw, w) + sx * kBlockW;
  const int nrows = min(kBlockH, cell_begin(cy + 1, th, inv_th, h) - y0), ncols = min(kBlockW, cell_begin(cx + 1, tw, inv_tw, w) - x0);
  if (nrows <= 0 || ncols <= 0) return;              // the whole workgroup: the cell ends before this block, or is empty

  const int ty1 = max(cy, 0), ty2 = min(cy + 1, grid - 1), tx1 = max(cx, 0), tx2 = min(cx + 1, grid - 1);
  {
    const int which = t >> 6;
    const int row = (which & 2) ? ty2 : ty1, col = (which & 1) ? tx2 : tx1;
    lut32[t] = luts[((size_t)(f * grid + row) * grid + col) * (kBins / 4) + (t & 63)];
  }
  __syncthreads();
  const uint8_t* lut = reinterpret_cast<const uint8_t*>(lut32);

  const int groups = (ncols + 3) >> 2;
  for (int i = t; i < nrows * groups; i += kThreads) {
    const int r = i / groups, g = i - r * groups;
    const int y = y0 + r, x = x0 + 4 * g;
    const int npx = min(4, x0 + ncols - x);
    const size_t pixel = ((size_t)f * h + y) * w + x;
    const float tyf = (float)y * inv_th - 0.5f;
    const float ya = tyf - (float)cy, ya1 = 1.0f - ya;               // floor(tyf) is cy all over the block
    uint32_t px[4];
    load_group(crops + pixel * 3, npx, px);
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < npx) {
        const int R = (int)(px[j] & 255u), G = (int)((px[j] >> 8) & 255u), B = (int)(px[j] >> 16);
        const int Y = (int)luma((uint32_t)R, (uint32_t)G, (uint32_t)B);
        const int cr = sat8(((R - Y) * 11682 + (128 << 14) + 8192) >> 14) - 128;
        const int cb = sat8(((B - Y) * 9241 + (128 << 14) + 8192) >> 14) - 128;
        const float txf = (float)(x + j) * inv_tw - 0.5f;
        const float xa = txf - (float)cx, xa1 = 1.0f - xa;
        const float res = ((float)lut[Y] * xa1 + (float)lut[kBins + Y] * xa) * ya1 +
                          ((float)lut[2 * kBins + Y] * xa1 + (float)lut[3 * kBins + Y] * xa) * ya;
        const int yn = (int)fminf(fmaxf(rintf(res), 0.0f), 255.0f);
        const uint32_t rgb[3] = {(uint32_t)sat8(yn + ((cr * 22987 + 8192) >> 14)),
                                 (uint32_t)sat8(yn + ((cb * -5636 + cr * -11698 + 8192) >> 14)),
                                 (uint32_t)sat8(yn + ((cb * 29049 + 8192) >> 14))};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int k = 3 * j + c;                                   // byte k of the group
          o[k >> 2] |= rgb[c] << (8 * (k & 3));
        }
      }
    }
    fcp_crop_bytes::store_rgb(out + pixel * 3, npx, o);
  }
}

}  // namespace

extern "C" int fcp_clahe_u8(const uint8_t* crops, int f, int h, int w, int grid, double clip_limit, uint8_t* luts, uint8_t* out,
                            fcp_stream_t stream) {
  FCP_REQUIRE(grid >= 1 && grid <= kMaxGrid, "clahe: grid must be 1..%d (got %d)", kMaxGrid, grid);
  FCP_REQUIRE(f >= 0 && h >= 2 * grid && w >= 2 * grid, "clahe: bad sizes (f %d, h %d, w %d): h and w must be at least 2 * grid = %d",
              f, h, w, 2 * grid);
  FCP_REQUIRE(h <= kMaxSide && w <= kMaxSide, "clahe: crops of at most %d x %d px (got h %d, w %d)", kMaxSide, kMaxSide, h, w);
  FCP_REQUIRE(f <= 65535, "clahe: at most 65535 crops per call (got %d)", f);
  FCP_REQUIRE(std::isfinite(clip_limit) && clip_limit > 0.0, "clahe: clip_limit must be finite and > 0 (got %g)", clip_limit);
  if (f == 0) return 0;
  FCP_REQUIRE(crops && luts && out, "clahe: null pointer");
  FCP_REQUIRE((reinterpret_cast<uintptr_t>(luts) & 3) == 0, "clahe: the LUT workspace must be 4-byte aligned");
  int eh = h, ew = w;
  if (h % grid != 0 || w % grid != 0) {
    eh += grid - h % grid;
    ew += grid - w % grid;
  }
  const int th = eh / grid, tw = ew / grid, area = th * tw;
  const double limit = clip_limit * area / 256;
  const uint32_t clip = limit >= (double)area ? (uint32_t)area : (uint32_t)(limit >= 1.0 ? (int)limit : 1);
  const float scale = 255.0f / (float)area, inv_th = 1.0f / (float)th, inv_tw = 1.0f / (float)tw;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* luts32 = reinterpret_cast<uint32_t*>(luts);
  hipLaunchKernelGGL(clahe_lut_kernel, dim3(grid * grid, f), dim3(kThreads), 0, s, crops, h, w, grid, th, tw, clip, scale, luts32);
  FCP_LAUNCH_OK();
  // a cell is th (tw) high (wide), one more where the float expression puts a border that is an integer (th even) one
  // pixel further: blocks past the end of their cell leave at once
  const int subs_y = fcp_cdiv(th + 1, kBlockH), subs_x = fcp_cdiv(tw + 1, kBlockW), subs = subs_y * subs_x;
  hipLaunchKernelGGL(clahe_apply_kernel, dim3((grid + 1) * (grid + 1) * subs, f), dim3(kThreads), 0, s, crops, luts32, h, w, grid, th,
                     tw, inv_th, inv_tw, subs_x, subs, out);
  FCP_LAUNCH_OK();
  return 0;
}
