// Sharpness of uint8 RGB crops: the exact integer sums behind the variance of the Laplacian,
// cv2.Laplacian(cv2.cvtColor(crop, cv2.COLOR_RGB2GRAY), cv2.CV_64F).var()  (INTEGRATION.md section 2e):
//
//   g      = (9798 R + 19235 G + 3735 B + 16384) >> 15                     OpenCV's 8-bit RGB2GRAY
//   L(y,x) = g(y-1,x) + g(y+1,x) + g(y,x-1) + g(y,x+1) - 4 g(y,x)          ksize = 1, BORDER_REFLECT_101
//   S1 = sum L,  S2 = sum L*L   over the crop, as 64-bit integers          (the host divides: align.sharpness_score)
//
// One launch over (row strip, face) workgroups of 256 lanes.  A workgroup turns the RGB bytes of its strip and of the row
// above and below it (reflected at the crop's edge) into gray bytes in LDS, four pixels per lane (read by the rules of
// fcp_crop_bytes.h: rows are 3 w bytes and start at any byte) and aligned dword store,
// adds the reflected column left and right of every row, then every lane evaluates L for four pixels of a row from three
// dword and two byte LDS reads.  Integer sums commute: wave shuffle, LDS across the four waves, one pair of 64-bit atomic
// adds per workgroup, so the result is the same from run to run and for every strip height.
#include "fcp_common.h"
#include "fcp_crop_bytes.h"
#include "fcp_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileBytes = 32768;   // gray tile of a workgroup: (rows + 2) * pitch bytes at most, 5 workgroups per CU
constexpr int kMaxRows = 8;         // rows of a strip (fewer when the crop is wide: the tile has to fit kTileBytes)
constexpr int kMaxWidth = 8192;     // three tile rows (a strip of one row) of pitch 8200 still fit kTileBytes
constexpr int kMaxHeight = 1 << 20; // strips are grid.x: keeps grid.x * 256 lanes below 2^32 at one row per strip

// Per-lane accumulators.  A lane handles ceil(rows * chunks / 256) groups of four pixels; rows * pitch <= kTileBytes and
// pitch > 4 * chunks give rows * chunks < 8192, so at most 32 groups = 128 pixels per lane.  |L| <= 1020: |S1| <=
// 128 * 1020 = 130 560 fits an int; S2 <= 128 * 1 040 400 = 133 171 200 would fit 32 bits too, but it is kept in 64 bits so
// that no change of the tile constants can make it wrap (a 32-bit S2 holds 4128 extreme pixels, a wave's sum does not).
static_assert(kTileBytes / 4 / kThreads * 4 * 1020 < (1 << 30), "per-lane S1 must fit an int");

__device__ __forceinline__ uint32_t gray_of(uint32_t r, uint32_t g, uint32_t b) {
  return (9798u * r + 19235u * g + 3735u * b + 16384u) >> 15;
}

__device__ __forceinline__ int byte_of(uint32_t v, int j) { return (int)((v >> (8 * j)) & 255u); }

// Tile row layout (pitch = 4 * chunks + 8 bytes, chunks = ceil(w / 4)): [3 unused][g(reflected -1)][g(0) .. g(w-1)]
// [g(reflected w)][unused], so that pixel x sits at byte 4 + x and every group of four pixels is one aligned dword.
__global__ void __launch_bounds__(kThreads) crop_sharpness_kernel(const uint8_t* __restrict__ crops, int h, int w, int rows,
                                                                  const int32_t* __restrict__ ok,
                                                                  unsigned long long* __restrict__ sums) {
  extern __shared__ uint32_t tile32[];
  __shared__ long long part[2][kThreads / 64];
  const int f = blockIdx.y;
  if (ok != nullptr && ok[f] == 0) return;                       // the whole workgroup: its sums stay 0
  uint8_t* tile = reinterpret_cast<uint8_t*>(tile32);
  const int chunks = (w + 3) >> 2;
  const int pitch = 4 * chunks + 8;
  const int y0 = blockIdx.x * rows;
  const int nrows = min(rows, h - y0);
  const uint8_t* face = crops + (size_t)f * h * w * 3;

  // RGB -> gray, rows y0 - 1 .. y0 + nrows.  A lane takes the 12 bytes of four pixels, consecutive lanes consecutive
  // 12-byte pieces.
  for (int i = threadIdx.x; i < (nrows + 2) * chunks; i += kThreads) {
    const int r = i / chunks, c = i - r * chunks;
    int y = y0 - 1 + r;
    y = y < 0 ? (h > 1 ? 1 : 0) : (y >= h ? (h > 1 ? h - 2 : 0) : y);
    const int npx = min(4, w - 4 * c);
    uint32_t px[3];
    fcp_crop_bytes::load_rgb(face + ((size_t)y * w + 4 * c) * 3, npx, px);
    const uint32_t w0 = px[0], w1 = px[1], w2 = px[2];
    // pixels past the row's end (npx < 4) get a meaningless gray: bytes 4 + w .. of the tile row, which nothing reads
    // before the column pass below has written the one that matters
    const uint32_t g0 = gray_of(w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u);
    const uint32_t g1 = gray_of(w0 >> 24, w1 & 255u, (w1 >> 8) & 255u);
    const uint32_t g2 = gray_of((w1 >> 16) & 255u, w1 >> 24, w2 & 255u);
    const uint32_t g3 = gray_of((w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24);
    tile32[(r * pitch + 4 + 4 * c) >> 2] = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
  }
  __syncthreads();
  for (int r = threadIdx.x; r < nrows + 2; r += kThreads) {      // reflect-101 columns -1 and w (column 0 when w == 1)
    uint8_t* row = tile + r * pitch;
    row[3] = row[4 + (w > 1 ? 1 : 0)];
    row[4 + w] = row[4 + (w > 1 ? w - 2 : 0)];
  }
  __syncthreads();

  int s1 = 0;
  unsigned long long s2 = 0;
  for (int i = threadIdx.x; i < nrows * chunks; i += kThreads) {
    const int r = i / chunks, c = i - r * chunks;
    const uint8_t* row = tile + (r + 1) * pitch + 4 + 4 * c;
    const uint32_t up = *reinterpret_cast<const uint32_t*>(row - pitch);
    const uint32_t mid = *reinterpret_cast<const uint32_t*>(row);
    const uint32_t down = *reinterpret_cast<const uint32_t*>(row + pitch);
    const int left = row[-1], right = row[4];
    const int npx = min(4, w - 4 * c);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < npx) {
        const int l = j == 0 ? left : byte_of(mid, j - 1);
        const int rr = j == 3 ? right : byte_of(mid, j + 1);      // j + 1 == npx < 4: the reflected column, byte 4 + w
        const int lap = byte_of(up, j) + byte_of(down, j) + l + rr - 4 * byte_of(mid, j);
        s1 += lap;
        s2 += (unsigned long long)(unsigned)(lap * lap);
      }
    }
  }

  long long v1 = s1;
  unsigned long long v2 = s2;
  for (int off = 32; off > 0; off >>= 1) {
    v1 += __shfl_down(v1, off, 64);
    v2 += __shfl_down(v2, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = v1;
    part[1][threadIdx.x >> 6] = (long long)v2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t1 = 0, t2 = 0;
    for (int k = 0; k < kThreads / 64; ++k) {
      t1 += part[0][k];
      t2 += part[1][k];
    }
    atomicAdd(&sums[2 * (size_t)f], (unsigned long long)t1);    // two's complement: the signed S1 adds up modulo 2^64
    atomicAdd(&sums[2 * (size_t)f + 1], (unsigned long long)t2);
  }
}

}  // namespace

extern "C" int fcp_crop_sharpness_u8(const uint8_t* crops, int f, int h, int w, const int32_t* ok, int64_t* sums,
                                     fcp_stream_t stream) {
  FCP_REQUIRE(f >= 0 && h >= 1 && w >= 1, "crop_sharpness: bad sizes (f %d, h %d, w %d)", f, h, w);
  FCP_REQUIRE(w <= kMaxWidth, "crop_sharpness: crops of at most %d px wide (got %d): a strip of one row must fit the LDS tile",
              kMaxWidth, w);
  FCP_REQUIRE(h <= kMaxHeight, "crop_sharpness: crops of at most %d px high (got %d)", kMaxHeight, h);
  FCP_REQUIRE(f <= 65535, "crop_sharpness: at most 65535 crops per call");
  if (f == 0) return 0;
  FCP_REQUIRE(crops && sums, "crop_sharpness: null pointer");
  const int pitch = (w + 3) / 4 * 4 + 8;
  int rows = kTileBytes / pitch - 2;
  rows = rows > kMaxRows ? kMaxRows : rows;
  rows = rows > h ? h : rows;
  FCP_HIP_OK(hipMemsetAsync(sums, 0, (size_t)f * 2 * sizeof(int64_t), (hipStream_t)stream));
  hipLaunchKernelGGL(crop_sharpness_kernel, dim3(fcp_cdiv(h, rows), f), dim3(kThreads), (size_t)(rows + 2) * pitch,
                     (hipStream_t)stream, crops, h, w, rows, ok, reinterpret_cast<unsigned long long*>(sums));
  FCP_LAUNCH_OK();
  return 0;
}
