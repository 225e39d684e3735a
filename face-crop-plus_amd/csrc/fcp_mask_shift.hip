// Grow or shrink the matte (Cropper(edge_shift=N)): binary morphology of the hard mask of the
// label map with a Euclidean disc, per face, in integers, with r = |shift|:
//
//   m0(y,x) = 1 where labels(y,x) < 19 and bit labels(y,x) of class_bits is set, else 0     (fcp_feather.h's mask_of)
//   only positions inside the crop exist: a pixel outside it is neither subject nor background and never a source
//   shift > 0: out(y,x) = 1 iff some (y',x') inside the crop has m0 = 1 and (y - y')^2 + (x - x')^2 <= r^2
//   shift < 0: out(y,x) = 1 iff m0(y,x) = 1 and no (y',x') inside the crop has m0 = 0 and (y - y')^2 + (x - x')^2 <= r^2
//   shift = 0: out = m0
//   out(y,x) is one byte, 0 or 1
//
// Both directions are one question.  A source is a subject pixel for a grow and a background pixel for a shrink (a
// background pixel is its own source at distance 0, which is the m0 = 1 clause); reached(y,x) = some source lies in the
// disc around (y,x); out = reached for a grow and its complement for a shrink.  The disc is a stack of row segments: the
// source (y + dy, x + dx) is in it iff |dy| <= r and |dx| <= k(dy), k(dy) the largest k with k^2 + dy^2 <= r^2.  So
//
//   reached(y, .) = OR over dy = 0 .. r of  dilate(source(y - dy, .) | source(y + dy, .), k(dy))
//
// with dilate(s, k)(x) = OR of s(x - k .. x + k): the rows dy and -dy share a half-width and are ORed before they are
// widened.  A row of sources is a bit string, and 64 pixels of it widen at once.
//
// One launch over (tile, face) workgroups of 256 lanes, a tile 64 x 64 output pixels.
//
//   stage    the source bits of rows y0 - r .. y0 + 63 + r, columns x0 - r .. x0 + 63 + r in LDS, a row as three 64-bit
//            words (192 >= 64 + 2 r bits; bit c of a row is column x0 - r + c).  A wave takes staged rows, eight at a
//            time: for each of a row's words lane l reads the label byte of column x0 - r + 64 word + l where that
//            position is inside the crop and inside the span, and __ballot packs the wave's 64 answers into the word.
//            A position outside the crop is a 0 bit by that predicate; no address is clamped and none outside the face
//            is formed.  The 24 loads of eight rows are issued before the first ballot: the pass is a chain of load
//            latencies, three long at r = 2 and six at r = 64 (with four loads a turn the kernel took 21 us where it now
//            takes 15, 64 crops of 256 x 256 at r = 2).
//   widen    lane (row = t & 63, part = t >> 6): the tile row `row`, and of dy = 0 .. r those with dy % 4 == part (a
//            wave has one part, so dy and k are the same in all its lanes).  L = spread(s, k) has bit i = OR of
//            s(i - k .. i), by doubling: log2(k + 1) shift-ORs of the 192 bits and one more for the remainder; then
//            dilate(s, k) = L | (L >> k), of which bits r .. r + 63 are the tile's columns.  k(dy) only falls as dy rises:
//            a lane carries it along, r decrements in all.  The part's OR goes to LDS.
//   write    a wave takes tile rows, lane l column x0 + l: the OR of the row's four parts, bit l, complemented for a
//            shrink; one 64-byte row store per wave, inside the crop only.
//
// LDS: 192 rows x 24 B + 4 x 64 x 8 B = 6656 B, so the 32 wave slots of a CU, not the 160 KiB, set the 8 workgroups a CU.
// Banks: the widen pass reads 8-byte words at a lane stride of 24 B, six banks: no two lanes of a 32-lane half meet.
// Work per lane at r = 64: 17 row pairs of about 100 integer operations each; at r = 2 one pair.  The halo costs
// (64 + 2 r)^2 / 64^2 label bytes per output pixel: 1.13 at r = 2, 9 at r = 64.
//
// Widths: a face offset f h w reaches 65535 x 8192 x 8192 and is size_t; everything inside a face (< 2^26) and every
// shift count (1 .. 63, see spread and window) is int.  No float, no atomics, nothing allocated, no workspace: every output
// byte has one writer and depends on the labels only, so the bytes are the same from run to run.  labels and out may start
// at any byte (they move as bytes); they must not overlap, since a tile reads the halo that its neighbours write.
#include "fcp_common.h"
#include "fcp_crop_checks.h"
#include "fcp_feather.h"
#include "fcp_hip.h"

namespace {

using namespace fcp_crop_checks;
using namespace fcp_feather;

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kTile = 64;                    // output pixels of a tile, both ways: a row of it is one 64-bit word
constexpr int kMaxShift = 64;
constexpr int kWords = 3;                    // 64-bit words of a staged row
constexpr int kMaxRows = kTile + 2 * kMaxShift;
constexpr int kInFlight = 8;                 // staged rows a wave loads before it packs them: 24 loads in flight
constexpr uint32_t kNowhere = 0x100u;        // in place of a label byte: a position outside the crop or the span

static_assert(kWords * 64 >= kTile + 2 * kMaxShift, "a staged row holds the tile and both halos");
static_assert(kTile == kWave && kThreads == kWaves * kTile, "a lane per column when staging and writing, per (row, part) when widening");
static_assert(kMaxRows * kWords * 8 + kWaves * kTile * 8 == 6656, "the LDS figure of the header");

struct Row {
  uint64_t a, b, c;                          // bits 0..63, 64..127, 128..191
};

// x | (x << s) over the 192 bits, 1 <= s <= 63
__device__ __forceinline__ Row or_shl(Row x, int s) {
  Row y;
  y.c = x.c | (x.c << s) | (x.b >> (64 - s));
  y.b = x.b | (x.b << s) | (x.a >> (64 - s));
  y.a = x.a | (x.a << s);
  return y;
}

// bit i of the result = OR of x(i - k .. i), 0 <= k <= 64
__device__ __forceinline__ Row spread(Row x, int k) {
  int n = 1;                                 // bit i holds x(i - n + 1 .. i)
  for (; 2 * n <= k + 1; n *= 2) x = or_shl(x, n);   // bound: n doubles up to k + 1 <= 65; the shift n <= 32
  if (n < k + 1) x = or_shl(x, k + 1 - n);   // the largest power of two n <= k + 1: 1 <= k + 1 - n < n <= 64
  return x;
}

// bits n .. n + 63 of x, 0 <= n <= 128
__device__ __forceinline__ uint64_t window(Row x, int n) {
  const uint64_t lo = n < 64 ? x.a : n < 128 ? x.b : x.c;
  const uint64_t hi = n < 64 ? x.b : n < 128 ? x.c : 0ull;
  const int s = n & 63;
  return s ? (lo >> s) | (hi << (64 - s)) : lo;
}

__global__ void __launch_bounds__(kThreads) mask_shift_kernel(const uint8_t* __restrict__ labels, int h, int w, int tiles_x,
                                                              uint32_t bits, int r, uint32_t shrink, uint8_t* __restrict__ out) {
  __shared__ uint64_t src[kMaxRows * kWords];        // src[row * 3 + word]: the source bits of staged row `row`
  __shared__ uint64_t parts[kWaves * kTile];         // parts[part * 64 + row]
  const int f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTile, y0 = ty * kTile;
  const uint8_t* face = labels + (size_t)f * h * w;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int span = kTile + 2 * r;                    // staged rows, and the bits of one that matter

  for (int row0 = wave * kInFlight; row0 < span; row0 += kWaves * kInFlight) {   // bound: span - row0
    uint32_t label[kInFlight][kWords];               // kNowhere: no such position, which is neither subject nor background
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
#pragma unroll
      for (int v = 0; v < kWords; ++v) {
        const int row = row0 + u, c = v * 64 + lane;
        const int gy = y0 - r + row, gx = x0 - r + c;
        const bool inside = row < span && c < span && gy >= 0 && gy < h && gx >= 0 && gx < w;
        label[u][v] = inside ? face[(size_t)gy * w + gx] : kNowhere;
      }
    }
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
#pragma unroll
      for (int v = 0; v < kWords; ++v) {
        const uint32_t subject = mask_of(label[u][v], bits) & 1u;
        const uint64_t word = __ballot(label[u][v] != kNowhere && subject != shrink);
        if (lane == 0 && row0 + u < span) src[(row0 + u) * kWords + v] = word;
      }
    }
  }
  __syncthreads();

  {
    const int row = lane, part = wave;
    uint64_t reached = 0ull;
    int k = r;
    for (int dy = part; dy <= r; dy += kWaves) {     // bound: r - dy
      while (k * k + dy * dy > r * r) --k;           // bound: k, which stays >= 0 since dy <= r
      const uint64_t* up = src + (row + r - dy) * kWords;
      const uint64_t* down = src + (row + r + dy) * kWords;
      const Row l = spread(Row{up[0] | down[0], up[1] | down[1], up[2] | down[2]}, k);
      reached |= window(l, r) | window(l, r + k);
    }
    parts[part * kTile + row] = reached;
  }
  __syncthreads();

  const int gx = x0 + lane;
  for (int row = wave; row < kTile; row += kWaves) {  // bound: kTile - row
    const int gy = y0 + row;
    if (gy < h && gx < w) {
      uint64_t reached = 0ull;
#pragma unroll
      for (int p = 0; p < kWaves; ++p) reached |= parts[p * kTile + row];
      out[((size_t)f * h + gy) * w + gx] = (uint8_t)(((uint32_t)(reached >> lane) & 1u) ^ shrink);
    }
  }
}

}  // namespace

extern "C" int fcp_mask_shift_u8(const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int shift, uint8_t* out,
                                 fcp_stream_t stream) {
  const char* who = "mask_shift";
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_CHECK(check_class_bits(who, class_bits));
  FCP_REQUIRE(shift >= -kMaxShift && shift <= kMaxShift, "%s: shift must be %d..%d (got %d)", who, -kMaxShift, kMaxShift, shift);
  if (f == 0) return 0;
  FCP_REQUIRE(labels && out, "%s: null pointer", who);
  const int tiles_x = fcp_cdiv(w, kTile), tiles_y = fcp_cdiv(h, kTile);
  hipLaunchKernelGGL(mask_shift_kernel, dim3(tiles_x * tiles_y, f), dim3(kThreads), 0, (hipStream_t)stream, labels, h, w, tiles_x,
                     class_bits, shift < 0 ? -shift : shift, shift < 0 ? 1u : 0u, out);
  FCP_LAUNCH_OK();
  return 0;
}
