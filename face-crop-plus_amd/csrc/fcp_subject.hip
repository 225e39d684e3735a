// One connected subject in a matte (Cropper(subject="largest", fill_holes=N)): connected-
// component labelling of the hard mask of the label map, per face, in integers, with H and W the crop's size:
//
//   m0(y,x) = 1 where labels(y,x) < 19 and bit labels(y,x) of class_bits is set, else 0     (fcp_feather.h's mask_of)
//   keep_largest: the 8-connected components of {m0 = 1}; the key of one is (its pixel count, then the SMALLER raster index
//                 y W + x of its first pixel in raster order); m1 = the component of the largest count, among equal counts
//                 the one whose first pixel comes first; no foreground pixel: m1 = m0.            otherwise m1 = m0
//   max_hole N:   the 4-connected components of {m1 = 0}; a hole is one without a pixel in row 0, row H - 1, column 0 or
//                 column W - 1; m2 = m1 plus every hole of at most N pixels.                      N = 0: m2 = m1
//   out(y,x) = m2(y,x), one byte, 0 or 1
//
// The label plane L is one int32 a pixel: the face-local raster index of a representative of the pixel's component, -1
// outside the set.  One invariant carries everything: L[x] <= x, and L[x] is in x's component.  Labels only ever
// decrease (atomicMin), so every find() strictly descends an integer, and the root a component ends with is its smallest
// raster index whatever the order of events: that is why the bytes are the same from run to run, and it is the tie rule.
//
// Widths.  A face-local index is below 8192 x 8192 = 2^26: int32, as is a component's area (<= 2^26), which shares its
// word with the border mark in bit 31; a sum of areas never carries there.  The key of the selection is the 64-bit
// (count << 32) | ~index.  Offsets into the planes are size_t.  No float.
//
// A workspace of 12 bytes per pixel (the caller's: nothing is allocated here), three int32 planes of f h w entries:
// L, A (the area and border mark of a tile-component, at its tile-local root, 0 elsewhere; after the flatten launch it
// is dead and its first word of a face holds the winner's index) and S (the same summed at the final root).  A pass
// writes every entry it later reads: the contents on entry are irrelevant.
//
// A pass over a set (the subject pass over {m0 = 1} at 8-connectivity, then the hole pass over {m1 = 0} at 4) is:
//
//   tile_kernel, (tile, face) workgroups of 256 lanes, a tile 64 x 32: stages the set's bits of the tile in LDS inside a
//   one-pixel frame of zeros, labels row runs (a lane per 8 pixels of a row), unites the runs of adjacent rows with LDS
//   atomicMin, flattens, counts every tile-component at its tile-local root with LDS atomics, and writes L, A and S = 0.
//   LDS: 33 x 68 frame bytes + 2 x 2048 x 4 = 18 628 B (8 workgroups a CU by the 160 KiB, the wave-slot limit).
//
//   seam_kernel, ONE workgroup of 1024 lanes a face, so that no workgroup depends on another inside the launch: walks the
//   pixel pairs across tile seams (with the two diagonals at 8-connectivity) and unites their roots with device-scope
//   atomicMin on L, deciding from the atomics' return values; every read of L here is a relaxed agent-scope atomic load,
//   since a plain load may be served by an L1 line older than an atomic's write.  (H / 32 - 1) W + (W / 64 - 1) H sites:
//   2560 at 256 x 256.
//
//   flatten_kernel, 256 pixels a workgroup: L is read-only now (the kernel boundary published it, plain loads); every
//   tile-local root adds its area and ORs its border mark into S at its final root: integer atomics, one per
//   tile-component, whose result does not depend on their order.
//
//   select_kernel (subject pass only), one workgroup of 1024 lanes a face: the maximum of (S << 32) | ~index over the
//   roots (L[p] == p), in a fixed tree through LDS; the winner's index goes to the face's first word of A.
//
//   write_subject_kernel / write_holes_kernel, 256 pixels a workgroup: out = (root == winner), or m1 | (the root's S has
//   no border mark and an area <= N).  The hole pass reads m1 from `out` when a subject pass wrote it there, otherwise m0
//   from the labels; keep_largest = 0, max_hole = 0 is one launch that writes m0.
//
// Launches: 5 for the subject, 4 for the holes, 9 for both.  Bytes per pixel of a pass: the tile launch reads 1 and writes
// 12, the flatten launch reads 4 (and 4 more of L per find step at a tile-local root), the select launch 8, the write
// launch 4 + 4 a find step + 4 of S in the hole pass and writes 1: about 34 for the subject pass and 26 for the holes,
// against the 55.5 of the background blur at sigma 8.
//
// No loop waits for another lane or workgroup; every loop below names the integer that bounds it.  labels and out may
// start at any byte (they are read and written as bytes); no byte outside out and the workspace is written.
#include "fcp_common.h"
#include "fcp_crop_checks.h"
#include "fcp_feather.h"
#include "fcp_hip.h"

namespace {

using namespace fcp_crop_checks;
using namespace fcp_feather;

constexpr int kThreads = 256;
constexpr int kFaceThreads = 1024;          // the one workgroup of a face (seam, select)
constexpr int kTileW = 64;
constexpr int kTileH = 32;
constexpr int kTilePx = kTileW * kTileH;
constexpr int kSeg = 8;                     // pixels of a row a lane labels
constexpr int kFramePitch = kTileW + 4;     // a zero column left and right of the tile, rounded up to dwords
constexpr int kFrameRows = kTileH + 1;      // a zero row above it
constexpr int kMaxHole = kMaxSide * kMaxSide;
constexpr uint32_t kBorderBit = 0x80000000u;
constexpr uint32_t kAreaMask = 0x7fffffffu;
constexpr int64_t kPlanes = 3;

constexpr size_t kTileLds = (size_t)kFrameRows * kFramePitch + 2 * (size_t)kTilePx * sizeof(int);
static_assert(kTileLds == 18628, "the LDS figure of the header");
static_assert(kTilePx == kThreads * kSeg && kTileW % kSeg == 0, "a lane per 8 pixels of a row");
static_assert((kFrameRows * kFramePitch) % 4 == 0, "the frame is cleared and followed by dwords");
static_assert(kMaxHole == 67108864 && kMaxHole < (1 << 30), "an area and the border mark share 32 bits");
static_assert(kFaceThreads * sizeof(unsigned long long) == 8192, "the select launch's LDS");

// which pixels a pass labels
enum Set { kForeground = 0, kBackgroundOfLabels = 1, kBackgroundOfOut = 2 };

// A relaxed atomic load of a label at the scope of the launch that reads it: the workgroup for the tile's labels in LDS,
// the agent for the label plane inside the seam launch (a plain load there may be served by an L1 line older than an
// atomic's write).
template <int kScope>
__device__ __forceinline__ int label_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, kScope);
}
constexpr int kTileScope = __HIP_MEMORY_SCOPE_WORKGROUP;
constexpr int kSeamScope = __HIP_MEMORY_SCOPE_AGENT;

// The root of x while other lanes unite.
template <int kScope>
__device__ __forceinline__ int find(const int* lab, int x) {
  for (int n = label_load<kScope>(lab + x); n != x; n = label_load<kScope>(lab + x)) x = n;   // bound: x, n < x, x >= 0
  return x;
}

// One component of a's and b's: the larger root is pointed at the smaller one with atomicMin (in LDS for the tile's
// labels, device-scope on the label plane), and the decision is taken from what the atomic returns.
template <int kScope>
__device__ __forceinline__ void unite(int* lab, int a, int b) {
  a = find<kScope>(lab, a);
  b = find<kScope>(lab, b);
  while (a != b) {                                                           // bound: max(a, b), smaller every turn, >= 0
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(lab + a, b);
    if (old == a) break;                                                     // a was a root and now points at b
    a = old;                                                                 // a pointed at old < a already: unite (old, b)
  }
}

// The root of x once the label plane is read-only (after the seam launch): plain loads.
__device__ __forceinline__ int find_plain(const int* __restrict__ lab, int x) {
  for (int n = lab[x]; n != x; n = lab[x]) x = n;                             // bound: x, n < x, x >= 0
  return x;
}

template <int kSet>
__device__ __forceinline__ uint32_t in_set(const uint8_t* src, size_t pixel, uint32_t bits) {
  if (kSet == kForeground) return mask_of(src[pixel], bits & ((1u << kClasses) - 1u)) & 1u;
  if (kSet == kBackgroundOfLabels) return (mask_of(src[pixel], bits & ((1u << kClasses) - 1u)) & 1u) ^ 1u;
  return src[pixel] == 0 ? 1u : 0u;
}

template <int kConn, int kSet>
__global__ void __launch_bounds__(kThreads) tile_kernel(const uint8_t* __restrict__ src, int h, int w, int tiles_x, uint32_t bits,
                                                        int* __restrict__ L, int* __restrict__ A, int* __restrict__ S) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[kTileLds];
  int* lab = reinterpret_cast<int*>(smem);
  int* cnt = lab + kTilePx;
  uint8_t* frame = reinterpret_cast<uint8_t*>(cnt + kTilePx);                // frame[(r + 1) * pitch + (c + 1)]: pixel (r, c)
  const int f = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  const size_t face = (size_t)f * h * w;

  for (int i = threadIdx.x; i < kFrameRows * kFramePitch / 4; i += kThreads)   // bound: i
    reinterpret_cast<uint32_t*>(frame)[i] = 0u;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kSeg; ++k) {
    const int p = k * kThreads + threadIdx.x, r = p / kTileW, c = p - r * kTileW;
    const int gy = y0 + r, gx = x0 + c;
    if (gy < h && gx < w) frame[(r + 1) * kFramePitch + c + 1] = (uint8_t)in_set<kSet>(src, face + (size_t)gy * w + gx, bits);
  }
  __syncthreads();

  // row runs: a pixel points at the start of its run inside the lane's 8 pixels, or at the pixel left of them
  const int r = threadIdx.x / (kTileW / kSeg), c0 = (threadIdx.x - r * (kTileW / kSeg)) * kSeg;
  const uint8_t* row = frame + (r + 1) * kFramePitch + c0 + 1;               // row[j]: pixel (r, c0 + j); row[-1] is readable
  const uint8_t* above = row - kFramePitch;
  const int i0 = r * kTileW + c0;
  {
    int run = -1;
#pragma unroll
    for (int j = 0; j < kSeg; ++j) {
      if (row[j]) {
        if (run < 0) run = (j == 0 && row[-1]) ? i0 - 1 : i0 + j;
      } else {
        run = -1;
      }
      lab[i0 + j] = run;
      cnt[i0 + j] = 0;
    }
  }
  __syncthreads();

  // the runs of adjacent rows; a pair that the pixel to the left unites as well is left to it
#pragma unroll
  for (int j = 0; j < kSeg; ++j) {
    if (!row[j]) continue;
    const bool up = above[j], ul = above[j - 1], ur = above[j + 1], lf = row[j - 1];
    if (up) {
      if (!(lf && ul)) unite<kTileScope>(lab, i0 + j, i0 + j - kTileW);
    } else if (kConn == 8) {
      if (ul && !lf) unite<kTileScope>(lab, i0 + j, i0 + j - kTileW - 1);
      if (ur) unite<kTileScope>(lab, i0 + j, i0 + j - kTileW + 1);
    }
  }
  __syncthreads();

  int root[kSeg];
#pragma unroll
  for (int j = 0; j < kSeg; ++j) root[j] = row[j] ? find<kTileScope>(lab, i0 + j) : -1;
  __syncthreads();
  // the area of a tile-component and its border mark at its root; equal roots of neighbouring pixels go as one add
  {
    const int gy = y0 + r;
    int pending = -1, n = 0;
    uint32_t mark = 0u;
#pragma unroll
    for (int j = 0; j < kSeg; ++j) {
      lab[i0 + j] = root[j];
      if (root[j] != pending) {
        if (pending >= 0) {
          atomicAdd(reinterpret_cast<uint32_t*>(cnt) + pending, (uint32_t)n);
          if (mark) atomicOr(reinterpret_cast<uint32_t*>(cnt) + pending, kBorderBit);
        }
        pending = root[j], n = 0, mark = 0u;
      }
      if (root[j] >= 0) {
        const int gx = x0 + c0 + j;
        ++n;
        if (gy == 0 || gy == h - 1 || gx == 0 || gx == w - 1) mark = 1u;
      }
    }
    if (pending >= 0) {
      atomicAdd(reinterpret_cast<uint32_t*>(cnt) + pending, (uint32_t)n);
      if (mark) atomicOr(reinterpret_cast<uint32_t*>(cnt) + pending, kBorderBit);
    }
  }
  __syncthreads();

#pragma unroll
  for (int k = 0; k < kSeg; ++k) {
    const int p = k * kThreads + threadIdx.x, pr = p / kTileW, pc = p - pr * kTileW;
    const int gy = y0 + pr, gx = x0 + pc;
    if (gy < h && gx < w) {
      const size_t pixel = face + (size_t)gy * w + gx;
      const int t = lab[p];
      int g = -1;
      if (t >= 0) {
        const int rr = t / kTileW;
        g = (y0 + rr) * w + x0 + (t - rr * kTileW);
      }
      L[pixel] = g;
      A[pixel] = t == p ? cnt[p] : 0;
      S[pixel] = 0;
    }
  }
}

template <int kConn>
__global__ void __launch_bounds__(kFaceThreads) seam_kernel(int* L, int h, int w, int tiles_x, int tiles_y) {
  int* lab = L + (size_t)blockIdx.x * h * w;
  const int nh = (tiles_y - 1) * w, nv = (tiles_x - 1) * h;                  // <= 255 x 8192 + 127 x 8192: int
  for (int i = threadIdx.x; i < nh + nv; i += kFaceThreads) {                // bound: nh + nv - i
    if (i < nh) {                                                            // the first row of a tile row against the row above
      const int k = i / w, x = i - k * w, y = (k + 1) * kTileH;
      const int p = y * w + x;
      if (label_load<kSeamScope>(lab + p) < 0) continue;
      if (label_load<kSeamScope>(lab + p - w) >= 0) {
        unite<kSeamScope>(lab, p, p - w);
      } else if (kConn == 8) {
        if (x > 0 && label_load<kSeamScope>(lab + p - w - 1) >= 0) unite<kSeamScope>(lab, p, p - w - 1);
        if (x + 1 < w && label_load<kSeamScope>(lab + p - w + 1) >= 0) unite<kSeamScope>(lab, p, p - w + 1);
      }
    } else {                                                                 // the first column of a tile column against the one left
      const int j = i - nh, k = j / h, y = j - k * h, x = (k + 1) * kTileW;
      const int p = y * w + x;
      if (label_load<kSeamScope>(lab + p) < 0) continue;
      if (label_load<kSeamScope>(lab + p - 1) >= 0) {
        unite<kSeamScope>(lab, p, p - 1);
      } else if (kConn == 8) {
        if (y > 0 && label_load<kSeamScope>(lab + p - w - 1) >= 0) unite<kSeamScope>(lab, p, p - w - 1);
        if (y + 1 < h && label_load<kSeamScope>(lab + p + w - 1) >= 0) unite<kSeamScope>(lab, p, p + w - 1);
      }
    }
  }
}

__global__ void __launch_bounds__(kThreads) flatten_kernel(const int* __restrict__ L, const int* __restrict__ A, uint32_t* S, int hw) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= hw) return;
  const size_t face = (size_t)blockIdx.y * hw;
  const uint32_t a = (uint32_t)A[face + p];
  if (a == 0u) return;
  const int root = find_plain(L + face, p);
  atomicAdd(S + face + root, a & kAreaMask);
  if (a & kBorderBit) atomicOr(S + face + root, kBorderBit);
}

__global__ void __launch_bounds__(kFaceThreads) select_kernel(const int* __restrict__ L, const uint32_t* __restrict__ S, int* A, int hw) {
  __shared__ unsigned long long keys[kFaceThreads];
  const size_t face = (size_t)blockIdx.x * hw;
  unsigned long long best = 0ull;                                            // a root's key is at least 1 << 32
  for (int p = threadIdx.x; p < hw; p += kFaceThreads) {                     // bound: hw - p
    if (L[face + p] == p) {
      const unsigned long long key = ((unsigned long long)(S[face + p] & kAreaMask) << 32) | (uint32_t)~(uint32_t)p;
      best = key > best ? key : best;
    }
  }
  keys[threadIdx.x] = best;
  __syncthreads();
  for (int s = kFaceThreads / 2; s > 0; s >>= 1) {                           // bound: s
    if ((int)threadIdx.x < s) {
      const unsigned long long o = keys[threadIdx.x + s];
      if (o > keys[threadIdx.x]) keys[threadIdx.x] = o;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) A[face] = keys[0] == 0ull ? -1 : (int)~(uint32_t)keys[0];
}

__global__ void __launch_bounds__(kThreads) write_subject_kernel(const int* __restrict__ L, const int* __restrict__ A, int hw,
                                                                 uint8_t* __restrict__ out) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= hw) return;
  const size_t face = (size_t)blockIdx.y * hw;
  const int winner = A[face];
  out[face + p] = (L[face + p] >= 0 && find_plain(L + face, p) == winner) ? 1 : 0;
}

__global__ void __launch_bounds__(kThreads) write_holes_kernel(const int* __restrict__ L, const uint32_t* __restrict__ S, int hw,
                                                               uint32_t max_hole, uint8_t* __restrict__ out) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= hw) return;
  const size_t face = (size_t)blockIdx.y * hw;
  uint8_t v = 1;                                                             // outside the set: m1 = 1
  if (L[face + p] >= 0) {
    const uint32_t s = S[face + find_plain(L + face, p)];
    v = (!(s & kBorderBit) && (s & kAreaMask) <= max_hole) ? 1 : 0;
  }
  out[face + p] = v;
}

__global__ void __launch_bounds__(kThreads) hard_mask_kernel(const uint8_t* __restrict__ labels, int hw, uint32_t bits,
                                                             uint8_t* __restrict__ out) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= hw) return;
  const size_t pixel = (size_t)blockIdx.y * hw + p;
  out[pixel] = (uint8_t)in_set<kForeground>(labels, pixel, bits);
}

template <int kConn, int kSet>
int label_pass(const uint8_t* src, int f, int h, int w, uint32_t bits, int* L, int* A, int* S, hipStream_t s) {
  const int tiles_x = fcp_cdiv(w, kTileW), tiles_y = fcp_cdiv(h, kTileH);
  hipLaunchKernelGGL((tile_kernel<kConn, kSet>), dim3(tiles_x * tiles_y, f), dim3(kThreads), 0, s, src, h, w, tiles_x, bits, L, A, S);
  FCP_LAUNCH_OK();
  hipLaunchKernelGGL(seam_kernel<kConn>, dim3(f), dim3(kFaceThreads), 0, s, L, h, w, tiles_x, tiles_y);
  FCP_LAUNCH_OK();
  hipLaunchKernelGGL(flatten_kernel, dim3(fcp_cdiv((long)h * w, kThreads), f), dim3(kThreads), 0, s, L, A,
                     reinterpret_cast<uint32_t*>(S), h * w);
  FCP_LAUNCH_OK();
  return 0;
}

}  // namespace

extern "C" int64_t fcp_subject_mask_workspace_bytes(int f, int h, int w) { return workspace_bytes(f, h, w, kPlanes * sizeof(int)); }

extern "C" int fcp_subject_mask_u8(const uint8_t* labels, int f, int h, int w, uint32_t class_bits, int keep_largest, int max_hole,
                                   uint8_t* out, void* workspace, int64_t workspace_bytes, fcp_stream_t stream) {
  const char* who = "subject_mask";
  FCP_CHECK(check_sizes(who, f, h, w));
  FCP_CHECK(check_class_bits(who, class_bits));
  FCP_REQUIRE(keep_largest == 0 || keep_largest == 1, "subject_mask: keep_largest must be 0 or 1 (got %d)", keep_largest);
  FCP_REQUIRE(max_hole >= 0 && max_hole <= kMaxHole, "subject_mask: max_hole must be 0..%d (got %d)", kMaxHole, max_hole);
  if (f == 0) return 0;
  FCP_REQUIRE(labels && out, "subject_mask: null pointer");
  FCP_CHECK(check_workspace(who, workspace, workspace_bytes, fcp_subject_mask_workspace_bytes(f, h, w)));
  hipStream_t s = (hipStream_t)stream;
  const size_t plane = (size_t)f * h * w;
  int* L = static_cast<int*>(workspace);
  int* A = L + plane;
  int* S = A + plane;
  const int hw = h * w;
  const dim3 pixels(fcp_cdiv(hw, kThreads), f);
  if (!keep_largest && max_hole == 0) {
    hipLaunchKernelGGL(hard_mask_kernel, pixels, dim3(kThreads), 0, s, labels, hw, class_bits, out);
    FCP_LAUNCH_OK();
    return 0;
  }
  if (keep_largest) {
    if (int rc = label_pass<8, kForeground>(labels, f, h, w, class_bits, L, A, S, s)) return rc;
    hipLaunchKernelGGL(select_kernel, dim3(f), dim3(kFaceThreads), 0, s, L, reinterpret_cast<const uint32_t*>(S), A, hw);
    FCP_LAUNCH_OK();
    hipLaunchKernelGGL(write_subject_kernel, pixels, dim3(kThreads), 0, s, L, A, hw, out);
    FCP_LAUNCH_OK();
  }
  if (max_hole > 0) {
    if (int rc = keep_largest ? label_pass<4, kBackgroundOfOut>(out, f, h, w, class_bits, L, A, S, s)
                              : label_pass<4, kBackgroundOfLabels>(labels, f, h, w, class_bits, L, A, S, s))
      return rc;
    hipLaunchKernelGGL(write_holes_kernel, pixels, dim3(kThreads), 0, s, L, reinterpret_cast<const uint32_t*>(S), hw,
                       (uint32_t)max_hole, out);
    FCP_LAUNCH_OK();
  }
  return 0;
}
