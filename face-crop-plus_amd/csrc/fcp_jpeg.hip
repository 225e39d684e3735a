// Baseline JPEG entropy-coded segments of uint8 crops (f,h,w,c), c = 3 (RGB; 4:4:4, 4:2:2 or 4:2:0) or 1 (gray), on the
// device: byte for byte what libjpeg-turbo's compressor writes between the SOS header and the end of the file, with the
// standard Huffman tables or with tables made for the face (libjpeg's optimize_coding) (INTEGRATION.md sections 2f and
// 2j; the header itself is jpegenc.jpeg_header, on the host).  Four kernels after one memset:
//
//   transform   one lane per 8x8 block, blocks in scan (MCU) order: 16-bit scaled RGB -> YCbCr, edge replication, chroma at
//               full resolution (4:4:4), as the pair average with the alternating 0, 1 bias (4:2:2) or as the 2x2
//               average with the alternating 1, 2 bias (4:2:0), the 13-bit integer forward DCT ("islow", output scaled by
//               8), division by 8 Q rounding half away from zero; 64 int16 per block, zig-zag order, to the workspace
//   count_scan  one workgroup per face: Huffman bit count of every block (DC difference against the block before it of
//               the same component), exclusive scan over the face -> the bit offset of every block
//   emit        one lane per block: the block's code bits, shifted to its offset, into 32-bit big-endian words; words a
//               block owns alone are stored, the two it may share with its neighbours are OR-ed with ordinary global
//               atomics (OR commutes: the words do not depend on the order), the last block adds the 1-bits of the pad
//   stuff       one workgroup per face: FF -> FF 00 with output positions from a scan of per-lane FF counts, then EOI
//               and the length; every store is checked against the caller's capacity
//
// and, with optimised tables, two more between transform and count_scan:
//
//   histogram   one lane per block, the same walk over its symbols as count_scan and emit: the frequency of every symbol
//               per face and table (Y DC, Y AC, chroma DC, chroma AC), through per-wave LDS histograms and integer
//               global atomics (adds commute: the counts do not depend on the order)
//   tables      one wave per table: libjpeg's jpeg_gen_optimal_table restated -> the table's 272-byte record for the
//               header and 256 x (code | length << 16) for count_scan and emit, which stage the face's own tables in LDS
//
// The chroma subsampling is a template argument of the kernels (an MCU is hs * vs Y blocks, then Cb, then Cr); gray crops
// run the 4:2:0 instances.  An MCU that overhangs an odd Y block grid carries dummy blocks: all AC zero and the DC of the
// block before them, i.e. a zero DC difference and an end-of-block, and the DC prediction passes through them unchanged.
// They are never transformed.
#include "fcp_block_scan.h"
#include "fcp_common.h"
#include "fcp_entropy.h"
#include "fcp_hip.h"

namespace {

using fcp_entropy::kFib35;
using fcp_entropy::round16;

constexpr int kThreads = 256;
constexpr int kMaxSide = 8192;          // 6 * 512 * 512 blocks * 1658 bits < 2^32: bit offsets of a face fit 32 bits
constexpr int kMaxBlockBits = 20 + 63 * 26;   // DC: 9-bit code + 11 bits; 63 x (16-bit code + 10 bits); no ZRL can join them
constexpr int kMaxBlockBitsOpt = 27 + 63 * 26;   // optimised tables: a DC code may be 16 bits long as well
constexpr int kTableBytes = 272;              // a table's record: 16 counts + up to 256 symbols in code order, zero padded
constexpr int kMaxCodeLength = 32;            // libjpeg's MAX_CLEN: the lengths its arrays hold before the limit to 16

// zig-zag position -> natural (row-major) index
constexpr int kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// T.81 Annex K.1 quantisation tables (natural order) and K.3 Huffman tables (codes per length, symbols in code order)
const uint8_t kQuantBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61,  12, 12, 14, 19, 26, 58, 60, 55,  14, 13, 16, 24, 40, 57, 69, 56,  14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77,  24, 35, 55, 64, 81, 104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101,
     72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99,  18, 21, 26, 66, 99, 99, 99, 99,  24, 26, 56, 99, 99, 99, 99, 99,  47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99,  99, 99, 99, 99, 99, 99, 99, 99,  99, 99, 99, 99, 99, 99, 99, 99,  99, 99, 99, 99, 99, 99, 99, 99}};
const uint8_t kDcCounts[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kAcCounts[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
const uint8_t kAcSymbols[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,
     35,  66,  177, 193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,
     41,  42,  52,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,
     90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137,
     138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182,
     183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226,
     227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145,
     161, 177, 193, 9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,
     39,  40,  41,  42,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,
     89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135,
     136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180,
     181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
     226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

struct QuantArg {
  uint16_t div[2][64];          // 8 * Q per zig-zag position: the DCT's output carries a factor of 8
};
struct HuffArg {
  uint32_t dc[2][12];           // code | length << 16, by size category
  uint32_t ac[2][256];          // code | length << 16, by run << 4 | size
};

// Where the blocks of a face are.  One component: blocks row by row.  Three: MCUs of hs * vs Y blocks row by row, Cb, Cr.
struct Geometry {
  int h, w, c;
  int ybw, ybh;                 // Y block grid: ceil(w / 8), ceil(h / 8)
  int mw;                       // MCUs (c == 3) or blocks (c == 1) per row
  int nblk;                     // blocks of a face in the scan, dummies included
  int hs, vs;                   // luma sampling factors: 1 1 (4:4:4), 2 1 (4:2:2), 2 2 (4:2:0)
};

// The same factors where the kernels need them at compile time; SS is the `subsampling` argument: 0, 1, 2.
template <int SS>
struct Mcu {
  static constexpr int hs = SS == 0 ? 1 : 2, vs = SS == 2 ? 2 : 1;
  static constexpr int ny = hs * vs, blocks = ny + 2;
};

struct BlockPos {
  int comp, by, bx;
  bool real;
};

template <int SS>
__device__ __forceinline__ BlockPos block_pos(const Geometry& g, int b) {
  using M = Mcu<SS>;
  BlockPos p;
  if (g.c == 1) {
    p.comp = 0, p.by = b / g.mw, p.bx = b - p.by * g.mw, p.real = true;
    return p;
  }
  const int m = b / M::blocks, k = b - M::blocks * m;
  const int my = m / g.mw, mx = m - my * g.mw;
  if (k < M::ny) {
    p.comp = 0, p.by = M::vs * my + k / M::hs, p.bx = M::hs * mx + k % M::hs;
    p.real = p.by < g.ybh && p.bx < g.ybw;
  } else {
    p.comp = k - M::ny + 1, p.by = my, p.bx = mx, p.real = true;
  }
  return p;
}

// ------------------------------------------------------------------------------------------------ transform
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// One pass of the integer DCT over d[0], d[S], .. d[7 S].  The first pass leaves its output scaled up by 4.
template <int S, bool FIRST>
__device__ __forceinline__ void dct8(int* d) {
  constexpr int N = FIRST ? 11 : 15;
  const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
  const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  d[4 * S] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * 4433;
  d[2 * S] = descale(z1 + t13 * 6270, N);
  d[6 * S] = descale(z1 - t12 * 15137, N);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373, z2 *= -20995;
  z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  d[7 * S] = descale(a4 + z1 + z3, N);
  d[5 * S] = descale(a5 + z2 + z4, N);
  d[3 * S] = descale(a6 + z2 + z3, N);
  d[S] = descale(a7 + z1 + z4, N);
}

__device__ __forceinline__ int chroma_of(const uint8_t* p, int comp) {
  const int r = p[0], g = p[1], b = p[2];
  constexpr int kOffset = (128 << 16) + 32767;
  return comp == 1 ? (-11059 * r - 21709 * g + 32768 * b + kOffset) >> 16 : (32768 * r - 27439 * g - 5329 * b + kOffset) >> 16;
}

template <int SS>
__global__ void __launch_bounds__(kThreads) jpeg_transform_kernel(const uint8_t* __restrict__ crops, Geometry g, QuantArg q,
                                                                  int16_t* __restrict__ coefs) {
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= g.nblk) return;
  const BlockPos pos = block_pos<SS>(g, b);
  if (!pos.real) return;                                     // dummy blocks have no coefficients: nothing reads theirs
  const uint8_t* face = crops + (size_t)blockIdx.y * g.h * g.w * g.c;
  int d[64];
  if (pos.comp == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int y = min(pos.by * 8 + i, g.h - 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int x = min(pos.bx * 8 + j, g.w - 1);
        const uint8_t* p = face + ((size_t)y * g.w + x) * g.c;
        d[8 * i + j] = (g.c == 1 ? (int)p[0] : (19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16) - 128;
      }
    }
  } else if (SS == 0) {                                        // full resolution: the pixel's own Cb / Cr
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const size_t y = min(pos.by * 8 + i, g.h - 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const size_t x = min(pos.bx * 8 + j, g.w - 1);
        d[8 * i + j] = chroma_of(face + (y * g.w + x) * 3, pos.comp) - 128;
      }
    }
  } else if (SS == 1) {                                        // libjpeg's h2v1_downsample: pairs, bias 0 1 0 1 ..
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const size_t y = min(pos.by * 8 + i, g.h - 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int xo = pos.bx * 8 + j;
        const size_t x0 = min(2 * xo, g.w - 1), x1 = min(2 * xo + 1, g.w - 1);
        const int sum = chroma_of(face + (y * g.w + x0) * 3, pos.comp) + chroma_of(face + (y * g.w + x1) * 3, pos.comp);
        d[8 * i + j] = ((sum + (j & 1)) >> 1) - 128;
      }
    }
  } else {
    const int rows = (g.h + 1) >> 1;                         // averaged rows that exist; the ones below repeat the last
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int r = min(pos.by * 8 + i, rows - 1);
      const size_t y0 = 2 * r, y1 = min(2 * r + 1, g.h - 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int xo = pos.bx * 8 + j;
        const size_t x0 = min(2 * xo, g.w - 1), x1 = min(2 * xo + 1, g.w - 1);
        const int sum = chroma_of(face + (y0 * g.w + x0) * 3, pos.comp) + chroma_of(face + (y0 * g.w + x1) * 3, pos.comp) +
                        chroma_of(face + (y1 * g.w + x0) * 3, pos.comp) + chroma_of(face + (y1 * g.w + x1) * 3, pos.comp);
        d[8 * i + j] = ((sum + 1 + (j & 1)) >> 2) - 128;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) dct8<1, true>(d + 8 * i);
#pragma unroll
  for (int j = 0; j < 8; ++j) dct8<8, false>(d + j);

  const int tbl = pos.comp == 0 ? 0 : 1;
  uint32_t packed[32];
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const int v = d[kZigzag[k]];
    const uint32_t div = q.div[tbl][k];
    const uint32_t mag = ((uint32_t)abs(v) + (div >> 1)) / div;
    const uint32_t s = (uint32_t)(v < 0 ? -(int)mag : (int)mag) & 0xffffu;
    if (k & 1) packed[k >> 1] |= s << 16; else packed[k >> 1] = s;
  }
  uint4* dst = reinterpret_cast<uint4*>(coefs + ((size_t)blockIdx.y * g.nblk + b) * 64);
#pragma unroll
  for (int k = 0; k < 8; ++k) dst[k] = make_uint4(packed[4 * k], packed[4 * k + 1], packed[4 * k + 2], packed[4 * k + 3]);
}

// ------------------------------------------------------------------------------------------------ entropy coding
// DC of the block the difference of block b is taken against: the nearest earlier block of the component that holds samples
// (dummies repeat the DC before them), 0 at the start of the face.
template <int SS>
__device__ __forceinline__ int dc_before(const Geometry& g, const int16_t* face_coefs, int b) {
  using M = Mcu<SS>;
  if (g.c == 1) return b == 0 ? 0 : face_coefs[(size_t)(b - 1) * 64];
  const int k = b % M::blocks;
  if (k >= M::ny) return b < M::blocks ? 0 : face_coefs[(size_t)(b - M::blocks) * 64];
  // Y blocks are the first ny of every MCU: the one before the first of an MCU is three back, past Cr and Cb
  for (int p = (k == 0 ? b - 3 : b - 1); p >= 0; p = (p % M::blocks == 0 ? p - 3 : p - 1))
    if (block_pos<SS>(g, p).real) return face_coefs[(size_t)p * 64];
  return 0;
}

__device__ __forceinline__ int size_of(int v) { return 32 - __clz(abs(v)); }             // bits of |v|; 0 for 0

__device__ __forceinline__ uint32_t value_bits(int v, int s) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u); }

// Walk one block's symbols: sink.dc(set, size category, value bits) once, then sink.ac(set, run << 4 | size, value bits,
// size) for every AC symbol, ZRL and EOB among them; set = 0 for Y, 1 for chroma.  What a symbol costs or looks like is
// the sink's business: count_scan, emit and the histogram are this one walk.
template <int SS, typename Sink>
__device__ __forceinline__ void code_block(const Geometry& g, const int16_t* face_coefs, int b, Sink& sink) {
  const BlockPos pos = block_pos<SS>(g, b);
  const int set = pos.comp == 0 ? 0 : 1;
  if (!pos.real) {
    sink.dc(set, 0, 0u);
    sink.ac(set, 0, 0u, 0);
    return;
  }
  const uint4* src = reinterpret_cast<const uint4*>(face_coefs + (size_t)b * 64);
  int run = 0;
  for (int k8 = 0; k8 < 8; ++k8) {
    const uint4 v4 = src[k8];
    const uint32_t words[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int v = (int)(int16_t)(words[j >> 1] >> (16 * (j & 1)));
      if (k8 == 0 && j == 0) {
        v -= dc_before<SS>(g, face_coefs, b);
        const int s = size_of(v);
        sink.dc(set, s, value_bits(v, s));
        continue;
      }
      if (v == 0) {
        ++run;
        continue;
      }
      while (run > 15) {
        sink.ac(set, 0xF0, 0u, 0);
        run -= 16;
      }
      const int s = size_of(v);
      sink.ac(set, (run << 4) | s, value_bits(v, s), s);
      run = 0;
    }
  }
  if (run > 0) sink.ac(set, 0, 0u, 0);
}

// The code tables of a workgroup, in LDS: code | length << 16 by DC size category and by AC symbol, per set.
struct CodeTables {
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};

struct CountSink {
  const CodeTables* t;
  uint32_t bits = 0;
  __device__ __forceinline__ void dc(int set, int s, uint32_t) { bits += (t->dc[set][s] >> 16) + s; }
  __device__ __forceinline__ void ac(int set, int sym, uint32_t, int s) { bits += (t->ac[set][sym] >> 16) + s; }
};

// One count per symbol into the wave's own histogram in LDS.  The transform's coefficients give size categories of 11
// at most; the indices are clamped all the same, so that no 16-bit value at all could leave the arrays.
struct HistSink {
  uint32_t* dc_bins;            // [2][16]
  uint32_t* ac_bins;            // [2][256]
  __device__ __forceinline__ void dc(int set, int s, uint32_t) { atomicAdd(dc_bins + set * 16 + min(s, 15), 1u); }
  __device__ __forceinline__ void ac(int set, int sym, uint32_t, int) { atomicAdd(ac_bins + set * 256 + (sym & 255), 1u); }
};

// Bits go out most significant first; put() takes up to 27 bits (a 16-bit DC code of an optimised table and 11 value bits).
struct EmitSink : fcp_entropy::BitWriter<true> {
  const CodeTables* t;
  __device__ __forceinline__ void dc(int set, int s, uint32_t bits) {
    const uint32_t e = t->dc[set][s];
    put(((e & 0xffffu) << s) | bits, (e >> 16) + s);
  }
  __device__ __forceinline__ void ac(int set, int sym, uint32_t bits, int s) {
    const uint32_t e = t->ac[set][sym];
    put(((e & 0xffffu) << s) | bits, (e >> 16) + s);
  }
};

// The standard tables from the kernel-argument block, or (face_codes != nullptr) the face's own four 256-entry tables the
// table kernel left in the workspace, in record order: Y DC, Y AC, chroma DC, chroma AC.  2144 bytes of LDS either way.
__device__ __forceinline__ void load_tables(const HuffArg& hf, const uint32_t* face_codes, CodeTables* t) {
  uint32_t* dc_tab = &t->dc[0][0];
  uint32_t* ac_tab = &t->ac[0][0];
  if (face_codes == nullptr) {
    const uint32_t* dc = &hf.dc[0][0];
    const uint32_t* ac = &hf.ac[0][0];
    for (int i = threadIdx.x; i < 24; i += kThreads) dc_tab[i] = dc[i];
    for (int i = threadIdx.x; i < 512; i += kThreads) ac_tab[i] = ac[i];
  } else {
    for (int i = threadIdx.x; i < 24; i += kThreads) dc_tab[i] = face_codes[(i / 12) * 512 + i % 12];
    for (int i = threadIdx.x; i < 512; i += kThreads) ac_tab[i] = face_codes[(i >> 8) * 512 + 256 + (i & 255)];
  }
  __syncthreads();
}

template <int SS>
__global__ void __launch_bounds__(kThreads) jpeg_count_scan_kernel(const int16_t* __restrict__ coefs, Geometry g, HuffArg hf,
                                                                   const uint32_t* __restrict__ codes,
                                                                   uint32_t* __restrict__ bitoff) {
  __shared__ CodeTables tabs;
  __shared__ uint32_t wave_sums[kThreads / 64];
  load_tables(hf, codes ? codes + (size_t)blockIdx.x * 1024 : nullptr, &tabs);
  const int16_t* face_coefs = coefs + (size_t)blockIdx.x * g.nblk * 64;
  uint32_t* off = bitoff + (size_t)blockIdx.x * (g.nblk + 1);
  uint32_t carry = 0;
  for (int base = 0; base < g.nblk; base += kThreads) {        // uniform trip count: every lane reaches the barriers
    const int b = base + threadIdx.x;
    CountSink sink;
    sink.t = &tabs;
    if (b < g.nblk) code_block<SS>(g, face_coefs, b, sink);
    uint32_t total;
    const uint32_t excl = fcp_block_exclusive_scan<kThreads>(sink.bits, wave_sums, &total);
    if (b < g.nblk) off[b] = carry + excl;
    carry += total;
  }
  if (threadIdx.x == 0) off[g.nblk] = carry;
}

template <int SS>
__global__ void __launch_bounds__(kThreads) jpeg_emit_kernel(const int16_t* __restrict__ coefs, Geometry g, HuffArg hf,
                                                             const uint32_t* __restrict__ codes,
                                                             const uint32_t* __restrict__ bitoff, uint32_t* __restrict__ raw,
                                                             size_t raw_words) {
  __shared__ CodeTables tabs;
  load_tables(hf, codes ? codes + (size_t)blockIdx.y * 1024 : nullptr, &tabs);
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b >= g.nblk) return;
  const int16_t* face_coefs = coefs + (size_t)blockIdx.y * g.nblk * 64;
  const uint32_t* off = bitoff + (size_t)blockIdx.y * (g.nblk + 1);
  const uint32_t start = off[b];
  EmitSink sink;
  sink.t = &tabs;
  sink.word = raw + (size_t)blockIdx.y * raw_words + (start >> 5);
  sink.n = start & 31u;
  sink.shared = sink.n != 0;
  code_block<SS>(g, face_coefs, b, sink);
  if (b == g.nblk - 1) {                                       // fill the last byte with 1-bits
    const uint32_t pad = (8u - (off[g.nblk] & 7u)) & 7u;
    if (pad) sink.put((1u << pad) - 1u, pad);
  }
  sink.finish();
}

// ------------------------------------------------------------------------------------------------ optimised tables
constexpr int kHistBins = 2 * 16 + 2 * 256;   // a wave's histogram: DC size categories and AC symbols of both sets

// hist (f, 4, 256), zeroed by the caller's memset: += the symbol counts of this workgroup's blocks.  Dummy blocks count
// their DC 0 and their EOB, like libjpeg's statistics pass.
template <int SS>
__global__ void __launch_bounds__(kThreads) jpeg_histogram_kernel(const int16_t* __restrict__ coefs, Geometry g,
                                                                  uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[kThreads / 64][kHistBins];
  for (int i = threadIdx.x; i < (kThreads / 64) * kHistBins; i += kThreads) (&bins[0][0])[i] = 0;
  __syncthreads();
  const int b = blockIdx.x * kThreads + threadIdx.x;
  if (b < g.nblk) {
    HistSink sink;
    sink.dc_bins = bins[threadIdx.x >> 6];
    sink.ac_bins = bins[threadIdx.x >> 6] + 32;
    code_block<SS>(g, coefs + (size_t)blockIdx.y * g.nblk * 64, b, sink);
  }
  __syncthreads();
  uint32_t* dst = hist + (size_t)blockIdx.y * 1024;
  for (int i = threadIdx.x; i < kHistBins; i += kThreads) {
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) n += bins[k][i];
    if (n == 0) continue;
    const int col = i < 32 ? (i >> 4) * 512 + (i & 15) : ((i - 32) >> 8) * 512 + 256 + ((i - 32) & 255);
    atomicAdd(dst + col, n);
  }
}

// libjpeg's jpeg_gen_optimal_table, one wave per table, out of the pieces of fcp_entropy.h.  Entry 256 of the merge is
// the pseudo-symbol of frequency 1, which keeps the all-ones code free.
// Preconditions (a row sums to less than Fibonacci(35) - 1, so no code is longer than 32 bits) are the caller's; if they
// do not hold the tables are meaningless but every index below is clamped into its array.
__global__ void __launch_bounds__(64) jpeg_tables_kernel(const uint32_t* __restrict__ freq, uint8_t* __restrict__ tables,
                                                         uint32_t* __restrict__ codes) {
  __shared__ int bits[kMaxCodeLength + 1];
  __shared__ uint8_t size_by_symbol[256];
  __shared__ uint8_t record[kTableBytes];
  __shared__ int first_pos[18];
  __shared__ uint32_t first_code[17];
  const int lane = threadIdx.x;
  const size_t t = blockIdx.x;
  uint32_t fr[5];
  int cs[5];
#pragma unroll
  for (int j = 0; j < 4; ++j) fr[j] = freq[t * 256 + lane + 64 * j];
  fr[4] = lane == 0 ? 1u : 0u;
  for (int i = lane; i < kTableBytes; i += 64) record[i] = 0;
  if (lane <= kMaxCodeLength) bits[lane] = 0;
  if (__ballot((fr[0] | fr[1] | fr[2] | fr[3]) != 0u) == 0ull) {          // nothing to code: an all-zero record
    for (int i = lane; i < kTableBytes; i += 64) tables[t * kTableBytes + i] = 0;
    if (codes)
      for (int i = lane; i < 256; i += 64) codes[t * 256 + i] = 0u;
    return;
  }
  fcp_entropy::huffman_code_sizes(fr, 257, cs);
#pragma unroll
  for (int j = 0; j < 5; ++j) cs[j] = min(cs[j], kMaxCodeLength);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 5; ++j)
    if (cs[j] > 0 && (j < 4 || lane == 0)) atomicAdd(&bits[cs[j]], 1);
#pragma unroll
  for (int j = 0; j < 4; ++j) size_by_symbol[lane + 64 * j] = (uint8_t)cs[j];
  __syncthreads();
  if (lane == 0) {
    fcp_entropy::limit_code_lengths<kMaxCodeLength, 16>(bits);
    int i = 16;
    while (i > 0 && bits[i] == 0) --i;
    if (i > 0) --bits[i];                                                 // the pseudo-symbol's code is not a symbol's
    fcp_entropy::code_starts<16>(bits, 255, first_pos, first_code);
    for (int len = 1; len <= 16; ++len) record[len - 1] = (uint8_t)(first_pos[len + 1] - first_pos[len]);
  }
  __syncthreads();
  // symbols in code order: by code size before the limit, then by value; the limited lengths go to them in that order
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int sym = lane + 64 * j;
    uint32_t entry = 0u;
    if (cs[j] > 0) {
      const int p = fcp_entropy::symbol_rank(size_by_symbol, 256, cs[j], sym);
      record[16 + p] = (uint8_t)sym;                                      // p < 256: at most 255 symbols come before one
      const int len = fcp_entropy::length_at_rank<16>(first_pos, p);
      if (len > 0) entry = ((first_code[len] + (uint32_t)(p - first_pos[len])) & 0xffffu) | ((uint32_t)len << 16);
    }
    if (codes) codes[t * 256 + sym] = entry;
  }
  __syncthreads();
  for (int i = lane; i < kTableBytes; i += 64) tables[t * kTableBytes + i] = record[i];
}

// ------------------------------------------------------------------------------------------------ byte stuffing
__global__ void __launch_bounds__(kThreads) jpeg_stuff_kernel(const uint32_t* __restrict__ raw, size_t raw_words, int nblk,
                                                              const uint32_t* __restrict__ bitoff, uint8_t* __restrict__ out,
                                                              long long out_stride, long long capacity,
                                                              int32_t* __restrict__ lengths) {
  __shared__ uint32_t wave_sums[kThreads / 64];
  const uint32_t nbytes = (bitoff[(size_t)blockIdx.x * (nblk + 1) + nblk] + 7u) >> 3;
  const uint4* src = reinterpret_cast<const uint4*>(raw + (size_t)blockIdx.x * raw_words);
  uint8_t* dst = out + (size_t)blockIdx.x * out_stride;
  long long carry = 0;                                         // stuffed zeros before this round
  for (uint32_t base = 0; base < nbytes; base += 16 * kThreads) {
    const uint32_t first = base + 16 * threadIdx.x;            // this lane's 16 bytes: four big-endian words
    uint32_t words[4] = {0, 0, 0, 0};
    if (first < nbytes) {
      const uint4 v = src[first >> 4];
      words[0] = v.x, words[1] = v.y, words[2] = v.z, words[3] = v.w;
    }
    uint32_t ffs = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      ffs += (first + j < nbytes && ((words[j >> 2] >> (24 - 8 * (j & 3))) & 255u) == 255u) ? 1u : 0u;
    uint32_t total;
    const uint32_t excl = fcp_block_exclusive_scan<kThreads>(ffs, wave_sums, &total);
    long long p = (long long)first + carry + excl;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (first + j < nbytes) {
        const uint32_t byte = (words[j >> 2] >> (24 - 8 * (j & 3))) & 255u;
        if (p < capacity) dst[p] = (uint8_t)byte;
        ++p;
        if (byte == 255u) {
          if (p < capacity) dst[p] = 0;
          ++p;
        }
      }
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    const long long end = (long long)nbytes + carry;
    if (end < capacity) dst[end] = 0xFF;
    if (end + 1 < capacity) dst[end + 1] = 0xD9;
    lengths[blockIdx.x] = (int32_t)(end + 2);
  }
}

// ------------------------------------------------------------------------------------------------ host side
struct Layout {
  Geometry g;
  size_t raw_words;             // per face, a multiple of 4: the stuffing pass reads 16 bytes at a time
  size_t coef_bytes, off_bytes, raw_bytes;
  size_t hist_bytes, code_bytes;   // optimised tables only: (f, 4, 256) counts behind the raw bits, then as many codes
  size_t total() const { return coef_bytes + off_bytes + raw_bytes + hist_bytes + code_bytes; }
};

int blocks_of(int h, int w, int c, int ss) {
  if (c == 1) return ((w + 7) / 8) * ((h + 7) / 8);
  const int hs = ss == 0 ? 1 : 2, vs = ss == 2 ? 2 : 1;
  return (hs * vs + 2) * ((w + 8 * hs - 1) / (8 * hs)) * ((h + 8 * vs - 1) / (8 * vs));
}

Layout layout_of(int f, int h, int w, int c, int ss, int optimize) {
  Layout l;
  Geometry& g = l.g;
  g.h = h, g.w = w, g.c = c;
  g.ybw = (w + 7) / 8, g.ybh = (h + 7) / 8;
  g.hs = ss == 0 ? 1 : 2, g.vs = ss == 2 ? 2 : 1;
  g.mw = c == 1 ? g.ybw : (w + 8 * g.hs - 1) / (8 * g.hs);
  g.nblk = blocks_of(h, w, c, ss);
  const int block_bits = optimize ? kMaxBlockBitsOpt : kMaxBlockBits;
  l.raw_words = (((size_t)g.nblk * block_bits + 7 + 31) / 32 + 3) & ~(size_t)3;
  l.coef_bytes = round16((size_t)f * g.nblk * 64 * sizeof(int16_t));
  l.off_bytes = round16((size_t)f * (g.nblk + 1) * sizeof(uint32_t));
  l.raw_bytes = (size_t)f * l.raw_words * sizeof(uint32_t);
  l.hist_bytes = l.code_bytes = optimize ? (size_t)f * 4 * 256 * sizeof(uint32_t) : 0;
  return l;
}

void huffman_codes(const uint8_t* counts, const uint8_t* symbols, uint32_t* by_symbol) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < counts[len - 1]; ++i) by_symbol[symbols[k++]] = code++ | ((uint32_t)len << 16);
    code <<= 1;
  }
}

int check_sizes(int f, int h, int w, int channels) {
  FCP_REQUIRE(f >= 0 && h >= 1 && w >= 1, "jpeg_encode: bad sizes (f %d, h %d, w %d)", f, h, w);
  FCP_REQUIRE(channels == 1 || channels == 3, "jpeg_encode: 1 (gray) or 3 (RGB) channels, not %d", channels);
  FCP_REQUIRE(h <= kMaxSide && w <= kMaxSide, "jpeg_encode: crops of at most %d x %d px (got h %d, w %d)", kMaxSide, kMaxSide,
              h, w);
  FCP_REQUIRE(f <= 65535, "jpeg_encode: at most 65535 crops per call");
  return 0;
}

// What the extended entry points check on top: the two settings, and the two limits a face's block count has.
int check_options(int h, int w, int channels, int subsampling, int optimize) {
  FCP_REQUIRE(subsampling >= 0 && subsampling <= 2, "jpeg_encode: subsampling 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), not %d",
              subsampling);
  FCP_REQUIRE(optimize == 0 || optimize == 1, "jpeg_encode: optimize 0 or 1, not %d", optimize);
  const long long nblk = blocks_of(h, w, channels, subsampling);
  FCP_REQUIRE(nblk * (optimize ? kMaxBlockBitsOpt : kMaxBlockBits) <= 0xffffffffll,
              "jpeg_encode: a face of %lld blocks is too large for 32-bit bit offsets (h %d, w %d)", nblk, h, w);
  FCP_REQUIRE(!optimize || 64 * nblk + 1 < kFib35,
              "jpeg_encode: optimised tables need fewer than %lld coefficients per face, a face of %lld blocks has %lld "
              "(a deeper Huffman tree than libjpeg's 32 levels would be possible)", kFib35 - 1, nblk, 64 * nblk);
  return 0;
}

template <int SS>
void launch_encode(const uint8_t* crops, int f, const Layout& l, const QuantArg& q, const HuffArg& hf, int optimize,
                   uint8_t* out, int64_t out_stride, int64_t capacity, int32_t* lengths, uint8_t* tables, int16_t* coefs,
                   uint32_t* bitoff, uint32_t* raw, uint32_t* hist, uint32_t* codes, hipStream_t s) {
  const dim3 per_block(fcp_cdiv(l.g.nblk, kThreads), f);
  hipLaunchKernelGGL(jpeg_transform_kernel<SS>, per_block, dim3(kThreads), 0, s, crops, l.g, q, coefs);
  if (optimize) {
    hipLaunchKernelGGL(jpeg_histogram_kernel<SS>, per_block, dim3(kThreads), 0, s, coefs, l.g, hist);
    hipLaunchKernelGGL(jpeg_tables_kernel, dim3(4 * f), dim3(64), 0, s, hist, tables, codes);
  }
  hipLaunchKernelGGL(jpeg_count_scan_kernel<SS>, dim3(f), dim3(kThreads), 0, s, coefs, l.g, hf, optimize ? codes : nullptr,
                     bitoff);
  hipLaunchKernelGGL(jpeg_emit_kernel<SS>, per_block, dim3(kThreads), 0, s, coefs, l.g, hf, optimize ? codes : nullptr, bitoff,
                     raw, l.raw_words);
  hipLaunchKernelGGL(jpeg_stuff_kernel, dim3(f), dim3(kThreads), 0, s, raw, l.raw_words, l.g.nblk, bitoff, out,
                     (long long)out_stride, (long long)capacity, lengths);
}

// Everything behind both entry points; the caller has checked sizes, subsampling and optimize.
int encode(const uint8_t* crops, int f, int h, int w, int channels, int quality, int subsampling, int optimize, uint8_t* out,
           int64_t out_stride, int64_t capacity, int32_t* lengths, uint8_t* tables, void* workspace, int64_t workspace_bytes,
           const char* sizer, fcp_stream_t stream) {
  FCP_REQUIRE(quality >= 1 && quality <= 100, "jpeg_encode: quality 1..100, not %d", quality);
  const Layout l = layout_of(f, h, w, channels, subsampling, optimize);
  if (int rc = fcp_entropy::check_slots("jpeg_encode", f, crops && lengths && workspace && (out || capacity == 0), out_stride,
                                        capacity, workspace, workspace_bytes, l.total(), sizer))
    return rc;
  if (f == 0) return 0;
  FCP_REQUIRE(!optimize || tables, "jpeg_encode: optimize needs the tables buffer (null pointer)");

  QuantArg q;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;          // the IJG quality scale, baseline range
  for (int t = 0; t < 2; ++t)
    for (int k = 0; k < 64; ++k) {
      int v = (kQuantBase[t][kZigzag[k]] * scale + 50) / 100;
      v = v < 1 ? 1 : (v > 255 ? 255 : v);
      q.div[t][k] = (uint16_t)(8 * v);
    }
  HuffArg hf = {};
  static const uint8_t dc_symbols[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
  for (int t = 0; t < 2; ++t) {
    huffman_codes(kDcCounts[t], dc_symbols, hf.dc[t]);
    huffman_codes(kAcCounts[t], kAcSymbols[t], hf.ac[t]);
  }

  uint8_t* ws = static_cast<uint8_t*>(workspace);
  int16_t* coefs = reinterpret_cast<int16_t*>(ws);
  uint32_t* bitoff = reinterpret_cast<uint32_t*>(ws + l.coef_bytes);
  uint32_t* raw = reinterpret_cast<uint32_t*>(ws + l.coef_bytes + l.off_bytes);
  uint32_t* hist = reinterpret_cast<uint32_t*>(ws + l.coef_bytes + l.off_bytes + l.raw_bytes);
  uint32_t* codes = reinterpret_cast<uint32_t*>(ws + l.coef_bytes + l.off_bytes + l.raw_bytes + l.hist_bytes);
  hipStream_t s = (hipStream_t)stream;
  FCP_HIP_OK(hipMemsetAsync(raw, 0, l.raw_bytes + l.hist_bytes, s));            // the counts sit right behind the bits
  switch (channels == 1 ? 2 : subsampling) {                                    // gray has no MCUs: any instance does
    case 0:
      launch_encode<0>(crops, f, l, q, hf, optimize, out, out_stride, capacity, lengths, tables, coefs, bitoff, raw, hist, codes, s);
      break;
    case 1:
      launch_encode<1>(crops, f, l, q, hf, optimize, out, out_stride, capacity, lengths, tables, coefs, bitoff, raw, hist, codes, s);
      break;
    default:
      launch_encode<2>(crops, f, l, q, hf, optimize, out, out_stride, capacity, lengths, tables, coefs, bitoff, raw, hist, codes, s);
  }
  FCP_LAUNCH_OK();
  return 0;
}

}  // namespace

extern "C" int64_t fcp_jpeg_workspace_bytes(int f, int h, int w, int channels) {
  if (check_sizes(f, h, w, channels) != 0) return -1;
  return (int64_t)layout_of(f, h, w, channels, 2, 0).total();
}

extern "C" int64_t fcp_jpeg_workspace_bytes_ex(int f, int h, int w, int channels, int subsampling, int optimize) {
  if (check_sizes(f, h, w, channels) != 0 || check_options(h, w, channels, subsampling, optimize) != 0) return -1;
  return (int64_t)layout_of(f, h, w, channels, subsampling, optimize).total();
}

extern "C" int fcp_jpeg_encode_u8(const uint8_t* crops, int f, int h, int w, int channels, int quality, int subsampling,
                                  uint8_t* out, int64_t out_stride, int64_t capacity, int32_t* lengths, void* workspace,
                                  int64_t workspace_bytes, fcp_stream_t stream) {
  if (check_sizes(f, h, w, channels) != 0) return FCP_ERR_ARG;
  FCP_REQUIRE(quality >= 1 && quality <= 100, "jpeg_encode: quality 1..100, not %d", quality);
  FCP_REQUIRE(subsampling == 2, "jpeg_encode: only 4:2:0 chroma subsampling (2) is built, not %d", subsampling);
  return encode(crops, f, h, w, channels, quality, 2, 0, out, out_stride, capacity, lengths, nullptr, workspace, workspace_bytes,
                "fcp_jpeg_workspace_bytes", stream);
}

extern "C" int fcp_jpeg_encode_ex_u8(const uint8_t* crops, int f, int h, int w, int channels, int quality, int subsampling,
                                     int optimize, uint8_t* out, int64_t out_stride, int64_t capacity, int32_t* lengths,
                                     uint8_t* tables, void* workspace, int64_t workspace_bytes, fcp_stream_t stream) {
  if (check_sizes(f, h, w, channels) != 0) return FCP_ERR_ARG;
  FCP_REQUIRE(quality >= 1 && quality <= 100, "jpeg_encode: quality 1..100, not %d", quality);
  if (check_options(h, w, channels, subsampling, optimize) != 0) return FCP_ERR_ARG;
  return encode(crops, f, h, w, channels, quality, subsampling, optimize, out, out_stride, capacity, lengths, tables, workspace,
                workspace_bytes, "fcp_jpeg_workspace_bytes_ex", stream);
}

extern "C" int fcp_jpeg_huffman_tables(const uint32_t* freq, int n, uint8_t* tables, uint32_t* codes, fcp_stream_t stream) {
  FCP_REQUIRE(n >= 0 && n <= 4 * 65535, "jpeg_huffman_tables: 0..%d rows, not %d", 4 * 65535, n);
  if (n == 0) return 0;
  FCP_REQUIRE(freq && tables, "jpeg_huffman_tables: null pointer");
  FCP_REQUIRE((reinterpret_cast<uintptr_t>(freq) & 3) == 0 && (reinterpret_cast<uintptr_t>(codes) & 3) == 0,
              "jpeg_huffman_tables: freq and codes must be 4-byte aligned");
  hipLaunchKernelGGL(jpeg_tables_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, freq, tables, codes);
  FCP_LAUNCH_OK();
  return 0;
}
