// Shared pieces of the convolution kernels (fp32-exact and fp16x3-split variants):
// kernel parameter block, the im2col walk and the fused epilogue.
#pragma once
#include <type_traits>
#include "fcp_common.h"
#include "fcp_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));


// Cache policy of the LDS-DMA operand loads (the `aux` immediate of raw.ptr.buffer.load.lds on gfx950: 1 = sc0, 2 = nt,
// 16 = sc1), activations (A) and filters (B): default policy for both — nt / sc1 on either operand measured equal or slower
// (profiles/r03_probes.md section 1).
constexpr int FCP_AUX_A = 0;
constexpr int FCP_AUX_B = 0;

namespace fcp_conv {

constexpr int BM = 128;   // output pixels per workgroup tile
constexpr int BK = 32;    // K slice: one filter tap x 32 input channels

struct ConvK {
  const float* in;
  const float* w;
  const float* bias;
  float* out;
  const float* res1;
  const float* res2;
  int n, in_h, in_w, ph, pw, cin, in_ld, in_up2;   // (cin: no kernel reads it; without it the kernarg layout shifts and two halo kernels spill more SGPRs: profiles/conv_epilogue.md)
  int cout, kh, kw, stride, pad, out_h, out_w, out_ld;
  int pad_h;      // rows of zero padding above input row 0 (= pad - band_top: fcp_conv_desc.band_top / band_bottom)
  int M, ktiles, ctiles, wrow;
  float act_slope, alpha, alpha2;
  int res1_pre, res1_ld, res1_h, res1_w, res1_resize, res2_ld;
  float res1_sh, res1_sw;
  int grid_m, grid_n, vec_ok;
  unsigned in_bytes, w_bytes;
  const float* wscale;  // per-cout power-of-two filter scale (fp16x3 path) or nullptr
  int in_fmt, out_fmt, res1_fmt, res2_fmt;   // 0 = fp32 NHWC, 1 = split32 (see fcp_hip.h)
  // second source of a 1x1 conv (channels >= csplit), LDS-DMA kernels only; in2 == nullptr: off
  const float* in2;
  unsigned in2_bytes;
  int csplit, in2_ld, ph2, pw2, stride2;
  int nt_store;   // 1: split32 outputs are written with non-temporal (streaming) stores
  // 256-row kernel only: M-tile schedule (see conv_igemm_f16x3_big).  `balance` / `cu_budget` come from the descriptor,
  // the launcher derives the rest.
  int balance, cu_budget;
  int mfull, tail_rows, round_size;
  int big_tiles;        // 256-row kernel (persistent): tiles of the launch = virtual block ids 0 .. big_tiles - 1
  int big_persist;      // 1: round_size workgroups walk the tiles; 0: one workgroup per tile
};


// K order: slice kt = (channel slice kt / taps, tap kt % taps): the kh*kw taps of one 32-channel
// slice are consecutive, so a 3x3 conv touches only 32 channels of its pixel neighbourhood for 9
// slices in a row — the per-XCD working set stays L2 resident instead of being re-fetched per tap.
//
// Operand addressing per 16-byte piece: `base` = byte offset of the piece at tap (0,0), channel 0
// (wrapping unsigned arithmetic; only used when valid) and `mask` bit t = tap t reads a real pixel
// (not the zero padding).  Per slice the offset is base + tap_off(uniform) + c0*4, or 0xFFFFFFFF.
struct TapPiece {
  unsigned base, mask;
};

template <bool CIN4>
__device__ __forceinline__ TapPiece make_tap_piece(const ConvK& p, unsigned pbase, int hi0, int wi0, unsigned chan_off) {
  TapPiece t;
  t.base = ((pbase + (unsigned)(hi0 * p.pw + wi0)) * (unsigned)p.in_ld + chan_off) * 4u;
  t.mask = 0u;
  const int taps = CIN4 ? p.kh : p.kh * p.kw;
  for (int q = 0; q < taps; ++q) {
    const int kh_i = CIN4 ? q : q / p.kw;
    const int kw_i = CIN4 ? 0 : q - kh_i * p.kw;
    const bool ok = (unsigned)(hi0 + kh_i) < (unsigned)p.in_h && (unsigned)(wi0 + kw_i) < (unsigned)p.in_w;
    t.mask |= ok ? (1u << q) : 0u;
  }
  return t;
}

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------------------------------
// The im2col walk of the generic implicit-GEMM kernels (conv_igemm_f32, _f16x3, _f16x3_dma, _f16x3_big), stated once: which
// tile a workgroup owns, where an output row's window starts, which tap and channel slice a K slice is, and the operand
// offset of a 16-byte piece at that tap.  How a slice reaches LDS, the pipeline and the MFMAs are the kernels' own.
// ---------------------------------------------------------------------------------------------------------------------

// XCD-aware tile order: hardware round-robins consecutive workgroup ids over the 8 XCDs; give each XCD a contiguous run of
// logical tiles so the N-tiles of one pixel block and neighbouring pixel blocks (3x3 halos) share an L2.
// bid of nb workgroups -> logical tile.
__device__ __forceinline__ int xcd_tile_order(int nb, int bid) {
  const int q8 = nb >> 3, r8 = nb & 7, xcd = bid & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
}

// Output pixel m -> (image, row, column); hw = out_h * out_w.  (M: int in the walk, long in the epilogue's res1_pixel.)
template <typename M>
__device__ __forceinline__ void conv_out_pixel(const ConvK& p, M m, int hw, int& ni, int& ho, int& wo) {
  ni = (int)(m / hw);
  const int rem = (int)(m - (M)ni * hw);
  ho = rem / p.out_w;
  wo = rem - ho * p.out_w;
}

// One output row (GEMM row m) of a tile whose rows end at m_end, decoded once.
struct ConvRow {
  int ni;           // image of the row: the fp32 kernel's flat path forms its 64-bit pixel index from it
  unsigned pbase;   // first pixel of that image (32-bit: the buffer paths)
  int hi0, wi0;     // input coordinates of tap (0, 0); a row at or past m_end has hi0 = -(1 << 28): every tap is padding
  unsigned base2;   // second source (p.in2 set): byte offset of the row's pixel there + chan_off2 floats, else 0xFFFFFFFF
};
__device__ __forceinline__ ConvRow conv_row(const ConvK& p, int m, int m_end, int hw, unsigned chan_off2) {
  ConvRow r = {0, 0u, -(1 << 28), 0, 0xFFFFFFFFu};
  if (m < m_end) {
    int ho, wo;
    conv_out_pixel(p, m, hw, r.ni, ho, wo);
    r.pbase = (unsigned)(r.ni * p.ph * p.pw);
    r.hi0 = ho * p.stride - p.pad_h;
    r.wi0 = wo * p.stride - p.pad;
    if (p.in2 != nullptr)
      r.base2 = (((unsigned)(r.ni * p.ph2 + ho * p.stride2) * (unsigned)p.pw2 + (unsigned)(wo * p.stride2)) * (unsigned)p.in2_ld + chan_off2) * 4u;
  }
  return r;
}

// One 16-byte operand piece of a row: channels chan_off .. + 3 of the tap's pixel, or (CIN4: 3 channels in an NHWC4 buffer,
// a K slice = one filter row of 8 pixels) pixel `col` of the tap row.  A kernel holds as many per row as its staging needs.
struct RowPiece {
  unsigned pbase;
  int hi0, wi0;       // the row's
  int col;            // CIN4: the piece's pixel in the tap row, else 0
  unsigned chan_off;  // 0 under CIN4
  TapPiece tp;
};
template <bool CIN4>
__device__ __forceinline__ RowPiece make_row_piece(const ConvK& p, const ConvRow& r, int col, unsigned chan_off) {
  RowPiece c = {r.pbase, r.hi0, r.wi0, CIN4 ? col : 0, CIN4 ? 0u : chan_off, {0u, 0u}};
  c.tp = make_tap_piece<CIN4>(p, c.pbase, c.hi0, c.wi0 + c.col, c.chan_off);
  return c;
}

// The K slice a kernel is at: taps fastest, then the 32-channel slice (the K order above).
struct TapWalk {
  int tap = 0, kh_i = 0, kw_i = 0, c0 = 0;
  template <bool CIN4>
  __device__ __forceinline__ void advance(const ConvK& p) {
    ++tap;
    if (CIN4) {
      ++kh_i;
    } else if (++kw_i >= p.kw) {
      kw_i = 0;
      if (++kh_i >= p.kh) { kh_i = 0; tap = 0; c0 += BK; }
    }
  }
};

// rowoff[i] = byte offset of piece i at channel 0 of the walk's tap, 0xFFFFFFFF = zero padding.  UP2: the kernel has the
// nearest-x2 operand fetch (p.in_up2), whose physical offset is not linear in the tap and is recomputed per tap.
template <bool CIN4, bool UP2, int NP>
__device__ __forceinline__ void set_tap(const ConvK& p, const TapWalk& t, const RowPiece (&pc)[NP], unsigned (&rowoff)[NP]) {
  if (UP2 && p.in_up2) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      int hi = pc[i].hi0 + t.kh_i;
      int wi = pc[i].wi0 + (CIN4 ? pc[i].col : t.kw_i);
      const bool ok = (unsigned)hi < (unsigned)p.in_h && (unsigned)wi < (unsigned)p.in_w;
      hi >>= 1; wi >>= 1;
      const unsigned pix = pc[i].pbase + (unsigned)(hi * p.pw + wi);
      rowoff[i] = ok ? (pix * (unsigned)p.in_ld + pc[i].chan_off) * 4u : 0xFFFFFFFFu;
    }
  } else {
    const unsigned tapoff = (unsigned)((t.kh_i * p.pw + t.kw_i) * p.in_ld) * 4u;   // wave-uniform
#pragma unroll
    for (int i = 0; i < NP; ++i) rowoff[i] = ((pc[i].tp.mask >> t.tap) & 1u) ? pc[i].tp.base + tapoff : 0xFFFFFFFFu;
  }
}
template <bool CIN4, bool UP2, int NP>
__device__ __forceinline__ void next_tap(const ConvK& p, TapWalk& t, const RowPiece (&pc)[NP], unsigned (&rowoff)[NP]) {
  t.advance<CIN4>(p);
  set_tap<CIN4, UP2>(p, t, pc, rowoff);
}

__device__ __forceinline__ f32x4 buf_load16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, 0, 0));
}
__device__ __forceinline__ u32x4_t buf_load16u(__amdgpu_buffer_rsrc_t rsrc, unsigned voff) {
  return __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, 0, 0));
}

// One K slice of the LDS-DMA kernels: A_LD + B_LD DMA instructions per wave, each 64 lanes x 16 B = LDS rows
// 8 * wave + STEP * i .. + 7 of the pixel tile at `a` and of the filter tile at `b` (STEP = rows one instruction set covers:
// a quarter of the threads' count).  Channels >= csplit come from the second source (wave-uniform choice).
template <int STEP, int A_LD, int B_LD>
__device__ __forceinline__ void dma_slice(const ConvK& p, __amdgpu_buffer_rsrc_t rs_in, __amdgpu_buffer_rsrc_t rs_in2, __amdgpu_buffer_rsrc_t rs_w,
                                          char* a, char* b, const unsigned (&rowoff)[A_LD], const unsigned (&base2)[A_LD],
                                          const unsigned (&woff)[B_LD], int c0, int kt) {
  constexpr int ROWB = 128;
  if (c0 >= p.csplit) {
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
      const unsigned ro = base2[i];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in2, (__attribute__((address_space(3))) void*)(a + STEP * i * ROWB), 16,
                                               (int)(ro == 0xFFFFFFFFu ? 0xFFFFFFFFu : ro + (unsigned)((c0 - p.csplit) * 4)), 0, 0, FCP_AUX_A);
    }
  } else {
#pragma unroll
    for (int i = 0; i < A_LD; ++i) {
      const unsigned ro = rowoff[i];
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (__attribute__((address_space(3))) void*)(a + STEP * i * ROWB), 16,
                                               (int)(ro == 0xFFFFFFFFu ? 0xFFFFFFFFu : ro + (unsigned)(c0 * 4)), 0, 0, FCP_AUX_A);
    }
  }
#pragma unroll
  for (int i = 0; i < B_LD; ++i)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (__attribute__((address_space(3))) void*)(b + STEP * i * ROWB), 16,
                                             (int)(woff[i] + (unsigned)(kt * BK * 4)), 0, 0, FCP_AUX_B);
}

// Chunk swizzle of a 128-byte fp16x3 LDS row: 16-byte chunk c of row `row` lives at chunk position c ^ swz(row).
__device__ __forceinline__ int swz(int row) { return ((row >> 1) & 7) ^ ((row & 1) << 2); }

// Fragment offsets inside a swizzled 128-byte fp16x3 LDS row [hi k0..31 | lo k0..31] (chunk swizzle ((row >> 1) & 7) ^
// ((row & 1) << 2), row = lane & 31): the hi / lo chunk of k-half s that lane `lane` feeds to v_mfma_f32_32x32x16_f16.
__device__ __forceinline__ void frag_offsets(int lane, int (&offH)[2], int (&offL)[2]) {
  const int rsw = (((lane & 31) >> 1) & 7) ^ ((lane & 1) << 2);
  const int half = lane >> 5;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    offH[s] = ((2 * s + half) ^ rsw) << 4;
    offL[s] = ((4 + 2 * s + half) ^ rsw) << 4;
  }
}

// ds_read_b128 with an immediate offset, as inline asm: the compiler's waitcnt pass would otherwise drain the pending LDS-DMA
// (vmcnt(0)) in front of every LDS read.
template <int IMM>
__device__ __forceinline__ f16x8 lds_read128i(unsigned addr) {
  f16x8 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(IMM));
  return v;
}

template <int TM, int TN>
__device__ __forceinline__ void clear_acc(f32x16 (&acc)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}

// Mixed-precision FMA (v_fma_mix_f32: every source is an f32 register or one binary16 half of a register, one rounding):
//   fcp_mix_sum(h, l, HI)  = float(h.half) + float(l.half)      — exactly what v_cvt_f32_f16 x2 + v_add_f32 give (the conversions
//   fcp_mix_diff(x, h, HI) = x - float(h.half)                    are exact, so there is one rounding either way), in ONE instruction.
// The epilogues of every fp16x3 kernel decode / encode 8-16 values per lane and chunk with these; as separate converts and
// adds that was a third of the bottleneck-chain kernel's epilogue instructions.
template <int HI>
__device__ __forceinline__ float fcp_mix_sum(unsigned h, unsigned l) {
  float r;
  const float one = 1.0f;
  if constexpr (HI) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,1] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(h), "s"(one), "v"(l));
  else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(h), "s"(one), "v"(l));
  return r;
}
template <int HI>
__device__ __forceinline__ float fcp_mix_diff(float x, unsigned h) {
  float r;
  const float minus_one = -1.0f;
  if constexpr (HI) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "s"(minus_one), "v"(x));
  else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "s"(minus_one), "v"(x));
  return r;
}

// 8 fp32 -> 8 hi + 8 lo binary16 (round-toward-zero packs; lo = x - hi is exact in fp32).  Idempotent on
// values that already are a hi + lo sum, so elementwise kernels may decode / re-encode freely.
__device__ __forceinline__ void split8(const f32x4& x0, const f32x4& x1, u32x4_t& hi, u32x4_t& lo) {
  const float x[8] = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned hu = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(x[2 * q], x[2 * q + 1]));
    const float r0 = fcp_mix_diff<0>(x[2 * q], hu);
    const float r1 = fcp_mix_diff<1>(x[2 * q + 1], hu);
    hi[q] = hu;
    lo[q] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(r0, r1));
  }
}
// One pair of split8 (x0 in the low halves of hu / lu), for kernels that own two channels per thread.  split8 is not written
// over it: the compiler then pairs its eight conversions differently and the chain kernels' code changes.
__device__ __forceinline__ void split2(float x0, float x1, unsigned& hu, unsigned& lu) {
  hu = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(x0, x1));
  lu = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(fcp_mix_diff<0>(x0, hu), fcp_mix_diff<1>(x1, hu)));
}
// inverse: value = float(hi) + float(lo) (exact)
__device__ __forceinline__ void join8(const u32x4_t& hi, const u32x4_t& lo, float (&x)[8]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned hu = hi[q], lu = lo[q];
    x[2 * q] = fcp_mix_sum<0>(hu, lu);
    x[2 * q + 1] = fcp_mix_sum<1>(hu, lu);
  }
}
// byte offset of channel c (multiple of 8) inside a split32 pixel: group (c/32)*128 B, hi at (c%32)*2, lo +64
__device__ __forceinline__ long split_chan_off(int c) { return (long)(c >> 5) * 128 + (c & 31) * 2; }

// 8 consecutive channels of one pixel from an activation tensor of either format
__device__ __forceinline__ void load8(const float* base, long pix, int ld, int c, int fmt, float (&x)[8]) {
  if (fmt == 1) {
    const char* pb = reinterpret_cast<const char*>(base) + pix * ld * 4 + split_chan_off(c);
    join8(*reinterpret_cast<const u32x4_t*>(pb), *reinterpret_cast<const u32x4_t*>(pb + 64), x);
  } else {
    const f32x4 a = *reinterpret_cast<const f32x4*>(base + pix * ld + c);
    const f32x4 b = *reinterpret_cast<const f32x4*>(base + pix * ld + c + 4);
    x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3]; x[4] = b[0]; x[5] = b[1]; x[6] = b[2]; x[7] = b[3];
  }
}

// 8 finished channels of one pixel as the two 16-byte pieces that are stored: split32 hi | lo, or fp32 channels 0-3 | 4-7
__device__ __forceinline__ void pack8(const float (&v)[8], int fmt, u32x4_t& a, u32x4_t& b) {
  if (fmt == 1) {
    split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, a, b);
  } else {
    a = __builtin_bit_cast(u32x4_t, f32x4{v[0], v[1], v[2], v[3]});
    b = __builtin_bit_cast(u32x4_t, f32x4{v[4], v[5], v[6], v[7]});
  }
}
// ... and their store to channels c .. c + 7 of pixel pix; nt: split32 pieces with non-temporal (streaming) stores
__device__ __forceinline__ void store8(float* base, long pix, int ld, int c, int fmt, int nt, const u32x4_t& a, const u32x4_t& b) {
  if (fmt == 1) {
    char* ob = reinterpret_cast<char*>(base) + pix * ld * 4 + split_chan_off(c);
    if (nt) {
      __builtin_nontemporal_store(a, reinterpret_cast<u32x4_t*>(ob));
      __builtin_nontemporal_store(b, reinterpret_cast<u32x4_t*>(ob + 64));
    } else {
      *reinterpret_cast<u32x4_t*>(ob) = a;
      *reinterpret_cast<u32x4_t*>(ob + 64) = b;
    }
  } else {
    float* dst = base + pix * ld + c;
    *reinterpret_cast<u32x4_t*>(dst) = a;
    *reinterpret_cast<u32x4_t*>(dst + 4) = b;
  }
}
// both at once (one branch on the format)
__device__ __forceinline__ void pack_store8(float* base, long pix, int ld, int c, int fmt, int nt, const float (&v)[8]) {
  u32x4_t a, b;
  if (fmt == 1) {
    pack8(v, 1, a, b);
    store8(base, pix, ld, c, 1, nt, a, b);
  } else {
    pack8(v, 0, a, b);
    store8(base, pix, ld, c, 0, 0, a, b);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The fused epilogue's arithmetic.  This is the ONE statement of how a conv kernel finishes an output value; the staged
// (conv_epilogue, conv_epilogue8), register (conv_epilogue_regs), halo-tile, bottleneck-chain and stem epilogues all call
// it, which is what "every tile choice and every fused form returns the same bits" rests on:
//
//     x = acc * wscale + bias            conv_scale_bias
//     if res1 and res1_pre:      x += r1            \
//     x = x >= 0 ? x : x * act_slope                 |
//     x = x * alpha                                  |  conv_finish
//     if res1 and not res1_pre:  x += r1             |
//     if res2:                   x = x * alpha2 + r2 /
//
// Every operation is rounded on its own (the library is built with -ffp-contract=off).  PART OF THE CONTRACT: under
// act_slope 0 (ReLU) a negative x becomes x * 0.f = -0.0, not +0.0, and `* alpha` keeps that sign; a fused form that wrote
// max(x, 0) would differ from the stand-alone kernels in the sign bit of its zeros.  So the constant forms below go through
// the same multiplications (x * 0.f is not foldable: it is -0.0 for a negative x).
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float conv_scale_bias(float acc, float ws, float b) { return acc * ws + b; }

// The settings as plain values: the fused kernels pass constants.  conv_finish / conv_value take them from a ConvEpi or
// straight from the launch's ConvK (anything with these six members; res1 / res2 only say whether the term is present).
struct ConvEpi {
  bool res1, res1_pre, res2;
  float act_slope, alpha, alpha2;
};
template <typename E>
__device__ __forceinline__ float conv_finish(const E e, float x, float r1, float r2) {   // e by value: see profiles/conv_epilogue.md
  if (e.res1 && e.res1_pre) x += r1;
  x = x >= 0.f ? x : x * e.act_slope;
  x = x * e.alpha;
  if (e.res1 && !e.res1_pre) x += r1;
  if (e.res2) x = x * e.alpha2 + r2;
  return x;
}
template <typename E>
__device__ __forceinline__ float conv_value(const E& e, float acc, float ws, float b, float r1, float r2) {
  return conv_finish(e, conv_scale_bias(acc, ws, b), r1, r2);
}
// ReLU forms of the fused kernels (act_slope 0, alpha 1): relu(x), relu(x + r1) and relu(acc * ws + b); a negative x gives -0.0
__device__ __forceinline__ float conv_finish_relu(float x) { return conv_finish(ConvEpi{false, false, false, 0.f, 1.f, 1.f}, x, 0.f, 0.f); }
__device__ __forceinline__ float conv_finish_relu(float x, float r1) { return conv_finish(ConvEpi{true, true, false, 0.f, 1.f, 1.f}, x, r1, 0.f); }
__device__ __forceinline__ float conv_value_relu(float acc, float ws, float b) { return conv_finish_relu(conv_scale_bias(acc, ws, b)); }

// Pixel of a resized res1 that output pixel m = (ni, ho, wo) adds: nearest neighbour, floor(o * in / out) clamped to the map
// (hw = out_h * out_w).
__device__ __forceinline__ long res1_pixel(const ConvK& p, long m, int hw) {
  int ni, ho, wo;
  conv_out_pixel(p, m, hw, ni, ho, wo);
  int sh = (int)floorf(ho * p.res1_sh);
  int sw = (int)floorf(wo * p.res1_sw);
  sh = sh < p.res1_h - 1 ? sh : p.res1_h - 1;
  sw = sw < p.res1_w - 1 ? sw : p.res1_w - 1;
  return ((long)ni * p.res1_h + sh) * p.res1_w + sw;
}

// 32x32 MFMA C/D layout: accumulator register rr (0..15) of lane l holds column l & 31 of this row (half = l >> 5).
// (fcp_bneck_chain.hip spells the sum out at its three sites: through this function, in either association with the tile's
// first row, the compiler schedules those kernels differently and puts the two-source pair form into scratch.)
__device__ __forceinline__ constexpr int mfma_c_row(int rr, int half) { return (rr & 3) + 8 * (rr >> 2) + 4 * half; }

// The accumulators of a workgroup tile leave the MFMA layout through the fp32 tile Cs[BM][BN] (the staged epilogues), then
// the barrier.  (The last main-loop iteration ended with a barrier: the A/B slices are dead.)
template <int BN, int TM, int TN, int WTM, int WTN>
__device__ __forceinline__ void stage_acc_tile(const f32x16 (&acc)[TM][TN], float* Cs, int lane, int wm, int wn) {
  const int half = lane >> 5;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const int row = wm * WTM + i * 32 + mfma_c_row(rr, half);
        Cs[row * BN + wn * WTN + j * 32 + (lane & 31)] = acc[i][j][rr];
      }
  __syncthreads();
}

// Fused epilogue, shared by both MFMA variants.  `acc` is in the 32x32 MFMA C/D layout.
template <int BN, int TM, int TN, int WTM, int WTN>
__device__ __forceinline__ void conv_epilogue(const ConvK& p, f32x16 (&acc)[TM][TN], float* smem, int tile_m,
                                              int tile_n, int tid, int lane, int wm, int wn, int hw) {
  // ---- epilogue.  The accumulators leave the MFMA layout through LDS (stage_acc_tile), so that every lane owns
  // 16-byte row-major chunks: residual loads and output stores are then
  // float4-wide and a wave covers whole 512-byte..1-KiB runs of the NHWC row.
  constexpr int CPR = BN / 4;             // float4 chunks per tile row
  constexpr int RPP = 256 / CPR;          // rows per pass
  constexpr int PASSES = BM / RPP;
  float* Cs = smem;                       // [BM][BN]
  const int ccol = (tid % CPR) * 4;
  const int crow = tid / CPR;
  const int co = tile_n * BN + ccol;
  const bool vec = p.vec_ok && (co + 3 < p.cout);
  const long m0 = (long)tile_m * BM + crow;

  const bool pre1 = p.res1 != nullptr && !p.res1_resize && vec;
  const bool pre2 = p.res2 != nullptr && vec;
  stage_acc_tile<BN, TM, TN, WTM, WTN>(acc, Cs, lane, wm, wn);

  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f}, ws4 = {1.f, 1.f, 1.f, 1.f};
  if (p.bias != nullptr) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (co + e < p.cout) bias4[e] = p.bias[co + e];
  }
  if (p.wscale != nullptr) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (co + e < p.cout) ws4[e] = p.wscale[co + e];
  }
  constexpr int EPC = PASSES < 4 ? PASSES : 4;     // passes per group: bounds the residual registers
#pragma unroll 1
  for (int g = 0; g < PASSES; g += EPC) {
    f32x4 r1v[EPC], r2v[EPC];
    if (pre1) {
#pragma unroll
      for (int i = 0; i < EPC; ++i) {
        const long m = m0 + (long)(g + i) * RPP;
        r1v[i] = m < p.M ? *reinterpret_cast<const f32x4*>(p.res1 + m * p.res1_ld + co) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if (pre2) {
#pragma unroll
      for (int i = 0; i < EPC; ++i) {
        const long m = m0 + (long)(g + i) * RPP;
        r2v[i] = m < p.M ? *reinterpret_cast<const f32x4*>(p.res2 + m * p.res2_ld + co) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int i = 0; i < EPC; ++i) {
      const int row = crow + (g + i) * RPP;
      const long m = m0 + (long)(g + i) * RPP;
      if (m >= p.M || co >= p.cout) continue;
      f32x4 v = *reinterpret_cast<const f32x4*>(Cs + row * BN + ccol);
      f32x4 r1 = {0.f, 0.f, 0.f, 0.f}, r2 = {0.f, 0.f, 0.f, 0.f};
      if (pre1) {
        r1 = r1v[i];
      } else if (p.res1 != nullptr) {
        const long roff = (p.res1_resize ? res1_pixel(p, m, hw) : m) * p.res1_ld + co;
        if (vec) {
          r1 = *reinterpret_cast<const f32x4*>(p.res1 + roff);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (co + e < p.cout) r1[e] = p.res1[roff + e];
        }
      }
      if (pre2) {
        r2 = r2v[i];
      } else if (p.res2 != nullptr) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (co + e < p.cout) r2[e] = p.res2[m * p.res2_ld + co + e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = conv_value(p, v[e], ws4[e], bias4[e], r1[e], r2[e]);
      float* dst = p.out + m * p.out_ld + co;
      if (vec) {
        *reinterpret_cast<f32x4*>(dst) = v;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (co + e < p.cout) dst[e] = v[e];
      }
    }
  }
}


template <int I, int N, typename F>
__device__ __forceinline__ void fcp_static_for(F&& f) {          // f(std::integral_constant<int, I>{}) for I .. N - 1
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    fcp_static_for<I + 1, N>(f);
  }
}

// Epilogue straight from the accumulators of a TRANSPOSED tile (the filter fragment was the MFMA's row operand: filters x
// pixels — same products, same K order, same bits as the pixel-major tile): no fp32 tile in LDS, no barrier, no read-back.
// Lane l holds, for pixel (l & 31) of a 32 x 32 tile, filters 8 q + 4 (l >> 5) + 0..3 in accumulator quad q.  Three lane
// permutations per register (v_permlane32_swap on the quads, then v_permlane32_swap + v_permlane16_swap on the results)
// leave lane (p = l & 15, g = l >> 4) with channels 8 g .. 8 g + 7 of pixel p (set A) and of pixel 16 + p (set B): one
// 16-byte hi and one 16-byte lo store per set, four neighbouring lanes filling the 64 bytes of a pixel's hi (lo) half —
// the store pattern and the expressions of the staged epilogue (conv_epilogue8).  cout % 8 == 0, 16-byte aligned tensors.
// Round 3: the staged form took 36 k cycles per 256 x 256 tile of the 256-row kernel with its stores ablated
// (tools/big_epi_ablate.sh, profiles/r03_probes.md section 15).
//   m_start / m_end: rows of the workgroup tile; tm_act: row tiles of this wave that exist (<= TM); co_tile / co_end: channels
template <int TM, int TN, int WTM, int WTN>
__device__ __forceinline__ void conv_epilogue_regs(const ConvK& p, f32x16 (&acc)[TM][TN], int m_start, int m_end, int tm_act, int co_tile,
                                                   int co_end, int wm, int wn, int lane, int hw) {
    const int lp = lane & 15, lg = lane >> 4;
  auto swap32 = [](float& x, float& y) {                          // x.lanes[32:63] <-> y.lanes[0:31]
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    const unsigned r0 = r[0], r1 = r[1];
    x = __uint_as_float(r0); y = __uint_as_float(r1);
  };
  auto swap16 = [](float& x, float& y) {                          // odd 16-lane rows of x <-> even rows of y
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    const unsigned r0 = r[0], r1 = r[1];
    x = __uint_as_float(r0); y = __uint_as_float(r1);
  };
  // Issue order of the vector memory (round 5).  The first version loaded a set's residual, waited, computed, stored, and
  // went on to the next set: the stores may alias the residual as far as the compiler can tell, so it never moved a load
  // above an earlier store, and vmcnt retires in order — every one of the 2 TM TN sets waited for its own HBM round trip AND
  // for the acknowledgement of the previous set's stores (16 serial round trips per 256 x 256 tile with a residual: the
  // 1x1 expand + identity convs and the FPN merges spent two thirds of their time there).  Now the sets are handled in GROUPS
  // of up to two row tiles of one column tile (<= 4 sets): the residual pieces of the whole group are requested first (8
  // registers per set), THEN the finished previous group is stored, then the group is computed into registers: one exposed
  // round trip per group, and no wait ever sits behind a store.
  constexpr int GI = TM < 2 ? TM : 2;                              // row tiles per group
  constexpr int NGI = (TM + GI - 1) / GI;                          // groups per column tile
  constexpr int NG = TN * NGI;
  u32x4_t pend_a[GI][2], pend_b[GI][2];                            // finished values of the previous group (hi | lo, or 2 x f32x4)
  auto row_of = [&](int i, int set) { return m_start + wm * WTM + i * 32 + 16 * set + lp; };
  auto chan_of = [&](int jj) { return co_tile + wn * WTN + jj * 32 + 8 * lg; };
  auto flush = [&](auto gc) {                                      // stores of group g
    constexpr int g = decltype(gc)::value, jj = g / NGI, i0 = (g % NGI) * GI;
    const int co = chan_of(jj);
    fcp_static_for<0, GI>([&](auto ic) {
      constexpr int i = i0 + decltype(ic)::value;
      if constexpr (i < TM) {
        fcp_static_for<0, 2>([&](auto sc) {
          constexpr int set = decltype(sc)::value;
          const int mi = row_of(i, set);
          if (i < tm_act && mi < m_end && co < co_end) store8(p.out, mi, p.out_ld, co, p.out_fmt, 0, pend_a[i - i0][set], pend_b[i - i0][set]);
        });
      }
    });
  };
  fcp_static_for<0, NG>([&](auto gc) {
    constexpr int g = decltype(gc)::value, j = g / NGI, i0 = (g % NGI) * GI;
    const int co = chan_of(j);                                      // this lane's eight channels in column tile j
    const bool cok = co < co_end;
    const int cc = cok ? co : co_tile;
    // ---- the group's residual pieces (raw 16-byte loads, decoded at use)
    u32x4_t r1a[GI][2], r1b[GI][2];
    if (p.res1 != nullptr) {
      fcp_static_for<0, GI>([&](auto ic) {
        constexpr int i = i0 + decltype(ic)::value;
        if constexpr (i < TM) {
          fcp_static_for<0, 2>([&](auto sc) {
            constexpr int set = decltype(sc)::value;
            const int mi = row_of(i, set);
            const long m = (i < tm_act && mi < m_end && cok) ? (long)mi : (long)m_start;
            const long rpix = p.res1_resize ? res1_pixel(p, m, hw) : m;
            if (p.res1_fmt == 1) {
              const char* pb = reinterpret_cast<const char*>(p.res1) + rpix * p.res1_ld * 4 + split_chan_off(cc);
              r1a[i - i0][set] = *reinterpret_cast<const u32x4_t*>(pb);
              r1b[i - i0][set] = *reinterpret_cast<const u32x4_t*>(pb + 64);
            } else {
              r1a[i - i0][set] = *reinterpret_cast<const u32x4_t*>(p.res1 + rpix * p.res1_ld + cc);
              r1b[i - i0][set] = *reinterpret_cast<const u32x4_t*>(p.res1 + rpix * p.res1_ld + cc + 4);
            }
          });
        }
      });
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (g > 0) flush(std::integral_constant<int, g - 1>{});   // the previous group's stores, behind this group's loads
    __builtin_amdgcn_sched_barrier(0);
    float bias8[8], ws8[8];
    {
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(p.wscale + cc), w1 = *reinterpret_cast<const f32x4*>(p.wscale + cc + 4);
      f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
      if (p.bias != nullptr) { b0 = *reinterpret_cast<const f32x4*>(p.bias + cc); b1 = *reinterpret_cast<const f32x4*>(p.bias + cc + 4); }
#pragma unroll
      for (int e = 0; e < 4; ++e) { ws8[e] = w0[e]; ws8[4 + e] = w1[e]; bias8[e] = b0[e]; bias8[4 + e] = b1[e]; }
    }
    fcp_static_for<0, GI>([&](auto ic) {
      constexpr int i = i0 + decltype(ic)::value;
      if constexpr (i < TM) {
        float va[8], vb[8];                                           // sets A / B after the permutations
        fcp_static_for<0, 4>([&](auto ec) {
          constexpr int e = decltype(ec)::value;
          // (named floats: __builtin_bit_cast applied directly to a vector-element expression read element 0)
          float q0 = acc[i][j][e], q1 = acc[i][j][4 + e], q2 = acc[i][j][8 + e], q3 = acc[i][j][12 + e];
          swap32(q0, q1);               // q0: ch e (lanes 0-31) | 8 + e (32-63);   q1: 4 + e | 12 + e           of pixel l & 31
          swap32(q2, q3);               // q2: 16 + e | 24 + e;                     q3: 20 + e | 28 + e
          swap32(q0, q2); swap16(q0, q2);   // q0 = set A: rows of 16 lanes hold ch e, 8 + e, 16 + e, 24 + e of pixels 0-15; q2 = set B (pixels 16-31)
          swap32(q1, q3); swap16(q1, q3);   // the same for ch 4 + e, 12 + e, 20 + e, 28 + e
          va[e] = q0; va[4 + e] = q1; vb[e] = q2; vb[4 + e] = q3;
        });
        fcp_static_for<0, 2>([&](auto sc) {
          constexpr int set = decltype(sc)::value;
          float (&v)[8] = set == 0 ? va : vb;
          float r1[8], r2[8];
          if (p.res1 != nullptr) {
            if (p.res1_fmt == 1) {
              join8(r1a[i - i0][set], r1b[i - i0][set], r1);
            } else {
              const f32x4 fa = __builtin_bit_cast(f32x4, r1a[i - i0][set]), fb = __builtin_bit_cast(f32x4, r1b[i - i0][set]);
              r1[0] = fa[0]; r1[1] = fa[1]; r1[2] = fa[2]; r1[3] = fa[3]; r1[4] = fb[0]; r1[5] = fb[1]; r1[6] = fb[2]; r1[7] = fb[3];
            }
          }
          if (p.res2 != nullptr) {
            const int mi = row_of(i, set);
            load8(p.res2, (i < tm_act && mi < m_end && cok) ? (long)mi : (long)m_start, p.res2_ld, cc, p.res2_fmt, r2);
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = conv_value(p, v[e], ws8[e], bias8[e], r1[e], r2[e]);
          pack8(v, p.out_fmt, pend_a[i - i0][set], pend_b[i - i0][set]);
        });
      }
    });
  });
  flush(std::integral_constant<int, NG - 1>{});
}

// Epilogue for 8-channel granularity: used whenever the output or a residual is in split32 format
// (cout % 8 == 0, all tensors 16-byte aligned).  Same arithmetic as conv_epilogue.
template <int BN, int TM, int TN, int WTM, int WTN>
__device__ __forceinline__ void conv_epilogue8(const ConvK& p, f32x16 (&acc)[TM][TN], float* smem, int tile_m,
                                               int tile_n, int tid, int lane, int wm, int wn, int hw) {
  constexpr int CPR = BN / 8;
  constexpr int RPP = 256 / CPR;
  constexpr int PASSES = BM / RPP;
  float* Cs = smem;
  const int ccol = (tid % CPR) * 8;
  const int crow = tid / CPR;
  const int co = tile_n * BN + ccol;
  const long m0 = (long)tile_m * BM + crow;
  stage_acc_tile<BN, TM, TN, WTM, WTN>(acc, Cs, lane, wm, wn);
  if (co >= p.cout) return;
  float bias8[8], ws8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bias8[e] = p.bias != nullptr ? p.bias[co + e] : 0.f;
    ws8[e] = p.wscale != nullptr ? p.wscale[co + e] : 1.f;
  }
#pragma unroll
  for (int g = 0; g < PASSES; ++g) {
    const int row = crow + g * RPP;
    const long m = m0 + (long)g * RPP;
    if (m >= p.M) continue;
    float v[8], r1[8], r2[8];
    {
      const f32x4 a = *reinterpret_cast<const f32x4*>(Cs + row * BN + ccol);
      const f32x4 b = *reinterpret_cast<const f32x4*>(Cs + row * BN + ccol + 4);
      v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    }
    if (p.res1 != nullptr) load8(p.res1, p.res1_resize ? res1_pixel(p, m, hw) : m, p.res1_ld, co, p.res1_fmt, r1);
    if (p.res2 != nullptr) load8(p.res2, m, p.res2_ld, co, p.res2_fmt, r2);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = conv_value(p, v[e], ws8[e], bias8[e], r1[e], r2[e]);
    pack_store8(p.out, m, p.out_ld, co, p.out_fmt, p.nt_store, v);
  }
}

int launch_f16x3(const ConvK& k, int tile_n, bool cin4, hipStream_t s);
int launch_f16x3_dma(const ConvK& k, int tile_n, hipStream_t s);
int launch_f16x3_halo(const ConvK& k, hipStream_t s);           // 3x3 / stride 1 / pad 1, cout <= 64: 8x32 halo tiles, one pass per 32 filters
int launch_f16x3_halo_wide(const ConvK& k, hipStream_t s);      // same patch, cout <= 128, cin % 64 == 0: column tiles inner, tap ring
int launch_f16x3_big(const ConvK& k, int tile_n, hipStream_t s);   // 256-row tiles, tile_n 128 | 256

}  // namespace fcp_conv
