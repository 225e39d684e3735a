// Fused ResNet bottleneck chain (fp16x3 path, split32 tensors), 64-channel bottlenecks (ResNet-50 layer 1):
//
//     t2  = relu(bn2(conv2_3x3(t1)))                     64 -> 64      (never leaves the workgroup)
//     out = relu(bn3(conv3_1x1(t2)) + x)                 64 -> 256     (written once)
//     t1' = relu(bn1'(conv1'_1x1(out)))                  256 -> CN     (the NEXT block's conv1: CN = 64, or 128 for
//                                                                       layer2.0.conv1)
//
// i.e. torchvision's Bottleneck.forward (retinaface.py:93-99 builds the body from it) from conv2 of block b to
// conv1 of block b+1.  Unfused, those three launches move  t1 + 2 t2 + 2 t2.. = 6.7 GB per block through HBM at
// the bench size (64 x 160 x 160 px: x and out are 1.68 GB each at 4 B per element) and run at the HBM rate;
// fused, a workgroup reads its t1 tile (+ halo, from L2) and its x tile, writes out and t1':  4.2 GB.
//
// One 256-thread workgroup owns an 8 x 16 patch of output pixels; two workgroups share a CU (80 KiB of LDS each), so
// one computes while the other waits on memory.
//
//   phase 1   implicit GEMM 128 x 64 x 576 over the patch's halo, staged once per channel slice (see PATCH below),
//             epilogue -> T2 in LDS as the split32 operand image [2 slices][128 rows][128 B].
//   chunks    for each group j of 32 output channels of conv3 (8 groups):
//               phase 2  acc2[128 x 32]  = T2 . W3[j]^T                (K = 64; W3 group by LDS-DMA, double-buffered)
//               epilogue out[:, j] = relu(acc2 * ws3 + b3 + x[:, j]) -> HBM, and -> T3 in LDS (operand image)
//               phase 3  acc3[128 x CN] += T3 . W1'[:, j]^T            (K slice j of conv1'; by LDS-DMA)
//   epilogue  t1' = relu(acc3 * ws1 + b1) -> HBM.
//
// Arithmetic is that of the stand-alone kernels, instruction for instruction (al*bh + ah*bl + ah*bh per k-half,
// K slices in ascending order, the same fp32 epilogue expressions, the same hi/lo split of every stored tensor), so
// out and t1' are BIT-IDENTICAL to running the three convolutions separately (tests/test_chain_gpu.py).
//
// The same chunk loop also runs WITHOUT phase 1 ("pair": HAS_C2 = false) on tiles of 128 consecutive pixels of
// 128-channel inputs, whose operand tile is then fetched by LDS-DMA instead of being computed:
//     out = relu(bn3(conv3_1x1(t)) [+ x])   128 -> NOUT;    t1' = relu(bn1'(conv1'_1x1(out)))   NOUT -> CN
//   * NOUT = 512, with residual, CN = 128:  conv3 of a layer-2 identity block + conv1 of the next block: the 512-channel
//     tensor (0.84 GB at the bench size) is not read back by a separate conv1 launch;
//   * NOUT = 256, no residual, CN = 64:  layer1.0's conv3 + downsample (one K-concatenated 1x1 conv over [conv2 out |
//     pooled stem]) + layer1.1's conv1.
// 128 KiB of LDS, one workgroup per CU.
#include "fcp_conv_common.h"

#include <type_traits>

using namespace fcp_conv;

namespace {

constexpr int FCP_CHAIN_STORE_AUX = 2;   // cache policy of the `out` stores of the chunk loop: nt (0 default / 16 sc1 measured equal)

struct ChainK {
  const float* t1;  unsigned t1_bytes;  int t1_ld;
  const float* w2;  unsigned w2_bytes;  const float* ws2;  const float* b2;
  const float* w3;  unsigned w3_bytes;  const float* ws3;  const float* b3;
  const float* res; int res_ld;
  float* out;       int out_ld;    unsigned out_bytes;
  const float* w1n; unsigned w1n_bytes; const float* ws1n; const float* b1n;
  float* t1n;       int t1n_ld;
  int n, h, w, M;
  int nt_store;
  int out_even;     // patch form: store `out` at even (y, x) only (FCP_CHAIN_OUT_EVEN_ONLY)
  // two-source pair (DIRECT forms): the trailing channels of conv3's input come from t1b, a split32 tensor (n, hb, wb, t1b_ld)
  // sampled at (y * sb, x * sb) — the K concatenation [conv2 out | x(::s, ::s)] of a stride-2 bottleneck's conv3 + downsample
  const float* t1b; unsigned t1b_bytes; int t1b_ld, hb, wb, sb;
};

// Pixels per workgroup tile: BMT = 128, 4 waves, up to two workgroups per CU; a wave owns 32 rows.  (Tiles of 256 pixels on
// 8 waves, one workgroup per CU, halve the filter traffic per pixel and were measured 0-6 % slower: profiles/r03_probes.md.)
constexpr int BMT = 128;
constexpr int C = 64;                 // bottleneck width of the variant with phase 1
constexpr int ROWB = 128;             // bytes per LDS operand row: 32 hi + 32 lo binary16
constexpr int STAGE = (BMT + C) * ROWB;         // 24 KiB; region 0 of the conv2 forms is two of these (phase 1's halo patch and filter stages)
constexpr int CT_OFF = 0;                       // chunk loop: BMT x 32 fp32 epilogue tile, rewritten in place as T3 (16 KiB)
constexpr int W1B_OFF = BMT * 128;              // chunk loop: K slice j of conv1' (CN rows x 128 B)
// conv1' K slices are double-buffered wherever LDS allows (everything but the conv2 form with CN = 128, whose chunk buffers
// live in the 48 KiB of the dead phase-1 stages): the next slice's DMA can then be issued BEFORE the chunk's `out` stores,
// see the chunk loop
constexpr bool w1_double(int cn, bool has_c2) { return !has_c2 || W1B_OFF + 2 * cn * 128 + 2 * C * 128 <= 2 * STAGE; }
constexpr int w3b_off(int cn, bool has_c2) { return W1B_OFF + (w1_double(cn, has_c2) ? 2 : 1) * cn * 128; }   // conv3 filter groups, 2 x (CW * 128 B)
// region 0 = phase-1 stages | epilogue tiles | chunk buffers; the operand tile T2 (BMT x CW, 4 B per element) follows it
constexpr int r0_bytes(int cw, int cn, bool has_c2) { return has_c2 ? 2 * STAGE : w3b_off(cn, has_c2) + 2 * cw * 128; }
// In the pair forms T2 ALIASES the chunk buffers: a wave's T2 fragments are the same for every chunk and live in
// registers, so the tile is only needed until they have been read.  That is what lets the 256-wide pair fit at all
// (144 + 128 KiB otherwise) and brings the 128-wide pairs down to 80 KiB: TWO workgroups per CU, the second one's
// MFMAs under the first one's epilogue (without the alias the 128-wide pairs took 128-144 KiB, one per CU).
constexpr bool alias_t2(bool has_c2) { return !has_c2; }
// DIRECT (two-source pair forms, round 5): the operand tile never exists in LDS at all — a lane's fragments are 16-byte pieces of
// the split32 pixel rows, i.e. plain buffer loads straight into the registers they live in for the whole chunk loop (a
// 128 x 384-channel tile is 192 KiB: it fits neither LDS nor an alias of the chunk buffers); LDS holds the chunk buffers only.
constexpr int lds_bytes(int cw, int cn, bool has_c2, bool direct = false) {   // 80 KiB (two per CU) | 112-160 KiB
  const int r0 = r0_bytes(cw, cn, has_c2), t2 = BMT * cw * 4;
  if (direct) return r0;
  return !alias_t2(has_c2) ? r0 + t2 : (r0 > W1B_OFF + t2 ? r0 : W1B_OFF + t2);
}
constexpr int wgs_per_cu(int cw, int cn, bool has_c2, bool direct = false) {
  // the two-source DIRECT pair holds 48 fragments + conv1's accumulators: one wave per SIMD; the EXPAND form (cn = 0: conv3 only,
  // no conv1' — no accumulators, no conv1' buffers: 80 KiB, < 256 registers) runs two workgroups per CU
  if (direct) return cn == 0 && lds_bytes(cw, cn, has_c2, true) <= 80 * 1024 ? 2 : 1;
  return lds_bytes(cw, cn, has_c2) <= 80 * 1024 ? 2 : 1;
}

// acc += al * bh + ah * bl + ah * bh: the fp16x3 product of one k-half, the small terms first
__device__ __forceinline__ void mfma3(f32x16& acc, const f16x8& ah, const f16x8& al, const f16x8& bh, const f16x8& bl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
}

// Eight channels of an fp32 tile row -> relu(acc * ws + b) (conv2's and conv1's tile epilogues)
__device__ __forceinline__ void row_values8(const float* c8, const float (&ws8)[8], const float (&b8)[8], float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(c8);
  const f32x4 b = *reinterpret_cast<const f32x4*>(c8 + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = conv_value_relu(a[e], ws8[e], b8[e]);
    v[4 + e] = conv_value_relu(b[e], ws8[4 + e], b8[4 + e]);
  }
}

// PATCH (the conv2 forms): the tile is an 8 x 16 PATCH of one image instead of 128 consecutive pixels, and phase 1 stages the
// patch's (8 + 2) x (16 + 2) halo ONCE per 32-channel slice; the nine taps read it at shifted rows (the scheme of
// conv3x3_halo_f16x3).  A tile of consecutive pixels fetches a 128-byte operand row per pixel, tap and slice: 288 of the ~720
// one-KiB vector-memory instructions a tile issues — and the chain kernels are bound by exactly that path
// (profiles/r04_probes.md section 1: same cycles with and without their MFMAs).  The halo form issues 46.  Same K order (channel
// slice outer, taps inner), same terms: bit-identical.
// Direct forms (operand fragments straight from global memory, no LDS tile): the two-source pair (cw2 > 0) and the EXPAND form
// (cn = 0, round 5): conv3 + identity of a block WITHOUT the next block's conv1 — out = relu(conv3(t1) + res) and nothing else.
// Where the pair needs one wave per SIMD (layer 3: 128 accumulator + 128 fragment registers), the expand form needs 128 + 16 and
// 80 KiB, i.e. two workgroups per CU like the forms that sit nearest their floors, and conv1' runs on the 256-row kernel.
constexpr bool direct_form(int cn, int cw2) { return cw2 > 0 || cn == 0; }
template <int CN, int CW, int NOUT, bool HAS_C2, bool HAS_RES, int CW2 = 0>
__global__ void __launch_bounds__(2 * BMT, wgs_per_cu(CW, CN, HAS_C2, direct_form(CN, CW2))) bneck_chain_c64(const ChainK p) {
  constexpr bool DIRECT = direct_form(CN, CW2);   // fragments loaded straight from global memory: the two-source pair (CW - CW2 channels from t1, CW2 from t1b)
  static_assert(!DIRECT || (!HAS_C2 && CW2 % 32 == 0 && CW2 < CW), "direct forms are pair forms");
  constexpr bool HAS_P3 = CN > 0;                   // conv1' of the next block (phase 3); false: the expand form
  static_assert(!HAS_C2 || CW == C, "phase 1 is written for 64-channel bottlenecks");
  constexpr bool PATCH = HAS_C2;                    // the conv2 forms run on pixel patches
  constexpr int PH = BMT / 16;                      // PATCH: rows of the (PH x 16)-pixel patch: 8
  constexpr int NTHR = 2 * BMT;                     // threads: one wave per 32 rows
  constexpr int NW = NTHR / 64;                     // waves
  constexpr int LR = NTHR / 8;                      // rows one DMA pass of the workgroup covers (8 rows per wave instruction)
  constexpr int TN3 = CN / 32;
  constexpr int TN3A = TN3 > 0 ? TN3 : 1;           // array extents (the expand form has no conv1' tiles)
  constexpr int CS = CW / 32;                       // K slices of conv3
  constexpr int NCH = NOUT / 32;                    // groups of 32 conv3 filters
  constexpr int W3CH = CW * 128;                    // bytes of one conv3 filter group in LDS
  constexpr bool ALIAS = alias_t2(HAS_C2) && !DIRECT;
  constexpr int T2_OFF = ALIAS ? W1B_OFF : r0_bytes(CW, CN, HAS_C2);
  constexpr int WGS = wgs_per_cu(CW, CN, HAS_C2, DIRECT);
  constexpr int WPS = WGS * NW / 4;                 // waves per SIMD: 2 = 256 registers per wave
  static_assert(lds_bytes(CW, CN, HAS_C2, DIRECT) <= 160 * 1024, "LDS budget");
  constexpr bool W1DB = w1_double(CN, HAS_C2);
  // The next chunk's filter DMAs: one at a time BETWEEN the phase-2 MFMAs, or as a burst at the top of the chunk.  An LDS-DMA
  // instruction holds its wave until the vector-memory path has taken it.  With ONE wave per SIMD (the one-workgroup pair
  // forms) a burst of CS + CN / 32 of them is ~1000-2000 cycles with the matrix pipe idle, and spreading them wins (layer-3
  // pair 451 vs 493 us); with TWO workgroups per CU the other workgroup's wave covers a burst, while spread instructions
  // stretch phase 2 to 5250 cycles for 768 cycles of MFMAs: the burst wins there (layer-2 pair 644 -> 525-548 us).  The
  // conv2 forms (two per CU, few filter pieces) are 1.5 % better spread.  profiles/r03_probes.md.
  constexpr bool SPREAD = W1DB && (HAS_C2 || WPS == 1);
  constexpr bool W1PRE = W1DB && !DIRECT && (HAS_C2 ? CN <= 64 || WPS == 1 : CN <= 128 && WPS == 1);   // conv1' fragments of a chunk requested under phase 2 (registers permitting)
  constexpr int W3B_OFF = w3b_off(CN, HAS_C2);
  static_assert(!HAS_C2 || W3B_OFF + 2 * W3CH <= 2 * STAGE, "chunk buffers must fit the phase-1 stage region");
  constexpr int NRES = HAS_RES ? 4 : 0;             // residual loads per chunk and thread
  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);

  const int tile_m = xcd_tile_order(gridDim.x, blockIdx.x);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int lrow = tid >> 3;                                     // 0..LR-1 (+LR i)
  const int csrc = (tid & 7) ^ swz(lrow);                        // source chunk of LDS position tid & 7
  const int l31 = lane & 31, half = lane >> 5;
  int offH[2], offL[2];                                          // fragment chunk offsets inside a 128-byte row, per k-half
  frag_offsets(lane, offH, offL);
  // the hi and lo fragment of k-half s of the 128-byte operand row at `row`
  auto frag_pair = [&](const char* row, int s, f16x8& hi, f16x8& lo) {
    hi = *reinterpret_cast<const f16x8*>(row + offH[s]);
    lo = *reinterpret_cast<const f16x8*>(row + offL[s]);
  };
  const int hw = p.h * p.w;
  // tile row -> pixel index in (n, h, w) order, or -1 for a row that has no pixel (past the end / outside the image)
  int pn = 0, py0 = 0, px0 = 0;                                  // PATCH: image and top-left pixel of the 8 x 16 patch
  if constexpr (PATCH) {
    const int txn = (p.w + 15) >> 4, tyn = (p.h + PH - 1) / PH;
    const int r = tile_m / txn;
    px0 = (tile_m - r * txn) * 16;
    pn = r / tyn;
    py0 = (r - pn * tyn) * PH;
  }
  auto pix = [&](int row) -> long {
    if constexpr (PATCH) {
      const int y = py0 + (row >> 4), x = px0 + (row & 15);
      return (y < p.h && x < p.w) ? ((long)pn * p.h + y) * p.w + x : -1L;
    } else {
      const long m = (long)tile_m * BMT + row;
      return m < p.M ? m : -1L;
    }
  };

  // ---- conv2 epilogue: fp32 tile [BMT][64] over the dead phase-1 buffers -> relu(acc * ws2 + b2) -> T2
  auto conv2_epilogue = [&](const f32x16 (&acc1)[2], int wm, int wn) {
    float* Cs = smem;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const int row = wm * 64 + i * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * half;   // mfma_c_row (fcp_conv_common.h), spelled out: see there
        Cs[row * C + wn * 32 + l31] = acc1[i][rr];
      }
    __syncthreads();
    {
      const int ccol = (tid & 7) * 8;
      float ws8[8], b8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        ws8[e] = p.ws2[ccol + e];
        b8[e] = p.b2[ccol + e];
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = (tid >> 3) + LR * g;
        float v[8];
        row_values8(Cs + row * C + ccol, ws8, b8, v);
        u32x4_t hi, lo;
        split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, hi, lo);
        const int q = (ccol & 31) >> 3, sw = swz(row);
        char* trow = lds + T2_OFF + (ccol >> 5) * (BMT * ROWB) + row * ROWB;
        *reinterpret_cast<u32x4_t*>(trow + ((q ^ sw) << 4)) = hi;
        *reinterpret_cast<u32x4_t*>(trow + (((4 + q) ^ sw) << 4)) = lo;
      }
    }
    __syncthreads();                                             // T2 complete; the fp32 tile is dead
  };

  // =========================================================================================== phase 1: 3x3 conv
  if constexpr (HAS_C2) {
    constexpr int HALO = (PH + 2) * 18;                          // 10 x 18 = 180 halo rows ...
    constexpr int HROWS = (HALO + LR - 1) / LR * LR;             // ... padded to whole DMA passes: 192
    constexpr int ASL = HROWS * ROWB;                            // one channel slice of the halo patch: 24 KiB
    // filter stages behind the two slices: TPB = 2 taps (K slices of 8 KiB) per stage and per workgroup barrier
    // (one tap per barrier measured equal: profiles/r04_probes.md 1e)
    constexpr int TPB = 2, NSTEP = 18 / TPB;
    static_assert(18 % TPB == 0, "taps per barrier must divide the 18 K slices");
    constexpr int BST_OFF = 2 * ASL, BSL = C * ROWB, BSTG = TPB * BSL;
    static_assert(BST_OFF + 2 * BSTG <= T2_OFF + BMT * C * 4, "halo patch + filter stages must fit region 0 + T2");
    f32x16 acc1[2];
    const int wm = wave / 2, wn = wave % 2;                      // 2 x 2 waves of 64 x 32
    __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.t1), 0, p.t1_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w2), 0, p.w2_bytes, 0x00020000);
    // ---- the halo patch, both channel slices: 6 passes of 32 rows each (rows >= 180 and pixels outside the image: zero fill)
#pragma unroll
    for (int i = 0; i < HROWS / LR; ++i) {
      const int r = lrow + LR * i;
      const int hy = r / 18, hx = r - hy * 18;
      const int y = py0 - 1 + hy, x = px0 - 1 + hx;
      const bool ok = r < HALO && (unsigned)y < (unsigned)p.h && (unsigned)x < (unsigned)p.w;
      const unsigned src = ok ? ((unsigned)((pn * p.h + y) * p.w + x) * (unsigned)p.t1_ld + (unsigned)(csrc * 4)) * 4u : 0xFFFFFFFFu;
#pragma unroll
      for (int cs = 0; cs < 2; ++cs)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (__attribute__((address_space(3))) void*)(lds + cs * ASL + (wave_u * 8 + LR * i) * ROWB), 16,
                                                 (int)(src == 0xFFFFFFFFu ? 0xFFFFFFFFu : src + (unsigned)(cs * 32 * 4)), 0, 0, 0);
    }
    constexpr int B_LD = C / LR;
    unsigned woff[B_LD];
#pragma unroll
    for (int i = 0; i < B_LD; ++i) woff[i] = (unsigned)(((lrow + LR * i) * (9 * C) + csrc * 4) * 4);
    auto dma_b = [&](int step, int stage) {                      // the TPB K slices of a step
#pragma unroll
      for (int u = 0; u < TPB; ++u)
#pragma unroll
        for (int i = 0; i < B_LD; ++i)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (__attribute__((address_space(3))) void*)(lds + BST_OFF + stage * BSTG + u * BSL + (wave_u * 8 + LR * i) * ROWB), 16,
                                                   (int)(woff[i] + (unsigned)((step * TPB + u) * BK * 4)), 0, 0, 0);
    };
    dma_b(0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc1[i][e] = 0.f;
    // halo row of the lane's pixel in the wave's two 32-row tiles: pixel p = wm * 64 + 32 i + l31 -> (p >> 4, p & 15)
    int hr0[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) hr0[i] = (wm * 4 + i * 2 + (l31 >> 4)) * 18 + (l31 & 15);
    const char* Bw = lds + BST_OFF + (wn * 32 + l31) * ROWB;
    fcp_static_for<0, NSTEP>([&](auto gc) {
      constexpr int g = decltype(gc)::value;
      // the filter slices of step g have landed (with the halo patch, at g = 0) and every wave has read those of step g - 1
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      fcp_static_for<0, TPB>([&](auto uc) {
        constexpr int kt = g * TPB + decltype(uc)::value, cs = kt / 9, tap = kt % 9;   // K order: channel slice outer, taps inner
        const char* Bb = Bw + (g & 1) * BSTG + decltype(uc)::value * BSL;
        f16x8 ah[2][2], al[2][2], bh[2], bl[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int hr = hr0[i] + (tap / 3) * 18 + tap % 3;
          const int sw = swz(hr);
          const char* Ab = lds + cs * ASL + hr * ROWB;
#pragma unroll
          for (int sq = 0; sq < 2; ++sq) {
            ah[sq][i] = *reinterpret_cast<const f16x8*>(Ab + (((2 * sq + half) ^ sw) << 4));
            al[sq][i] = *reinterpret_cast<const f16x8*>(Ab + (((4 + 2 * sq + half) ^ sw) << 4));
          }
        }
#pragma unroll
        for (int sq = 0; sq < 2; ++sq) {
          frag_pair(Bb, sq, bh[sq], bl[sq]);
        }
        if constexpr (decltype(uc)::value == TPB - 1) {
          // the step's last fragment reads are out: the next step's filters may go into the stage step g - 1 has left.
          // (Issued behind ALL LDS reads of the step: the compiler drains pending LDS-DMA in front of an LDS read.)
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (g + 1 < NSTEP) dma_b(g + 1, (g + 1) & 1);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int sq = 0; sq < 2; ++sq)
#pragma unroll
          for (int i = 0; i < 2; ++i)
            mfma3(acc1[i], ah[sq][i], al[sq][i], bh[sq], bl[sq]);
        __builtin_amdgcn_sched_barrier(0);
      });
    });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                  // every wave has consumed the last slice: patch and stages are dead
    __builtin_amdgcn_sched_barrier(0);
    conv2_epilogue(acc1, wm, wn);
  } else if constexpr (!DIRECT) {
    // ---- no conv2: the operand tile is the input itself (CS slices of 128 pixels x 128 B), by LDS-DMA
    __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.t1), 0, p.t1_bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < BMT / LR; ++i) {
      const int m = tile_m * BMT + lrow + LR * i;
      const unsigned ro = m < p.M ? ((unsigned)m * (unsigned)p.t1_ld + (unsigned)(csrc * 4)) * 4u : 0xFFFFFFFFu;
#pragma unroll
      for (int sl = 0; sl < CS; ++sl)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_in, (__attribute__((address_space(3))) void*)(lds + T2_OFF + sl * BMT * ROWB + wave_u * 8 * ROWB + LR * i * ROWB),
                                                 16, (int)(ro == 0xFFFFFFFFu ? 0xFFFFFFFFu : ro + (unsigned)(sl * 128)), 0, 0, 0);
    }
  }

  // ========================================================================== chunk loop: conv3 (+x, relu) and conv1'
  __amdgpu_buffer_rsrc_t rs_w3 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w3), 0, p.w3_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rs_w1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w1n), 0, p.w1n_bytes, 0x00020000);
  // conv3 filter group j: 32 rows x CS K slices = 4 CS pieces of 8 rows.  Wave w moves pieces w PW3 .. w PW3 + PW3 - 1.
  constexpr int PW3 = 4 * CS / NW;                  // per wave: CS
  constexpr int PW1 = CN / (8 * NW);                // conv1' slice: CN rows, 8 per wave instruction
  static_assert(PW3 >= 1 && (PW1 >= 1 || !HAS_P3), "filter pieces per wave");
  // piece i of the wave's share of filter group j: 8 rows of one K slice
  auto w3_piece = [&](int i, int j, int buf) {
    const int g = wave_u * PW3 + i, sl = g >> 2, r = (g & 3) * 8 + (lane >> 3);
    char* dst = lds + W3B_OFF + buf * W3CH + sl * 4096 + (g & 3) * 8 * ROWB;
    const unsigned src = (unsigned)((j * 32 + r) * (CW * 4) + sl * 128 + (((lane & 7) ^ swz(r)) << 4));
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w3, (__attribute__((address_space(3))) void*)dst, 16, (int)src, 0, 0, 0);
  };
  // conv1' K slice j: CN rows.  Wave w moves rows w * CN/NW + 8 i + lane / 8, piece i at a time.
  auto w1_piece = [&](int i, int j, int buf) {
    char* dst = lds + W1B_OFF + buf * (CN * ROWB) + wave_u * (CN / NW) * ROWB;
    const int r = wave_u * (CN / NW) + 8 * i + (lane >> 3);
    const unsigned src = (unsigned)(r * (NOUT * 4) + j * 128 + (((lane & 7) ^ swz(r)) << 4));
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w1, (__attribute__((address_space(3))) void*)(dst + 8 * i * ROWB), 16, (int)src, 0, 0, 0);
  };
  auto dma_w3 = [&](int j, int buf) {
#pragma unroll
    for (int i = 0; i < PW3; ++i) w3_piece(i, j, buf);
  };
  auto dma_w1 = [&](int j, int buf) {
#pragma unroll
    for (int i = 0; i < PW1; ++i) w1_piece(i, j, buf);
  };
  // instruction k of {filter group j, conv1' slice j} (PW3 + PW1 per wave), for issue between the phase-2 MFMAs
  // (the loops above written as fcp_static_for over dma_one cost seven kernels their code and two of them registers)
  constexpr int NDMA = PW3 + PW1;
  auto dma_one = [&](auto kc, int j, int buf) {
    constexpr int k = decltype(kc)::value;
    if constexpr (k < PW3) w3_piece(k, j, buf);
    else w1_piece(k - PW3, j, buf);
  };

  f32x16 acc3[TN3A];
#pragma unroll
  for (int t = 0; t < TN3; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc3[t][e] = 0.f;

  const char* a2base = lds + T2_OFF + (wave * 32 + l31) * ROWB;   // + slice * BM * ROWB
  const char* a3base = lds + CT_OFF + (wave * 32 + l31) * ROWB;
  // Epilogue items of this thread: rows erow0, erow0 + 16 OF THE WAVE'S OWN 32 ROWS, channel group eq (8 channels) of the
  // 32-channel chunk.  A wave stages, finishes and re-reads (phase 3) only its own rows of the epilogue tile, so the three
  // steps of a chunk need no workgroup barrier between them and the four waves may drift apart inside a chunk (one wave's
  // MFMAs beside another's epilogue); what the waves share are the filter buffers: ONE barrier per chunk.
  const int eq = lane & 3;
  const int erow0 = wave * 32 + (lane >> 2);
  long rm[2];                                                    // residual pixel of the two items (clamped)
  unsigned so[2];                                                // byte offset of the two items in `out`, 0xFFFFFFFF past the end
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int prow = erow0 + 16 * it;
    const long m = pix(prow);
    rm[it] = m >= 0 ? m : (long)p.M - 1;
    // out_even: a stride-2 consumer reads even (y, x) only — patch origins are even, so the parity is that of the tile row;
    // the dropped stores still issue (exact vmcnt), the hardware discards them: no HBM traffic
    const bool keep = !PATCH || !p.out_even || ((((prow >> 4) | prow) & 1) == 0);
    so[it] = (m >= 0 && keep) ? (unsigned)(m * p.out_ld * 4 + eq * 16) : 0xFFFFFFFFu;
  }
  __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(p.out, 0, p.out_bytes, 0x00020000);

  // ---- vector-memory issue order.  vmcnt retires IN ORDER and an `out` store to HBM takes microseconds to be
  // acknowledged, so no wait may sit behind a store it does not need.  Per chunk j (all counts per thread):
  //     top(j):   wait for D(j) = {conv3 filter group j, conv1' slice j}; barrier; issue D(j+1) into the other buffers
  //     phase 2, epilogue (consumes the residual R(j)); issue c(j+1) x2 (the lane's scale / bias), R(j+1) x NRES
  //     phase 3; issue the stores S(j) x4 through a buffer resource (rows past the end are dropped by the hardware:
  //     the count is exact)
  // D(j+1) is a whole chunk ahead of its use and the ops younger than it at top(j+1) are exactly c(j+1), R(j+1), S(j):
  // vmcnt(6 + NRES) waits for the DMAs without touching the stores, which are first forced two chunks after their
  // issue.  Where LDS has no room for a second conv1' buffer (W1DB false) slice j is issued at top(j) and a second
  // wait + barrier in front of phase 3 drains S(j-1) with it.
  u32x4_t rhi[2], rlo[2];
  auto load_res = [&](int j) {
    if constexpr (!HAS_RES) return;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const char* pb = reinterpret_cast<const char*>(p.res) + rm[it] * p.res_ld * 4 + j * 128 + eq * 16;
      rhi[it] = *reinterpret_cast<const u32x4_t*>(pb);
      rlo[it] = *reinterpret_cast<const u32x4_t*>(pb + 64);
    }
  };
  const int nch = NCH;
  float ws_l = p.ws3[l31], b_l = p.b3[l31];                      // this lane's conv3 channel of chunk 0 (MFMA layout: col = lane & 31)
  constexpr int NCONST = 2;
  f16x8 ah[CS][2], al[CS][2];                                    // phase-2 A fragments: the wave's own 32 rows of T2, [slice][k-half]
  auto read_a2 = [&]() {
#pragma unroll
    for (int sl = 0; sl < CS; ++sl)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        frag_pair(a2base + sl * BMT * ROWB, s, ah[sl][s], al[sl][s]);
      }
  };
  if constexpr (DIRECT) {
    // ---- the wave's operand fragments straight from the two source tensors: lane (l31, half) of k-half s of slice sl needs
    //      the 16-byte pieces (2 s + half) [hi] and (4 + 2 s + half) [lo] of its pixel's 128-byte channel-slice record — the
    //      split32 format IS the fragment layout.  Rows past the end read zeros (out-of-range buffer offsets).
    constexpr int CS1 = (CW - CW2) / 32;
    __amdgpu_buffer_rsrc_t rs_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.t1), 0, p.t1_bytes, 0x00020000);
    __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.t1b), 0, p.t1b_bytes, 0x00020000);
    // chunk 0's filters first: their L2 round trip runs under the fragments' HBM round trip (one wait for both)
    asm volatile("" ::: "memory");
    dma_w3(0, 0);
    if constexpr (W1DB) dma_w1(0, 0);
    asm volatile("" ::: "memory");
    const long m = pix(wave * 32 + l31);
    unsigned oa = 0xFFFFFFFFu, ob = 0xFFFFFFFFu;
    if (m >= 0) {
      const int ni = (int)(m / hw);
      const int rem = (int)(m - (long)ni * hw);
      const int y = rem / p.w, x = rem - y * p.w;
      oa = (unsigned)m * (unsigned)p.t1_ld * 4u;
      ob = ((unsigned)(ni * p.hb + y * p.sb) * (unsigned)p.wb + (unsigned)(x * p.sb)) * (unsigned)p.t1b_ld * 4u;
    }
#pragma unroll
    for (int sl = 0; sl < CS; ++sl)
#pragma unroll
      for (int sk = 0; sk < 2; ++sk) {
        const bool first = sl < CS1;                                 // compile-time after unrolling
        const unsigned base = first ? oa : ob;
        const unsigned off = (unsigned)((first ? sl : sl - CS1) * 128);
        const unsigned vh = base == 0xFFFFFFFFu ? base : base + off + (unsigned)((2 * sk + half) << 4);
        const unsigned vl = base == 0xFFFFFFFFu ? base : base + off + (unsigned)((4 + 2 * sk + half) << 4);
        ah[sl][sk] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(first ? rs_a : rs_b, (int)vh, 0, 0));
        al[sl][sk] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(first ? rs_a : rs_b, (int)vl, 0, 0));
      }
    // all of them landed HERE, outside the chunk loop: a fragment the compiler still believed in flight at the loop header
    // would get a conservative vmcnt wait in front of its first use in EVERY chunk, draining the loop's counted pipeline
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int sl = 0; sl < CS; ++sl)
#pragma unroll
      for (int sk = 0; sk < 2; ++sk) asm volatile("" : "+v"(ah[sl][sk]), "+v"(al[sl][sk]));
    __builtin_amdgcn_sched_barrier(0);
  }
  if constexpr (ALIAS) {                                         // T2 shares LDS with the chunk buffers: fragments first, filters after
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    read_a2();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
  asm volatile("" ::: "memory");
  if constexpr (!DIRECT) {
    dma_w3(0, 0);
    if constexpr (W1DB) dma_w1(0, 0);
  }
  asm volatile("" ::: "memory");
  if (nch > 0) load_res(0);
  __builtin_amdgcn_sched_barrier(0);

  for (int j = 0; j < nch; ++j) {
    const bool more = j + 1 < NCH;
    // ---- top: this chunk's filters have landed (everything younger may fly), every wave is done with chunk j - 1
    // (W1DB false: group j was issued at top(j-1) and already forced by the wait in front of phase 3 of chunk j-1; the
    //  ops younger than that wait — c(j), R(j), S(j-1) — may all stay in flight, which is the same count)
    if (j == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NRES) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + NCONST + NRES) : "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!SPREAD) {
      if (more) dma_w3(j + 1, (j + 1) & 1);
      if constexpr (W1DB) {
        if (more) dma_w1(j + 1, (j + 1) & 1);
      } else {
        dma_w1(j, 0);
      }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    // ---- phase 2 operands: T2 (A: the wave's own 32 rows, the same for every chunk — read once, kept in registers) and
    //      filter group j (B), all K slices
    const char* b2base = lds + W3B_OFF + (j & 1) * W3CH + l31 * ROWB;
    if constexpr (!ALIAS && !DIRECT) {
      if (j == 0) read_a2();
    }
    constexpr int BG = (CS <= 4 && (HAS_C2 || WPS == 1)) ? CS : 2;   // slices of filter fragments in flight (all of them up to CS = 4, registers permitting)
    f16x8 bh[2][BG][2], bl[2][BG][2];                            // [buffer][slice in group][k-half]
    auto read_b2 = [&](int buf, int g) {
#pragma unroll
      for (int q = 0; q < BG; ++q)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          frag_pair(b2base + (g * BG + q) * 4096, s, bh[buf][q][s], bl[buf][q][s]);
        }
    };
    read_b2(0, 0);
    // conv1' fragments of this chunk (W1DB: slice j landed with filter group j): requested behind the phase-2 operands,
    // they arrive under the phase-2 MFMAs and phase 3 starts with only its two T3 fragments per k-half to wait for
    f16x8 dh[2][TN3A], dl[2][TN3A];                              // [k-half][column tile]
    if constexpr (W1PRE) {
      const char* w1b = lds + W1B_OFF + (j & 1) * (CN * ROWB);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < TN3; ++t) {
          frag_pair(w1b + (t * 32 + l31) * ROWB, s, dh[s][t], dl[s][t]);
        }
      __builtin_amdgcn_sched_barrier(0);
    }
    f32x16 acc2;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc2[e] = 0.f;
    fcp_static_for<0, CS / BG>([&](auto gc) {
      constexpr int g = decltype(gc)::value;
      if constexpr (g + 1 < CS / BG) read_b2((g + 1) & 1, g + 1);  // next group's fragments under this group's MFMAs
      fcp_static_for<0, 2 * BG>([&](auto tc) {
        constexpr int q = decltype(tc)::value / 2, s = decltype(tc)::value % 2, sl = g * BG + q, trip = 2 * sl + s;
        mfma3(acc2, ah[sl][s], al[sl][s], bh[g & 1][q][s], bl[g & 1][q][s]);
        constexpr int PER = (NDMA + 2 * CS - 1) / (2 * CS);       // DMA instructions per MFMA triple (1, or 2 where CN > 32 CS)
        if constexpr (SPREAD && trip * PER < NDMA) {
          __builtin_amdgcn_sched_barrier(0);
          if (more) dma_one(std::integral_constant<int, trip * PER>{}, j + 1, (j + 1) & 1);
          if constexpr (PER == 2 && trip * PER + 1 < NDMA) {
            if (more) dma_one(std::integral_constant<int, trip * PER + 1>{}, j + 1, (j + 1) & 1);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        static_assert(PER <= 2, "at most two DMA instructions per MFMA triple");
      });
    });
    // ---- acc2 * ws3 + b3 (per lane: one channel) -> the wave's rows of the fp32 tile.  Channel group q of a row is
    //      stored in the two 16-byte pieces the split32 image of that group will occupy (hi piece q ^ sw, lo piece
    //      (4 + q) ^ sw), so the epilogue rewrites each item in place.
    {
      const int q = l31 >> 3;
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const int row = wave * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * half;   // mfma_c_row, spelled out
        const int piece = ((l31 & 4) ? (4 + q) : q) ^ swz(row);
        *reinterpret_cast<float*>(lds + CT_OFF + row * ROWB + (piece << 4) + (l31 & 3) * 4) = conv_scale_bias(acc2[rr], ws_l, b_l);
      }
    }
    // ---- epilogue of conv3 for this chunk (own rows: LDS accesses of one wave execute in order, no barrier):
    //      out = relu(. + x) -> registers (stored in phase 3) and T3 (in place)
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HAS_RES)     // keep the residual's first use HERE: hoisted into phase 2 it would be waited for a phase early
      asm volatile("" : "+v"(rhi[0]), "+v"(rlo[0]), "+v"(rhi[1]), "+v"(rlo[1]));
    u32x4_t ohi[2], olo[2];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int row = erow0 + 16 * it;
      const int sw = swz(row);
      char* crow = lds + CT_OFF + row * ROWB;
      const f32x4 a = *reinterpret_cast<const f32x4*>(crow + ((eq ^ sw) << 4));
      const f32x4 b = *reinterpret_cast<const f32x4*>(crow + (((4 + eq) ^ sw) << 4));
      float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
      float r[8];
      if constexpr (HAS_RES) join8(rhi[it], rlo[it], r);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if constexpr (HAS_RES) v[e] = conv_finish_relu(v[e], r[e]);
        else v[e] = conv_finish_relu(v[e]);
      }
      split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, ohi[it], olo[it]);
      if constexpr (HAS_P3) {                                      // ... and T3, conv1's operand (the expand form has no phase 3)
        *reinterpret_cast<u32x4_t*>(crow + ((eq ^ sw) << 4)) = ohi[it];
        *reinterpret_cast<u32x4_t*>(crow + (((4 + eq) ^ sw) << 4)) = olo[it];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    if (more) {                                                  // a chunk ahead: the lane's channel constants, the residual
      ws_l = p.ws3[(j + 1) * 32 + l31];
      b_l = p.b3[(j + 1) * 32 + l31];
      load_res(j + 1);
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!W1DB) {                                       // single conv1' buffer: slice j was issued at the top
      if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NCONST + NRES) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    auto store_out = [&]() {
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        const unsigned o = so[it] == 0xFFFFFFFFu ? 0xFFFFFFFFu : so[it] + (unsigned)(j * 128);
        __builtin_amdgcn_raw_buffer_store_b128(ohi[it], rs_out, o, 0, FCP_CHAIN_STORE_AUX);     // aux 2: nt (streamed once)
        __builtin_amdgcn_raw_buffer_store_b128(olo[it], rs_out, o == 0xFFFFFFFFu ? o : o + 64u, 0, FCP_CHAIN_STORE_AUX);
      }
    };
    if constexpr (!HAS_P3) {
      store_out();                                                 // expand form: the chunk ends with its stores
    } else {
    // ---- phase 3: acc3 += T3 . W1'[:, slice j]^T, one k-half at a time (fragment registers: CN = 128 has none to spare);
    //      this chunk's `out` stores go out behind the first k-half's fragment reads
    const char* w1base = lds + W1B_OFF + (W1DB ? (j & 1) * (CN * ROWB) : 0);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      f16x8 ch, cl;
      frag_pair(a3base, s, ch, cl);
      if constexpr (!W1PRE) {
#pragma unroll
        for (int t = 0; t < TN3; ++t) {
          frag_pair(w1base + (t * 32 + l31) * ROWB, s, dh[s][t], dl[s][t]);
        }
      }
      if (s == 0) {
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
        store_out();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int t = 0; t < TN3; ++t) mfma3(acc3[t], ch, cl, dh[s][t], dl[s][t]);
    }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();

  // ================================================================================ conv1' epilogue -> t1' (HBM)
  float* Cs = smem;                                              // fp32 tile [BMT][64], one 64-column half at a time
#pragma unroll
  for (int hh = 0; hh < CN / 64; ++hh) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) {
        const int row = wave * 32 + (rr & 3) + 8 * (rr >> 2) + 4 * half;   // mfma_c_row, spelled out
        Cs[row * 64 + t * 32 + l31] = acc3[CN == 64 ? t : 2 * hh + t][rr];
      }
    __syncthreads();
    const int ccol = (tid & 7) * 8;
    const int co = hh * 64 + ccol;
    float ws8[8], b8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      ws8[e] = p.ws1n[co + e];
      b8[e] = p.b1n[co + e];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = (tid >> 3) + LR * g;
      const long m = pix(row);
      if (m < 0) continue;
      float v[8];
      row_values8(Cs + row * 64 + ccol, ws8, b8, v);
      pack_store8(p.t1n, m, p.t1n_ld, co, 1, p.nt_store, v);
    }
    __syncthreads();
  }
}

template <int CN, int CW, int NOUT, bool HAS_C2, bool HAS_RES, int CW2 = 0>
int launch(const ChainK& k, hipStream_t s) {
  constexpr int LDS = lds_bytes(CW, CN, HAS_C2, direct_form(CN, CW2));
  FCP_LDS_OPT_IN((&bneck_chain_c64<CN, CW, NOUT, HAS_C2, HAS_RES, CW2>), LDS);
  const int tiles = HAS_C2 ? k.n * fcp_cdiv(k.h, BMT / 16) * ((k.w + 15) >> 4) : fcp_cdiv(k.M, BMT);   // conv2 forms: 8 x 16 patches
  hipLaunchKernelGGL((bneck_chain_c64<CN, CW, NOUT, HAS_C2, HAS_RES, CW2>), dim3(tiles), dim3(2 * BMT), LDS, s, k);
  FCP_LAUNCH_OK();
  return 0;
}

// The supported forms, one row each: what the descriptor must say -> the kernel that runs it.  c: all of conv3's input
// channels, cb of them from the second source; cn = 0: no conv1' (engine.chain_supported lists the same rows for callers)
struct ChainForm {
  bool has_c2;
  int c, cb, nout;
  bool residual;
  int cn;
  int (*launch)(const ChainK&, hipStream_t);
};
const ChainForm FORMS[] = {
    // conv2, c, cb, nout, residual, cn
    {true, 64, 0, 256, true, 64, launch<64, 64, 256, true, true>},
    {true, 64, 0, 256, true, 128, launch<128, 64, 256, true, true>},
    {false, 128, 0, 512, true, 128, launch<128, 128, 512, false, true>},
    {false, 128, 0, 256, false, 64, launch<64, 128, 256, false, false>},
    {false, 256, 0, 1024, true, 256, launch<256, 256, 1024, false, true>},
    {false, 128, 0, 512, true, 256, launch<256, 128, 512, false, true>},          // CN = 256: 128 accumulator registers, one wave per SIMD only
    {false, 384, 256, 512, false, 128, launch<128, 384, 512, false, false, 256>},   // two-source pair: [conv2 out 128 | x(::2, ::2) 256] -> 512 -> 128
    {false, 256, 0, 1024, true, 0, launch<0, 256, 1024, false, true>},              // expand form: conv3 256 -> 1024 + identity, no conv1'
};

}  // namespace

extern "C" int fcp_bottleneck_chain_f16x3(const fcp_chain_desc* d, fcp_stream_t stream) {
  FCP_REQUIRE(d != nullptr, "chain: null descriptor");
  const bool has_p3 = d->cn != 0 || d->w1n != nullptr;          // cn = 0 and no conv1' filter: the expand form (conv3 + identity only)
  FCP_REQUIRE(d->t1 && d->w3 && d->ws3 && d->b3 && d->out && (!has_p3 || (d->w1n && d->ws1n && d->b1n && d->t1n)),
              "chain: null pointer (every convolution carries folded-BN bias and filter scales)");
  const bool has_c2 = d->w2 != nullptr;
  FCP_REQUIRE(!has_c2 || (d->ws2 && d->b2), "chain: conv2 needs its scales and bias");
  const int cb = d->t1b ? d->cb : 0;                            // channels of the second source
  const ChainForm* form = nullptr;
  for (const ChainForm& f : FORMS)
    if (f.has_c2 == has_c2 && f.c == d->c && f.cb == cb && f.nout == d->nout && f.residual == (d->res != nullptr) && f.cn == d->cn &&
        (f.cn != 0) == has_p3)
      form = &f;
  FCP_REQUIRE((form && form->cb) || !d->t1b, "chain: a second source (t1b) exists for the two-source pair form only (c 384 = 128 + 256, nout 512, cn 128)");
  FCP_REQUIRE(form != nullptr, "chain: unsupported shape (c %d, conv2 %d, nout %d, residual %d, cn %d)", d->c, (int)has_c2, d->nout,
              d->res != nullptr, d->cn);
  FCP_REQUIRE(d->n > 0 && d->h > 0 && d->w > 0, "chain: bad sizes");
  const long M = (long)d->n * d->h * d->w;
  FCP_REQUIRE(M < (1L << 31), "chain: too many pixels");
  auto aligned = [](const void* p, int ld) { return ((uintptr_t)p & 127) == 0 && ld % 32 == 0; };
  FCP_REQUIRE(aligned(d->t1, d->t1_ld) && (!d->res || aligned(d->res, d->res_ld)) && aligned(d->out, d->out_ld) && (!has_p3 || aligned(d->t1n, d->t1n_ld)),
              "chain: tensors are split32 views: 128-byte aligned, channel stride a multiple of 32");
  FCP_REQUIRE(d->t1_ld >= d->c - cb && (!d->res || d->res_ld >= d->nout) && d->out_ld >= d->nout && (!has_p3 || d->t1n_ld >= d->cn), "chain: channel strides too small");
  const unsigned long t1_bytes = (unsigned long)M * d->t1_ld * 4ul;
  FCP_REQUIRE(t1_bytes < 0xFFFFFFF0ul, "chain: t1 must be below 4 GiB");
  ChainK k;
  k.t1 = d->t1; k.t1_bytes = (unsigned)t1_bytes; k.t1_ld = d->t1_ld;
  k.w2 = reinterpret_cast<const float*>(d->w2); k.w2_bytes = 128u * 9 * 64 * 4; k.ws2 = d->ws2; k.b2 = d->b2;
  k.w3 = reinterpret_cast<const float*>(d->w3); k.w3_bytes = (unsigned)(d->nout * d->c * 4); k.ws3 = d->ws3; k.b3 = d->b3;
  k.res = d->res; k.res_ld = d->res_ld; k.out = d->out; k.out_ld = d->out_ld;
  const unsigned long out_bytes = (unsigned long)M * d->out_ld * 4ul;
  FCP_REQUIRE(out_bytes < 0xFFFFFFF0ul, "chain: out must span less than 4 GiB");
  k.out_bytes = (unsigned)out_bytes;
  k.w1n = reinterpret_cast<const float*>(d->w1n); k.w1n_bytes = has_p3 ? (unsigned)(fcp_cdiv(d->cn, 128) * 128 * d->nout * 4) : 0u; k.ws1n = d->ws1n; k.b1n = d->b1n;
  k.t1n = d->t1n; k.t1n_ld = d->t1n_ld;
  k.n = d->n; k.h = d->h; k.w = d->w; k.M = (int)M;
  static const int nt_env = getenv("FCP_NT_STORE") ? atoi(getenv("FCP_NT_STORE")) : 1;
  k.nt_store = nt_env;
  k.t1b = nullptr; k.t1b_bytes = 0; k.t1b_ld = 0; k.hb = 0; k.wb = 0; k.sb = 1;
  if (d->t1b) {
    FCP_REQUIRE(aligned(d->t1b, d->t1b_ld) && d->t1b_ld >= d->cb && d->t1b_stride >= 1 && d->t1b_h > 0 && d->t1b_w > 0 &&
                (long)(d->h - 1) * d->t1b_stride < d->t1b_h && (long)(d->w - 1) * d->t1b_stride < d->t1b_w,
                "chain: t1b must be a split32 view whose (h, w) grid covers the output grid at t1b_stride");
    const unsigned long tb = (unsigned long)d->n * d->t1b_h * d->t1b_w * d->t1b_ld * 4ul;
    FCP_REQUIRE(tb < 0xFFFFFFF0ul, "chain: t1b must be below 4 GiB");
    k.t1b = d->t1b; k.t1b_bytes = (unsigned)tb; k.t1b_ld = d->t1b_ld; k.hb = d->t1b_h; k.wb = d->t1b_w; k.sb = d->t1b_stride;
  }
  k.out_even = (d->flags & FCP_CHAIN_OUT_EVEN_ONLY) ? 1 : 0;
  FCP_REQUIRE(!k.out_even || has_c2, "chain: FCP_CHAIN_OUT_EVEN_ONLY needs a conv2 form");
  hipStream_t s = (hipStream_t)stream;
  // d->tile_m is a hint this library ignores: the conv2 forms run on 8 x 16 patches, the others on 128-pixel tiles
  return form->launch(k, s);
}
