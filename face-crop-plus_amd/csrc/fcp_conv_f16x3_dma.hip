// fp16x3 convolution, both operands fed by LDS-DMA.
//
// When the activation tensor is in split32 format, a K slice of a pixel (one filter tap x 32
// channels) is byte-for-byte the 128-byte LDS row image [hi k0..31 | lo k0..31], exactly like a
// row of the offline-split filter.  Both tiles are then moved global -> LDS by
// `buffer_load_dwordx4 ... lds` (1 KiB per wave instruction, out-of-range lanes write zeros = the
// conv's zero padding): no staging registers, no conversion, no ds_write.  The 16-byte chunks of a
// row are XOR-swizzled on the *source* side (lane l of the DMA writes LDS position l & 7, so it
// fetches chunk (l & 7) ^ sw(row)); the fragment reads apply the same involution.
//
// Pipeline (NST LDS stages, one barrier per slice): all fragment reads of slice kt are issued
// first, then the DMA of slice kt+NST-1 (so the compiler never has an LDS read behind a pending
// DMA), then the 24 MFMAs; a vmcnt(0) + s_barrier closes the step.
#include "fcp_conv_common.h"

using namespace fcp_conv;

namespace {

constexpr int NST = 2;   // LDS stages (three were measured slower: they cost an occupancy step)

// EP8: the output or a residual is split32 (cout % 8 == 0): the tile is accumulated transposed (filters x pixels — same bits) and
// the epilogue works from the registers (conv_epilogue_regs); else the pixel-major tile and the staged fp32 epilogue.
template <int BN, bool EP8>
__global__ void __launch_bounds__(256, (BN == 128 ? 2 : 3)) conv_igemm_f16x3_dma(const ConvK p) {
  constexpr int WAVES_N = (BN == 32) ? 1 : 2;
  constexpr int WAVES_M = 4 / WAVES_N;
  constexpr int WTM = BM / WAVES_M;
  constexpr int WTN = BN / WAVES_N;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int A_LD = BM / 32;
  constexpr int B_LD = BN / 32;
  constexpr int ROWB = 128;
  constexpr int STAGE = (BM + BN) * ROWB;

  extern __shared__ __attribute__((aligned(16))) float smem[];
  char* lds = reinterpret_cast<char*>(smem);

  const int logical = xcd_tile_order(gridDim.x, blockIdx.x);
  const int tile_n = logical % p.grid_n;
  const int tile_m = logical / p.grid_n;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int lrow = tid >> 3;                                     // 0..31 (+32 i)
  const int csrc = (tid & 7) ^ (((lrow >> 1) & 7) ^ ((lrow & 1) << 2));   // source chunk of LDS position tid & 7

  const int hw = p.out_h * p.out_w;
  __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, p.in_bytes, 0x00020000);
  __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, p.w_bytes, 0x00020000);
  // optional second source (1x1 convs): channels >= csplit come from in2 sampled at stride2
  __amdgpu_buffer_rsrc_t rs_in2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in2 ? p.in2 : p.in), 0, p.in2_bytes, 0x00020000);
  RowPiece pc[A_LD];
  unsigned base2[A_LD], rowoff[A_LD], woff[B_LD];
#pragma unroll
  for (int i = 0; i < A_LD; ++i) {
    const ConvRow r = conv_row(p, tile_m * BM + lrow + 32 * i, p.M, hw, (unsigned)(csrc * 4));
    pc[i] = make_row_piece<false>(p, r, 0, (unsigned)(csrc * 4));
    base2[i] = r.base2;
  }
#pragma unroll
  for (int i = 0; i < B_LD; ++i) woff[i] = (unsigned)(((tile_n * BN + lrow + 32 * i) * p.wrow + csrc * 4) * 4);
  TapWalk tw;
  auto dma = [&](int kt, int stage) {    // slice kt (the walk is at it) -> LDS stage
    char* a = lds + stage * STAGE + wave_u * 8 * ROWB;
    dma_slice<32>(p, rs_in, rs_in2, rs_w, a, a + BM * ROWB, rowoff, base2, woff, tw.c0, kt);
  };

  f32x16 acc[TM][TN];
  clear_acc(acc);

  const int aoff = (wm * WTM + (lane & 31)) * ROWB;
  const int boff = BM * ROWB + (wn * WTN + (lane & 31)) * ROWB;
  int offH[2], offL[2];
  frag_offsets(lane, offH, offL);

  set_tap<false, true>(p, tw, pc, rowoff);
  dma(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  int stage = 0;
  const int kt_end = p.ktiles;
  for (int kt = 0; kt < kt_end; ++kt) {
    const char* Ab = lds + stage * STAGE + aoff;
    const char* Bb = lds + stage * STAGE + boff;
    f16x8 ah[2][TM], al[2][TM], bh[2][TN], bl[2][TN];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        ah[s][i] = *reinterpret_cast<const f16x8*>(Ab + i * 32 * ROWB + offH[s]);
        al[s][i] = *reinterpret_cast<const f16x8*>(Ab + i * 32 * ROWB + offL[s]);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        bh[s][j] = *reinterpret_cast<const f16x8*>(Bb + j * 32 * ROWB + offH[s]);
        bl[s][j] = *reinterpret_cast<const f16x8*>(Bb + j * 32 * ROWB + offL[s]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // fragments are in registers
    __builtin_amdgcn_sched_barrier(0);
    const int ahead = kt + NST - 1;
    const bool issue = ahead < p.ktiles;
    if (issue) {
      next_tap<false, true>(p, tw, pc, rowoff);
      int st = stage + NST - 1;
      if (st >= NST) st -= NST;
      dma(ahead, st);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if constexpr (EP8) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s][j], al[s][i], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl[s][j], ah[s][i], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh[s][j], ah[s][i], acc[i][j], 0, 0, 0);
          } else {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[s][i], bh[s][j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s][i], bl[s][j], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[s][i], bh[s][j], acc[i][j], 0, 0, 0);
          }
        }
    __builtin_amdgcn_sched_barrier(0);   // keep the waits below behind the MFMAs ("memory" does not order MFMAs)
    // slice kt+1 must have landed before anyone reads it
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (++stage >= NST) stage = 0;
  }

  if constexpr (EP8) {
    const int m_end = (tile_m + 1) * BM < p.M ? (tile_m + 1) * BM : p.M;
    conv_epilogue_regs<TM, TN, WTM, WTN>(p, acc, tile_m * BM, m_end, TM, tile_n * BN, (tile_n + 1) * BN < p.cout ? (tile_n + 1) * BN : p.cout,
                                         wm, wn, lane, hw);
  } else {
    conv_epilogue<BN, TM, TN, WTM, WTN>(p, acc, smem, tile_m, tile_n, tid, lane, wm, wn, hw);
  }
}

template <int BN, bool EP8>
int launch_ep(const ConvK& k, hipStream_t s) {
  size_t lds = (size_t)NST * (BM + BN) * 128;
  const size_t epi = EP8 ? 0 : (size_t)BM * BN * 4;       // the staged epilogue's C tile
  if (lds < epi) lds = epi;
  FCP_LDS_OPT_IN((&conv_igemm_f16x3_dma<BN, EP8>), lds);
  hipLaunchKernelGGL((conv_igemm_f16x3_dma<BN, EP8>), dim3(k.grid_m * k.grid_n), dim3(256), lds, s, k);
  FCP_LAUNCH_OK();
  return 0;
}
template <int BN>
int launch(const ConvK& k, hipStream_t s) {
  const bool ep8 = (k.out_fmt | k.res1_fmt | k.res2_fmt) != 0;
  return ep8 ? launch_ep<BN, true>(k, s) : launch_ep<BN, false>(k, s);
}

}  // namespace

namespace fcp_conv {

int launch_f16x3_dma(const ConvK& k, int tile_n, hipStream_t s) {
  switch (tile_n) {
    case 32: return launch<32>(k, s);
    case 64: return launch<64>(k, s);
    default: return launch<128>(k, s);
  }
}

}  // namespace fcp_conv
