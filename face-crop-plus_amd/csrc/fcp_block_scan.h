// Exclusive scan of one 32-bit value per lane over a workgroup of THREADS lanes (a multiple of 64), once for the bit
// packers of fcp_jpeg.hip and fcp_png.hip: a shuffle scan inside every wave, the waves' sums through LDS.  Every lane of
// the workgroup must call it (two barriers); wave_sums holds THREADS / 64 words and may be reused by the next call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

// Returns the sum of v over the lanes before this one; *total (same for every lane) is the sum over the workgroup.
template <int THREADS>
__device__ __forceinline__ uint32_t fcp_block_exclusive_scan(uint32_t v, uint32_t* wave_sums, uint32_t* total) {
  uint32_t incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(incl, off, 64);
    if ((threadIdx.x & 63) >= off) incl += up;
  }
  __syncthreads();                                             // wave_sums may still be read from the round before
  if ((threadIdx.x & 63) == 63) wave_sums[threadIdx.x >> 6] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < THREADS / 64; ++k) {
    if (k < (int)(threadIdx.x >> 6)) before += wave_sums[k];
    all += wave_sums[k];
  }
  *total = all;
  return before + incl - v;
}
