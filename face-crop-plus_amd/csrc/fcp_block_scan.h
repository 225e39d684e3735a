// Exclusive scan and sum of one value per lane over a workgroup of THREADS lanes (a multiple of 64), once for the bit
// packers of fcp_jpeg.hip and fcp_png.hip: shuffles inside every wave, the waves' sums through LDS.  Every lane of the
// workgroup must call them (two barriers); the LDS array holds THREADS / 64 values and may be reused by the next call.
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

// Returns the sum of v over the workgroup (same for every lane).
template <int THREADS, typename T>
__device__ __forceinline__ T fcp_block_sum(T v, T* wave_sums) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();                                             // wave_sums may still be read from the round before
  if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
  __syncthreads();
  T all = 0;
#pragma unroll
  for (int k = 0; k < THREADS / 64; ++k) all += wave_sums[k];
  return all;
}
