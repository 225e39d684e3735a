// A lane's group of up to four pixels of a uint8 crop row: how fcp_sharpness.hip, fcp_matte.hip, fcp_matte_blur.hip and
// fcp_clahe.hip move crop, label and alpha bytes.  Rows are 3 w (RGB) or w (labels, alpha) bytes and start at any byte
// (odd widths, offset views), so a group starts at any byte too.  The contract, which the guard-byte and offset-view
// tests pin:
//  * a load reads the aligned dwords that hold at least one byte of the group, and no other: never a dword (so never a
//    page) that holds no byte of the array;
//  * a store writes dwords when the group is whole (npx == 4) and its address aligned, the group's own bytes otherwise:
//    no byte outside the group is written.
// Byte k of an RGB group (pixel k / 3, channel k % 3) is bits 8 (k & 3) .. of dword k >> 2; what lies past the group's
// last byte in a loaded dword is unspecified.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fcp_crop_bytes {

__device__ __forceinline__ bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// The 3 npx bytes (npx 1..4) at cp as c[0..2]: up to four aligned dwords, funnel-shifted by the skew of cp.
__device__ __forceinline__ void load_rgb(const uint8_t* cp, int npx, uint32_t c[3]) {
  const int skew = (int)(reinterpret_cast<uintptr_t>(cp) & 3), nbytes = skew + 3 * npx;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(cp - skew);
  const uint32_t d0 = p[0];
  const uint32_t d1 = nbytes > 4 ? p[1] : 0u;
  const uint32_t d2 = nbytes > 8 ? p[2] : 0u;
  const uint32_t d3 = nbytes > 12 ? p[3] : 0u;
  const int sh = 8 * skew;
  c[0] = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
  c[1] = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
  c[2] = (uint32_t)((((uint64_t)d3 << 32) | d2) >> sh);
}

// load_rgb with its four loads in flight together: a dword that holds no byte of the group is not skipped by a branch, which
// makes every load wait for the one before it, but replaced by the group's last dword, read again.  The same contract.
__device__ __forceinline__ void load_rgb_together(const uint8_t* cp, int npx, uint32_t c[3]) {
  const int skew = (int)(reinterpret_cast<uintptr_t>(cp) & 3), last = (skew + 3 * npx - 1) >> 2;
  const uint32_t* p = reinterpret_cast<const uint32_t*>(cp - skew);
  const uint32_t d0 = p[0], d1 = p[min(1, last)], d2 = p[min(2, last)], d3 = p[min(3, last)];
  const int sh = 8 * skew;
  c[0] = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh);
  c[1] = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
  c[2] = (uint32_t)((((uint64_t)d3 << 32) | d2) >> sh);
}

// The first 3 npx bytes of o[0..2] to op.
__device__ __forceinline__ void store_rgb(uint8_t* op, int npx, const uint32_t o[3]) {
  if (npx == 4 && aligned4(op)) {
    uint32_t* q = reinterpret_cast<uint32_t*>(op);
    q[0] = o[0];
    q[1] = o[1];
    q[2] = o[2];
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < 3 * npx) op[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
  }
}

// One-byte pixels (labels, alpha): the npx bytes at p as v[0..npx-1], 0 above; and v[0..npx-1] as bytes to p.
__device__ __forceinline__ void load_u8(const uint8_t* p, int npx, uint32_t v[4]) {
  if (npx == 4 && aligned4(p)) {
    const uint32_t d = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (d >> (8 * j)) & 255u;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < npx ? p[j] : 0u;
  }
}

__device__ __forceinline__ void store_u8(uint8_t* p, int npx, const uint32_t v[4]) {
  if (npx == 4 && aligned4(p)) {
    *reinterpret_cast<uint32_t*>(p) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < npx) p[j] = (uint8_t)v[j];
  }
}

}  // namespace fcp_crop_bytes
