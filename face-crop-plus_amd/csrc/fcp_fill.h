// Where the fill of a composite comes from: what fcp_matte.hip's matte_kernel and fcp_cutout.hip's cutout_cols_kernel put
// behind the subject, as a template parameter of the one kernel (INTEGRATION.md sections 2g, 2n and 2r).  A source
// travels in the kernel's argument block; on the device fill.face(f, h, w) is the fill of the workgroup's face, and
// face.group(p, npx) that of a lane's group of npx pixels at pixel p of the face (p = y w + x), whose byte k (pixel
// k / 3, channel k % 3, fcp_crop_bytes.h's order) is group.byte(k).
//
//   Colour  : one colour for every pixel of every face (packed_fill's dword); nothing is read.
//   Picture : the face's picture of a bank (k, h, w, 3) uint8 that is resident on the device, chosen by picks (f,) int32.
//             The 12 bytes of a group are read with load_rgb by the rules of fcp_crop_bytes.h: rows are 3 w bytes at any
//             byte offset, and no dword is read that holds no byte of the bank.  The pick is the same for the whole
//             workgroup (a scalar load) and is clamped to 0 .. k - 1 here, so that a caller of the C entry who breaks
//             the precondition still reads inside the bank.  The bank is never written: it is __restrict__.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fcp_crop_bytes.h"

namespace fcp_fill {

constexpr int kMaxPictures = 4096;      // of a bank

struct Colour {
  uint32_t rgb;
  struct Group {
    uint32_t rgb;
    __device__ __forceinline__ uint32_t byte(int k) const { return (rgb >> (8 * (k % 3))) & 255u; }
  };
  struct Face {
    uint32_t rgb;
    __device__ __forceinline__ Group group(size_t, int) const { return {rgb}; }
  };
  __device__ __forceinline__ Face face(int, int, int) const { return {rgb}; }
};

struct Picture {
  const uint8_t* __restrict__ bank;
  const int32_t* __restrict__ picks;
  int k;
  struct Group {
    uint32_t b[3];
    __device__ __forceinline__ uint32_t byte(int k) const { return (b[k >> 2] >> (8 * (k & 3))) & 255u; }
  };
  struct Face {
    const uint8_t* __restrict__ picture;
    __device__ __forceinline__ Group group(size_t p, int npx) const {
      Group g;
      fcp_crop_bytes::load_rgb(picture + p * 3, npx, g.b);
      return g;
    }
  };
  __device__ __forceinline__ Face face(int f, int h, int w) const {
    const int pick = min(max(picks[f], 0), k - 1);
    return {bank + (size_t)pick * h * w * 3};
  }
};

}  // namespace fcp_fill
