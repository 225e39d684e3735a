// The gray of an RGB pixel, OpenCV's 8-bit RGB2GRAY: the guide of fcp_matte_refine.hip and the patch plane of
// fcp_nlm.hip.  It is the gray of min_sharpness as well; fcp_sharpness.hip states it itself, where
// tests/test_matte_refine_cpu.py reads it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fcp_gray {

__device__ __forceinline__ uint32_t gray_of(uint32_t r, uint32_t g, uint32_t b) {
  return (9798u * r + 19235u * g + 3735u * b + 16384u) >> 15;       // at most (32768 * 255 + 16384) >> 15 = 255
}

}  // namespace fcp_gray
