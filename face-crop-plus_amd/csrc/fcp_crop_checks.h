// The argument checks that the entry points of the crop post-processing kernels share (fcp_matte.hip, fcp_matte_blur.hip,
// fcp_cutout.hip, fcp_matte_refine.hip, fcp_subject.hip), host side.  Each sets the error under the entry point's name
// `who` and returns FCP_ERR_ARG, or 0; an entry point calls them through FCP_CHECK in the order it refuses.
#pragma once
#include <cstdint>

#include "fcp_common.h"
#include "fcp_feather.h"
#include "fcp_fill.h"

#define FCP_CHECK(expr)              \
  do {                               \
    if (int _rc = (expr)) return _rc; \
  } while (0)

namespace fcp_crop_checks {

using fcp_feather::kClasses;
using fcp_feather::kMaxSide;

// f h w bytes_per_pixel of a workspace, -1 for sizes that check_sizes refuses
inline int64_t workspace_bytes(int f, int h, int w, int64_t bytes_per_pixel) {
  if (f < 0 || f > 65535 || h < 1 || w < 1 || h > kMaxSide || w > kMaxSide) return -1;
  return (int64_t)f * h * w * bytes_per_pixel;
}

inline int check_sizes(const char* who, int f, int h, int w) {
  FCP_REQUIRE(f >= 0 && h >= 1 && w >= 1, "%s: bad sizes (f %d, h %d, w %d)", who, f, h, w);
  FCP_REQUIRE(h <= kMaxSide && w <= kMaxSide, "%s: crops of at most %d x %d px (got h %d, w %d)", who, kMaxSide, kMaxSide, h, w);
  FCP_REQUIRE(f <= 65535, "%s: at most 65535 crops per call (got %d)", who, f);
  return 0;
}

inline int check_fill(const char* who, int r, int g, int b) {
  FCP_REQUIRE(r >= 0 && r <= 255 && g >= 0 && g <= 255 && b >= 0 && b <= 255, "%s: fill components must be 0..255 (got %d, %d, %d)",
              who, r, g, b);
  return 0;
}

inline int check_class_bits(const char* who, uint32_t class_bits) {
  FCP_REQUIRE((class_bits >> kClasses) == 0, "%s: class_bits 0x%x names a class at or above %d", who, class_bits, kClasses);
  return 0;
}

inline int check_feather(const char* who, int feather) {
  FCP_REQUIRE(feather == 0 || feather == 3 || feather == 5 || feather == 7, "%s: feather must be 0, 3, 5 or 7 (got %d)", who, feather);
  return 0;
}

// k pictures of a bank (fcp_fill.h's Picture)
inline int check_pictures(const char* who, int k) {
  FCP_REQUIRE(k >= 1 && k <= fcp_fill::kMaxPictures, "%s: a bank of 1..%d pictures (got k %d)", who, fcp_fill::kMaxPictures, k);
  return 0;
}

// the caller's workspace of at least `need` bytes (an entry point's own fcp_*_workspace_bytes)
inline int check_workspace(const char* who, const void* workspace, int64_t workspace_bytes, int64_t need) {
  FCP_REQUIRE(workspace != nullptr && workspace_bytes >= need, "%s: the workspace needs %lld bytes (got %lld)", who, (long long)need,
              (long long)workspace_bytes);
  FCP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
  return 0;
}

inline uint32_t packed_fill(int r, int g, int b) { return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16); }

}  // namespace fcp_crop_checks
