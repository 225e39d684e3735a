// cv2.resize(INTER_AREA, uint8) of one destination pixel: the arithmetic of the batch builder (fcp_batch.hip) and of the
// ragged level builder (fcp_pyramid.hip).  Restates the portable C++ path of cv::resize (imgproc/resize.cpp), scales >= 1:
//  * both scales integral (|scale - round(scale)| < DBL_EPSILON): box sums, (s+2)>>2 for 2x2 (ResizeAreaFastVec), else
//    cvRound(float(sum) * (1.f/area)) (resizeAreaFast_Invoker);
//  * otherwise computeResizeAreaTab's float32 alpha tables (evaluated in double, per thread) with the row accumulation and
//    the column accumulation in float32, table order, cvRound (ResizeArea_Invoker).
// The including translation unit is built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

namespace fcp_area {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint8_t sat_u8(int v) { return (uint8_t)clampi(v, 0, 255); }

// One destination index of computeResizeAreaTab: entries are
//   [sx1-1 : a_first] (if has_first), [sx1 .. sx2-1 : a_mid], [sx2 : a_last] (if has_last).
struct AreaCell {
  int sx1, sx2;
  float a_first, a_mid, a_last;
  bool has_first, has_last;
};

__device__ __forceinline__ AreaCell area_cell(int d, double scale, int ssize) {
  AreaCell c;
  const double fsx1 = d * scale;
  const double fsx2 = fsx1 + scale;
  const double cell = fmin(scale, ssize - fsx1);
  int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
  sx2 = min(sx2, ssize - 1);
  sx1 = min(sx1, sx2);
  c.sx1 = sx1;
  c.sx2 = sx2;
  c.has_first = sx1 - fsx1 > 1e-3;
  c.a_first = (float)((sx1 - fsx1) / cell);
  c.a_mid = (float)(1.0 / cell);
  c.has_last = fsx2 - sx2 > 1e-3;
  c.a_last = (float)(fmin(fmin(fsx2 - sx2, 1.), cell) / cell);
  return c;
}

__device__ __forceinline__ int cell_count(const AreaCell& c) {
  return (c.has_first ? 1 : 0) + (c.sx2 - c.sx1) + (c.has_last ? 1 : 0);
}
__device__ __forceinline__ void cell_entry(const AreaCell& c, int j, int& si, float& a) {
  if (c.has_first) {
    if (j == 0) { si = c.sx1 - 1; a = c.a_first; return; }
    --j;
  }
  if (j < c.sx2 - c.sx1) { si = c.sx1 + j; a = c.a_mid; return; }
  si = c.sx2; a = c.a_last;
}

// Destination pixel (dx, dy) of INTER_AREA from the (sh, sw, 3) image S to (dh, dw); scale_x = 1. / ((double)dw / sw)
// and scale_y likewise, both >= 1.  Writes the three channels to o[0..2].
__device__ __forceinline__ void area_pixel(const uint8_t* __restrict__ S, int sh, int sw, double scale_x, double scale_y,
                                           int dx, int dy, uint8_t* o) {
  const int isx = (int)rint(scale_x), isy = (int)rint(scale_y);
  if (fabs(scale_x - isx) < DBL_EPSILON && fabs(scale_y - isy) < DBL_EPSILON) {
    int sum[3] = {0, 0, 0};
    for (int yy = 0; yy < isy; ++yy) {
      const uint8_t* p = S + ((long)(dy * isy + yy) * sw + (long)dx * isx) * 3;
      for (int xx = 0; xx < isx; ++xx, p += 3) { sum[0] += p[0]; sum[1] += p[1]; sum[2] += p[2]; }
    }
    if (isx == 2 && isy == 2) {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (uint8_t)((sum[c] + 2) >> 2);
    } else {
      const float inv_area = __fdiv_rn(1.f, (float)(isx * isy));
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = sat_u8((int)rintf((float)sum[c] * inv_area));
    }
    return;
  }
  const AreaCell cx = area_cell(dx, scale_x, sw), cy = area_cell(dy, scale_y, sh);
  const int nx = cell_count(cx), ny = cell_count(cy);
  float sum[3] = {0.f, 0.f, 0.f};
  for (int k = 0; k < ny; ++k) {
    int sy; float beta;
    cell_entry(cy, k, sy, beta);
    const uint8_t* row = S + (long)sy * sw * 3;
    float buf[3] = {0.f, 0.f, 0.f};
    for (int j = 0; j < nx; ++j) {
      int sx; float alpha;
      cell_entry(cx, j, sx, alpha);
      const uint8_t* p = row + sx * 3;
      buf[0] = buf[0] + (float)p[0] * alpha;
      buf[1] = buf[1] + (float)p[1] * alpha;
      buf[2] = buf[2] + (float)p[2] * alpha;
    }
    if (k == 0) {
      sum[0] = beta * buf[0]; sum[1] = beta * buf[1]; sum[2] = beta * buf[2];
    } else {
      sum[0] += beta * buf[0]; sum[1] += beta * buf[1]; sum[2] += beta * buf[2];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = sat_u8((int)rintf(sum[c]));
}

}  // namespace fcp_area
