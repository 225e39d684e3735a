// Interpolation tables of cv::warpAffine(INTER_CUBIC / INTER_LANCZOS4) on 8-bit images, restated from the published
// imgproc/src/imgwarp.cpp (initInterTab1D / initInterTab2D with fixpt = true), not pinned against a build.
//
//   1-D: 32 fractions x = i * (1.f/32) (float32), K coefficients each:
//     cubic      interpolateCubic, A = -0.75, float32 one operation at a time;
//     lanczos4   interpolateLanczos4: s0, c0 = sin, cos of -(x+3)*pi/4 (double), coeff[i] = (cs[i][0]*s0 + cs[i][1]*c0)
//                / (y*y) with y = -(x+3-i)*pi/4, 1e30f at the zero of the kernel, normalised by 1/sum in float32.
//   2-D: w[k1][k2] = saturate_short(round_half_even(float(ty[k1]*tx[k2]) * 32768.f)); when the K*K weights do not sum to
//     32768, the difference is taken off (diff > 0) the smallest or given to (diff < 0) the largest entry of the 2x2
//     block at rows / columns K/2, K/2+1 (first strict extreme in row-major order, starting at (K/2, K/2)).
//
// The 1-D tables are built on the host only (glibc sin / cos for Lanczos), so they do not depend on a device libm; the
// 2-D weights are rebuilt per pixel on the device from the same floats with interp_weights_2d, which is also what the
// host export fcp_warp_interp_weights runs.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FCP_HD __host__ __device__
#else
#define FCP_HD
#endif

namespace fcp_interp {

constexpr int TAB = 32;            // INTER_TAB_SIZE
constexpr int ONE = 1 << 15;       // INTER_REMAP_COEF_SCALE

// The float 1-D table of one method, passed to the kernels by value (512 B for cubic, 1 KiB for Lanczos-4).
template <int K>
struct Tab1D {
  float c[TAB * K];
};

// cv2.INTER_CUBIC = 2, cv2.INTER_LANCZOS4 = 4 -> taps per axis, 0 for anything else.
inline int taps_of(int interp) { return interp == 2 ? 4 : (interp == 4 ? 8 : 0); }

// interpolateCubic(x, coeffs), float32 operation by operation.
inline void cubic_coeffs(float x, float* c) {
  const float A = -0.75f;
  c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
  c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
  c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
  c[3] = 1.f - c[0] - c[1] - c[2];
}

// interpolateLanczos4(x, coeffs).
inline void lanczos4_coeffs(float x, float* c) {
  const double s45 = 0.70710678118654752440084436210485;
  const double cs[8][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
  const double pi = 3.1415926535897932384626433832795;
  float sum = 0;
  const double y0 = -(x + 3) * pi * 0.25, s0 = sin(y0), c0 = cos(y0);
  for (int i = 0; i < 8; ++i) {
    const float t = x + 3 - i;
    if (t >= 1e-6f || t <= -1e-6f) {
      const double y = -t * pi * 0.25;
      c[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
    } else {
      c[i] = 1e30f;
    }
    sum += c[i];
  }
  sum = 1.f / sum;
  for (int i = 0; i < 8; ++i) c[i] *= sum;
}

// initInterTab1D for K = 4 (cubic) or 8 (Lanczos-4).
template <int K>
inline void build_tab1d(Tab1D<K>& t) {
  const float scale = 1.f / TAB;
  for (int i = 0; i < TAB; ++i) {
    if (K == 4) cubic_coeffs(i * scale, t.c + i * K);
    else lanczos4_coeffs(i * scale, t.c + i * K);
  }
}

// The fixed-point K x K weights of one (fy, fx) pair from the 1-D rows ty = tab[fy], tx = tab[fx], row-major into w.
// Static indices only, so that a kernel keeps w in registers.
template <int K>
FCP_HD inline void interp_weights_2d(const float* ty, const float* tx, int* w) {
  int isum = 0;
#pragma unroll
  for (int k1 = 0; k1 < K; ++k1) {
#pragma unroll
    for (int k2 = 0; k2 < K; ++k2) {
      const float v = (ty[k1] * tx[k2]) * 32768.f;
      const float r = rintf(v);                              // cvRound: round half to even
      const int iv = r < -32768.f ? -32768 : (r > 32767.f ? 32767 : (int)r);
      w[k1 * K + k2] = iv;
      isum += iv;
    }
  }
  const int diff = isum - ONE;
  constexpr int h = K / 2;
  int mn = 0, mx = 0, vmn = w[h * K + h], vmx = vmn;          // positions 0..3 of the 2x2 block, row-major
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int v = w[(h + r / 2) * K + h + r % 2];
    if (v < vmn) { vmn = v; mn = r; }
    else if (v > vmx) { vmx = v; mx = r; }
  }
  const int at = diff < 0 ? mx : mn;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int& e = w[(h + r / 2) * K + h + r % 2];
    if (diff != 0 && r == at) e = (int16_t)(e - diff);
  }
}

}  // namespace fcp_interp
