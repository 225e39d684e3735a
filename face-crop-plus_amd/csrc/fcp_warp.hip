// 5-point transform estimation + OpenCV-exact bilinear warpAffine (uint8, 3ch).
//
// estimate: cv2.estimateAffinePartial2D / estimateAffine2D with
// ransacReprojThreshold=inf accept the first minimal sample as all-inlier and
// then refine on all points (10 LM iterations on a *linear* residual), i.e. they
// return the linear least-squares similarity / affine; computed here in closed
// form in float64, one lane per face.
//
// warp: restatement of cv::warpAffine's fixed-point path (imgwarp.cpp):
// inverse map in double, AB_BITS=10, round_delta=16, INTER_BITS=5, bilinear
// weights = (32-fy)(32-fx)*32 etc. (sum 32768), out = (sum + 16384) >> 15,
// borders through cv::borderInterpolate.  Built with -ffp-contract=off so the
// double expressions round exactly like the scalar C++ they restate.
//
// warp (float family, opt-in): the float32 SIMD linear warp of newer OpenCV
// builds — same inverse map rounded to float, sx = x*m0 + (y*m1 + m2) and the
// bilinear blend in separately rounded float32 ops, rintf to uint8.
//
// warp (INTER_CUBIC / INTER_LANCZOS4, opt-in): the same coordinates as the fixed-point linear warp, a K x K neighbourhood
// (K = 4 / 8) starting K/2 - 1 pixels before the tap, int16 weights from fcp_interp.h, out = (sum + 16384) >> 15
// saturated to 0..255 (remapBicubic / remapLanczos4).
#include "fcp_common.h"
#include "fcp_hip.h"
#include "fcp_interp.h"

namespace {

__device__ __forceinline__ bool estimate_one(const float* __restrict__ src, const float* __restrict__ dst, int i, int k,
                                             int allow_skew, bool is_live, double* __restrict__ mat, int* __restrict__ ok);

__global__ void __launch_bounds__(64) estimate_transform_kernel(const float* __restrict__ src,
                                                                const float* __restrict__ dst, int f, int k,
                                                                int allow_skew, double* __restrict__ mat,
                                                                int* __restrict__ ok,
                                                                const int* __restrict__ face_count,
                                                                long long* __restrict__ valid_total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int live = face_count != nullptr ? min(*face_count, f) : f;   // rows >= live are padding of a fixed-size batch
  bool counted = false;
  if (i < f) counted = estimate_one(src, dst, i, k, allow_skew, i < live, mat, ok);
  if (valid_total != nullptr) {                                        // whole wave gets here: one atomic per wave
    const unsigned long long votes = __ballot(counted);
    if ((threadIdx.x & 63) == 0 && votes != 0ull) atomicAdd(reinterpret_cast<unsigned long long*>(valid_total), (unsigned long long)__popcll(votes));
  }
}

// One face: returns whether it is a valid (live, non-degenerate) face; writes its matrix and ok flag.
__device__ __forceinline__ bool estimate_one(const float* __restrict__ src, const float* __restrict__ dst, int i, int k,
                                             int allow_skew, bool is_live, double* __restrict__ mat, int* __restrict__ ok) {
  const float* s = src + (long)i * k * 2;
  bool finite = is_live;
  double mx = 0, my = 0, MX = 0, MY = 0;
  for (int p = 0; p < k; ++p) {
    const double x = s[2 * p], y = s[2 * p + 1];
    finite = finite && isfinite(x) && isfinite(y);
    mx += x; my += y; MX += dst[2 * p]; MY += dst[2 * p + 1];
  }
  mx /= k; my /= k; MX /= k; MY /= k;
  double m[6] = {0, 0, 0, 0, 0, 0};
  bool good = finite;
  if (!allow_skew) {
    // minimise sum |a x - b y + tx - X|^2 + |b x + a y + ty - Y|^2
    double sxx = 0, sa = 0, sb = 0;
    for (int p = 0; p < k; ++p) {
      const double x = s[2 * p] - mx, y = s[2 * p + 1] - my;
      const double X = dst[2 * p] - MX, Y = dst[2 * p + 1] - MY;
      sxx += x * x + y * y;
      sa += x * X + y * Y;
      sb += x * Y - y * X;
    }
    good = good && sxx > 0.0;
    if (good) {
      const double a = sa / sxx, b = sb / sxx;
      m[0] = a; m[1] = -b; m[2] = MX - a * mx + b * my;
      m[3] = b; m[4] = a;  m[5] = MY - b * mx - a * my;
    }
  } else {
    // full affine: two independent 2-unknown LSQ problems on centred coordinates
    double sxx = 0, sxy = 0, syy = 0, sxX = 0, syX = 0, sxY = 0, syY = 0;
    for (int p = 0; p < k; ++p) {
      const double x = s[2 * p] - mx, y = s[2 * p + 1] - my;
      const double X = dst[2 * p] - MX, Y = dst[2 * p + 1] - MY;
      sxx += x * x; sxy += x * y; syy += y * y;
      sxX += x * X; syX += y * X; sxY += x * Y; syY += y * Y;
    }
    const double det = sxx * syy - sxy * sxy;
    good = good && fabs(det) > 1e-12 * (sxx * syy + 1e-300);
    if (good) {
      const double a = (sxX * syy - syX * sxy) / det, b = (syX * sxx - sxX * sxy) / det;
      const double c = (sxY * syy - syY * sxy) / det, d = (syY * sxx - sxY * sxy) / det;
      m[0] = a; m[1] = b; m[2] = MX - a * mx - b * my;
      m[3] = c; m[4] = d; m[5] = MY - c * mx - d * my;
    }
  }
  for (int q = 0; q < 6; ++q) good = good && isfinite(m[q]);
  for (int q = 0; q < 6; ++q) mat[(long)i * 6 + q] = good ? m[q] : 0.0;
  ok[i] = good ? 1 : 0;
  return good;
}

// cv::saturate_cast<int>(double) == cvRound (cvtsd2si: nearest-even, 0x80000000 when out of range)
__device__ __forceinline__ int cv_round(double v) {
  if (!(v >= -2147483648.0 && v < 2147483648.0)) return (int)0x80000000;
  return (int)rint(v);
}
__device__ __forceinline__ int sat_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// cv::borderInterpolate; border codes follow cv2.BORDER_*: 0 constant, 1 replicate, 2 reflect, 3 wrap, 4 reflect_101
__device__ __forceinline__ int border_interp(int p, int len, int border) {
  if ((unsigned)p < (unsigned)len) return p;
  if (border == 1) return p < 0 ? 0 : len - 1;
  if (border == 2 || border == 4) {
    const int delta = border == 4;
    if (len == 1) return 0;
    do {
      if (p < 0) p = -p - 1 + delta;
      else p = len - 1 - (p - len) - delta;
    } while ((unsigned)p >= (unsigned)len);
    return p;
  }
  if (border == 3) {
    if (p < 0) p -= ((p - len + 1) / len) * len;
    if (p >= len) p %= len;
    return p;
  }
  return -1;  // constant
}

// Six consecutive bytes (two RGB pixels) at byte offset `off` of `base`: one aligned 12-byte load + a funnel shift
// instead of six byte loads.  The caller guarantees that (off & ~3) + 12 stays inside the allocation.
__device__ __forceinline__ unsigned long long load6(const uint8_t* __restrict__ base, long off) {
  const long a = off & ~3L;
  const unsigned sh = (unsigned)(off & 3) * 8u;
  const unsigned* q = reinterpret_cast<const unsigned*>(base + a);
  const unsigned d0 = q[0], d1 = q[1], d2 = q[2];
  const unsigned long long lo = (unsigned long long)d0 | ((unsigned long long)d1 << 32);
  return sh ? (lo >> sh) | ((unsigned long long)d2 << (64u - sh)) : lo;
}

// Where the source pixels of one face are: first pixel at byte s0off of the source base, sh x sw pixels, rows sstep bytes
// apart; the 12-byte interior loads stay below byte `total` of the base.
struct SrcView {
  long s0off, sstep, total;
  int sh, sw;
};

// Source policy of the batch warp: face -> image img_idx[face] of an (n,h,w,3) batch, un-padded by paddings[img] (t,b,l,r)
// when given (cropper.py:538-539).
struct BatchSource {
  const uint8_t* base;
  int n, h, w;
  const int* img_idx;
  const int* paddings;
  __device__ __forceinline__ void view(int face, SrcView& v) const {
    const int img = img_idx[face];
    int pt = 0, pb = 0, pl = 0, pr = 0;
    if (paddings != nullptr) { pt = paddings[img * 4]; pb = paddings[img * 4 + 1]; pl = paddings[img * 4 + 2]; pr = paddings[img * 4 + 3]; }
    v.sh = h - pt - pb; v.sw = w - pl - pr;
    v.sstep = (long)w * 3;
    v.s0off = ((long)img * h + pt) * v.sstep + (long)pl * 3;
    v.total = (long)n * h * v.sstep;             // bytes of the batch
  }
};

// Source policy of the ragged warp: face -> its own (h,w,3) image at a 64-bit offset of one byte blob of `bytes` bytes
// (descriptors validated by the launcher).
struct RaggedSource {
  const uint8_t* base;
  long bytes;
  const fcp_warp_src* srcs;
  __device__ __forceinline__ void view(int face, SrcView& v) const {
    const fcp_warp_src s = srcs[face];
    v.sh = s.h; v.sw = s.w;
    v.sstep = (long)s.w * 3;
    v.s0off = s.off;
    v.total = bytes;
  }
};

template <int PX, class Src>
__global__ void __launch_bounds__(256) warp_affine_kernel(
    const Src src, const double* __restrict__ mat, const int* __restrict__ ok, int out_h, int out_w, int border,
    uint8_t* __restrict__ out) {
  const int face = blockIdx.y;
  const int groups_per_row = (out_w + PX - 1) / PX;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = g < groups_per_row * out_h;
  const int y = active ? g / groups_per_row : 0;
  const int x0 = active ? (g - y * groups_per_row) * PX : 0;
  uint8_t* dst = out + (((long)face * out_h + y) * out_w + x0) * 3;
  uint8_t px[PX * 3];
#pragma unroll
  for (int q = 0; q < PX * 3; ++q) px[q] = 0;

  const bool valid = ok == nullptr || ok[face] != 0;       // uniform over the workgroup (one face per blockIdx.y)
  // The inverse map is the same for every lane of the workgroup: one lane inverts the forward transform exactly like
  // cv::warpAffine does (two double divisions), the others read it from LDS.
  __shared__ double sM[6];
  if (valid && threadIdx.x == 0) {
    double M[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) M[q] = mat[(long)face * 6 + q];
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
#pragma unroll
    for (int q = 0; q < 6; ++q) sM[q] = M[q];
  }
  __syncthreads();
  if (!active) return;
  if (valid) {
    SrcView v;
    src.view(face, v);
    const uint8_t* __restrict__ images = src.base;
    const int sh = v.sh, sw = v.sw;
    const long sstep = v.sstep, s0off = v.s0off, total = v.total;
    const uint8_t* S0 = images + s0off;
    double M[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) M[q] = sM[q];
    const int X0 = (int)((unsigned)cv_round((M[1] * y + M[2]) * 1024.0) + 16u);
    const int Y0 = (int)((unsigned)cv_round((M[4] * y + M[5]) * 1024.0) + 16u);
    const int width1 = sw - 1 > 0 ? sw - 1 : 0, height1 = sh - 1 > 0 ? sh - 1 : 0;
#pragma unroll
    for (int q = 0; q < PX; ++q) {
      const int x = x0 + q;
      if (x >= out_w) break;
      const int ad = cv_round(M[0] * x * 1024.0), bd = cv_round(M[3] * x * 1024.0);
      const int X = (int)((unsigned)X0 + (unsigned)ad) >> 5;
      const int Y = (int)((unsigned)Y0 + (unsigned)bd) >> 5;
      const int sx = sat_short(X >> 5), sy = sat_short(Y >> 5);
      const int fx = X & 31, fy = Y & 31;
      const int w0 = (32 - fy) * (32 - fx) * 32, w1 = (32 - fy) * fx * 32;
      const int w2 = fy * (32 - fx) * 32, w3 = fy * fx * 32;
      const uint8_t *v0, *v1, *v2, *v3;
      const uint8_t zero[3] = {0, 0, 0};
      if ((unsigned)sx < (unsigned)width1 && (unsigned)sy < (unsigned)height1) {
        const long o0 = s0off + sy * sstep + sx * 3, o1 = o0 + sstep;
        if (((o1 & ~3L) + 12) <= total) {
          // interior: the 2 x 2 neighbourhood is two runs of six bytes — two 12-byte loads instead of twelve byte loads
          const unsigned long long r0 = load6(images, o0), r1 = load6(images, o1);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int a0 = (int)((r0 >> (8 * c)) & 255u), a1 = (int)((r0 >> (8 * c + 24)) & 255u);
            const int a2 = (int)((r1 >> (8 * c)) & 255u), a3 = (int)((r1 >> (8 * c + 24)) & 255u);
            const int acc = a0 * w0 + a1 * w1 + a2 * w2 + a3 * w3;
            const int r = (acc + (1 << 14)) >> 15;
            px[q * 3 + c] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
          }
          continue;
        }
        v0 = images + o0; v1 = v0 + 3; v2 = v0 + sstep; v3 = v2 + 3;
      } else {
        if (border == 0 && (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0)) continue;  // all-constant: 0
        int sx0, sx1, sy0, sy1;
        if (border == 1) {
          sx0 = sx < 0 ? 0 : (sx < sw ? sx : sw - 1);
          sx1 = sx + 1 < 0 ? 0 : (sx + 1 < sw ? sx + 1 : sw - 1);
          sy0 = sy < 0 ? 0 : (sy < sh ? sy : sh - 1);
          sy1 = sy + 1 < 0 ? 0 : (sy + 1 < sh ? sy + 1 : sh - 1);
        } else {
          sx0 = border_interp(sx, sw, border); sx1 = border_interp(sx + 1, sw, border);
          sy0 = border_interp(sy, sh, border); sy1 = border_interp(sy + 1, sh, border);
        }
        v0 = (sx0 >= 0 && sy0 >= 0) ? S0 + sy0 * sstep + sx0 * 3 : zero;
        v1 = (sx1 >= 0 && sy0 >= 0) ? S0 + sy0 * sstep + sx1 * 3 : zero;
        v2 = (sx0 >= 0 && sy1 >= 0) ? S0 + sy1 * sstep + sx0 * 3 : zero;
        v3 = (sx1 >= 0 && sy1 >= 0) ? S0 + sy1 * sstep + sx1 * 3 : zero;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int acc = v0[c] * w0 + v1[c] * w1 + v2[c] * w2 + v3[c] * w3;
        const int r = (acc + (1 << 14)) >> 15;
        px[q * 3 + c] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
      }
    }
  }
  if (PX == 4 && x0 + 4 <= out_w && (out_w & 3) == 0) {
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);  // 12 aligned bytes
    d32[0] = px[0] | (px[1] << 8) | (px[2] << 16) | ((uint32_t)px[3] << 24);
    d32[1] = px[4] | (px[5] << 8) | (px[6] << 16) | ((uint32_t)px[7] << 24);
    d32[2] = px[8] | (px[9] << 8) | (px[10] << 16) | ((uint32_t)px[11] << 24);
  } else {
    for (int q = 0; q < PX && x0 + q < out_w; ++q) {
      dst[q * 3] = px[q * 3]; dst[q * 3 + 1] = px[q * 3 + 1]; dst[q * 3 + 2] = px[q * 3 + 2];
    }
  }
}

// Bilinear blend of the float family: two row lerps, one column lerp, each a separately rounded float32 op (no FMA:
// the library is built with -ffp-contract=off), then round-half-even and saturate to uint8.
__device__ __forceinline__ uint8_t lerp2_f32(float p00, float p01, float p10, float p11, float ax, float ay) {
  const float v0 = p00 + ax * (p01 - p00);
  const float v1 = p10 + ax * (p11 - p10);
  const float v = rintf(v0 + ay * (v1 - v0));
  return (uint8_t)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
}

// The float32 family of cv::warpAffine(INTER_LINEAR) (the SIMD linear warp of newer OpenCV builds): source coordinates and
// bilinear weights in float32, one rounding at the end.  Same launch geometry, un-padding, border handling and stores as
// warp_affine_kernel; only the coordinate / weight arithmetic differs.
template <int PX, class Src>
__global__ void __launch_bounds__(256) warp_affine_float_kernel(
    const Src src, const double* __restrict__ mat, const int* __restrict__ ok, int out_h, int out_w, int border,
    uint8_t* __restrict__ out) {
  const int face = blockIdx.y;
  const int groups_per_row = (out_w + PX - 1) / PX;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = g < groups_per_row * out_h;
  const int y = active ? g / groups_per_row : 0;
  const int x0 = active ? (g - y * groups_per_row) * PX : 0;
  uint8_t* dst = out + (((long)face * out_h + y) * out_w + x0) * 3;
  uint8_t px[PX * 3];
#pragma unroll
  for (int q = 0; q < PX * 3; ++q) px[q] = 0;

  const bool valid = ok == nullptr || ok[face] != 0;       // uniform over the workgroup (one face per blockIdx.y)
  // inverse map in double exactly as warp_affine_kernel, then each coefficient rounded to float once
  __shared__ float sM[6];
  if (valid && threadIdx.x == 0) {
    double M[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) M[q] = mat[(long)face * 6 + q];
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
#pragma unroll
    for (int q = 0; q < 6; ++q) sM[q] = (float)M[q];
  }
  __syncthreads();
  if (!active) return;
  if (valid) {
    SrcView v;
    src.view(face, v);
    const uint8_t* __restrict__ images = src.base;
    const int sh = v.sh, sw = v.sw;
    const long sstep = v.sstep, s0off = v.s0off, total = v.total;
    const uint8_t* S0 = images + s0off;
    const float m0 = sM[0], m1 = sM[1], m2 = sM[2], m3 = sM[3], m4 = sM[4], m5 = sM[5];
    const float fy = (float)y;
    const float bx = fy * m1 + m2, by = fy * m4 + m5;     // the (y*m1 + m2) term of sx = x*m0 + (y*m1 + m2)
    const int width1 = sw - 1 > 0 ? sw - 1 : 0, height1 = sh - 1 > 0 ? sh - 1 : 0;
#pragma unroll
    for (int q = 0; q < PX; ++q) {
      const int x = x0 + q;
      if (x >= out_w) break;
      const float fx = (float)x;
      const float sxf = fx * m0 + bx, syf = fx * m3 + by;
      const float ixf = floorf(sxf), iyf = floorf(syf);
      const float ax = sxf - ixf, ay = syf - iyf;
      // clamped in float before the conversion; the clamped value drives the border logic below
      const int sx = (int)fminf(fmaxf(ixf, -32768.f), 32767.f), sy = (int)fminf(fmaxf(iyf, -32768.f), 32767.f);
      if ((unsigned)sx < (unsigned)width1 && (unsigned)sy < (unsigned)height1) {
        const long o0 = s0off + sy * sstep + sx * 3, o1 = o0 + sstep;
        if (((o1 & ~3L) + 12) <= total) {
          const unsigned long long r0 = load6(images, o0), r1 = load6(images, o1);
#pragma unroll
          for (int c = 0; c < 3; ++c)
            px[q * 3 + c] = lerp2_f32((float)(int)((r0 >> (8 * c)) & 255u), (float)(int)((r0 >> (8 * c + 24)) & 255u),
                                      (float)(int)((r1 >> (8 * c)) & 255u), (float)(int)((r1 >> (8 * c + 24)) & 255u), ax, ay);
          continue;
        }
        const uint8_t* v0 = images + o0;
        const uint8_t* v2 = v0 + sstep;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          px[q * 3 + c] = lerp2_f32(v0[c], v0[3 + c], v2[c], v2[3 + c], ax, ay);
        continue;
      }
      if (border == 0 && (sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0)) continue;  // all-constant: 0
      int sx0, sx1, sy0, sy1;
      if (border == 1) {
        sx0 = sx < 0 ? 0 : (sx < sw ? sx : sw - 1);
        sx1 = sx + 1 < 0 ? 0 : (sx + 1 < sw ? sx + 1 : sw - 1);
        sy0 = sy < 0 ? 0 : (sy < sh ? sy : sh - 1);
        sy1 = sy + 1 < 0 ? 0 : (sy + 1 < sh ? sy + 1 : sh - 1);
      } else {
        sx0 = border_interp(sx, sw, border); sx1 = border_interp(sx + 1, sw, border);
        sy0 = border_interp(sy, sh, border); sy1 = border_interp(sy + 1, sh, border);
      }
      const uint8_t zero[3] = {0, 0, 0};                   // a constant-border tap outside the slice reads 0
      const uint8_t* v0 = (sx0 >= 0 && sy0 >= 0) ? S0 + sy0 * sstep + sx0 * 3 : zero;
      const uint8_t* v1 = (sx1 >= 0 && sy0 >= 0) ? S0 + sy0 * sstep + sx1 * 3 : zero;
      const uint8_t* v2 = (sx0 >= 0 && sy1 >= 0) ? S0 + sy1 * sstep + sx0 * 3 : zero;
      const uint8_t* v3 = (sx1 >= 0 && sy1 >= 0) ? S0 + sy1 * sstep + sx1 * 3 : zero;
#pragma unroll
      for (int c = 0; c < 3; ++c) px[q * 3 + c] = lerp2_f32(v0[c], v1[c], v2[c], v3[c], ax, ay);
    }
  }
  if (PX == 4 && x0 + 4 <= out_w && (out_w & 3) == 0) {
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);  // 12 aligned bytes
    d32[0] = px[0] | (px[1] << 8) | (px[2] << 16) | ((uint32_t)px[3] << 24);
    d32[1] = px[4] | (px[5] << 8) | (px[6] << 16) | ((uint32_t)px[7] << 24);
    d32[2] = px[8] | (px[9] << 8) | (px[10] << 16) | ((uint32_t)px[11] << 24);
  } else {
    for (int q = 0; q < PX && x0 + q < out_w; ++q) {
      dst[q * 3] = px[q * 3]; dst[q * 3 + 1] = px[q * 3 + 1]; dst[q * 3 + 2] = px[q * 3 + 2];
    }
  }
}

// The 3K bytes of K consecutive RGB pixels at byte offset `off` of `base`, realigned into 3K/4 dwords: ND = 3K/4 + 1 aligned
// dwords from (off & ~3), then a byte funnel shift.  The caller guarantees that (off & ~3) + 4 * ND stays inside the
// allocation.
template <int K>
__device__ __forceinline__ void load_taps(const uint8_t* __restrict__ base, long off, unsigned (&e)[3 * K / 4]) {
  constexpr int ND = 3 * K / 4 + 1;
  const unsigned* q = reinterpret_cast<const unsigned*>(base + (off & ~3L));
  const unsigned sh = (unsigned)(off & 3);
  unsigned d[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i) d[i] = q[i];
#pragma unroll
  for (int i = 0; i < ND - 1; ++i) e[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
}

// cv::warpAffine(INTER_CUBIC, K = 4 / INTER_LANCZOS4, K = 8) of uint8 RGB: the fixed-point linear warp's coordinates, launch
// geometry, un-padding, source policies and packed store; the K x K int16 weights of each pixel are rebuilt from the float
// 1-D table (copied to LDS once per workgroup) by fcp_interp::interp_weights_2d, and the taps are summed in int32.
template <int K, int PX, class Src>
__global__ void __launch_bounds__(256) warp_affine_interp_kernel(
    const Src src, const fcp_interp::Tab1D<K> tab, const double* __restrict__ mat, const int* __restrict__ ok, int out_h,
    int out_w, int border, uint8_t* __restrict__ out) {
  const int face = blockIdx.y;
  const int groups_per_row = (out_w + PX - 1) / PX;
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = g < groups_per_row * out_h;
  const int y = active ? g / groups_per_row : 0;
  const int x0 = active ? (g - y * groups_per_row) * PX : 0;
  uint8_t* dst = out + (((long)face * out_h + y) * out_w + x0) * 3;
  uint8_t px[PX * 3];
#pragma unroll
  for (int q = 0; q < PX * 3; ++q) px[q] = 0;

  const bool valid = ok == nullptr || ok[face] != 0;       // uniform over the workgroup (one face per blockIdx.y)
  __shared__ double sM[6];
  __shared__ float sT[fcp_interp::TAB * K];
  if (valid) {
    for (int i = threadIdx.x; i < fcp_interp::TAB * K; i += blockDim.x) sT[i] = tab.c[i];
    if (threadIdx.x == 0) {                                // inverse map: exactly warp_affine_kernel's
      double M[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) M[q] = mat[(long)face * 6 + q];
      double D = M[0] * M[4] - M[1] * M[3];
      D = D != 0 ? 1. / D : 0;
      const double A11 = M[4] * D, A22 = M[0] * D;
      M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
      const double b1 = -M[0] * M[2] - M[1] * M[5];
      const double b2 = -M[3] * M[2] - M[4] * M[5];
      M[2] = b1; M[5] = b2;
#pragma unroll
      for (int q = 0; q < 6; ++q) sM[q] = M[q];
    }
  }
  __syncthreads();
  if (!active) return;
  if (valid) {
    SrcView v;
    src.view(face, v);
    const uint8_t* __restrict__ images = src.base;
    const int sh = v.sh, sw = v.sw;
    const long sstep = v.sstep, s0off = v.s0off, total = v.total;
    const uint8_t* S0 = images + s0off;
    double M[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) M[q] = sM[q];
    const int X0 = (int)((unsigned)cv_round((M[1] * y + M[2]) * 1024.0) + 16u);
    const int Y0 = (int)((unsigned)cv_round((M[4] * y + M[5]) * 1024.0) + 16u);
    const int width1 = sw - K + 1 > 0 ? sw - K + 1 : 0, height1 = sh - K + 1 > 0 ? sh - K + 1 : 0;
    constexpr int ND = 3 * K / 4 + 1;
#pragma unroll
    for (int q = 0; q < PX; ++q) {
      const int x = x0 + q;
      if (x >= out_w) break;
      const int ad = cv_round(M[0] * x * 1024.0), bd = cv_round(M[3] * x * 1024.0);
      const int X = (int)((unsigned)X0 + (unsigned)ad) >> 5;
      const int Y = (int)((unsigned)Y0 + (unsigned)bd) >> 5;
      const int sx = sat_short(X >> 5) - (K / 2 - 1), sy = sat_short(Y >> 5) - (K / 2 - 1);
      int w[K * K];
      fcp_interp::interp_weights_2d<K>(sT + (Y & 31) * K, sT + (X & 31) * K, w);
      int acc[3] = {0, 0, 0};
      const long o0 = s0off + sy * sstep + sx * 3;
      if ((unsigned)sx < (unsigned)width1 && (unsigned)sy < (unsigned)height1 &&
          (((o0 + (K - 1) * sstep) & ~3L) + 4 * ND) <= total) {
        // interior: each of the K rows is one run of 3K bytes, read as ND aligned dwords
#pragma unroll
        for (int r = 0; r < K; ++r) {
          unsigned e[3 * K / 4];
          load_taps<K>(images, o0 + r * sstep, e);
#pragma unroll
          for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const int b = k * 3 + c;
              acc[c] += (int)((e[b >> 2] >> (8 * (b & 3))) & 255u) * w[r * K + k];
            }
          }
        }
      } else {
        if (border == 0 && (sx >= sw || sx + K <= 0 || sy >= sh || sy + K <= 0)) continue;   // all-constant: 0
        // replicate clamps inline, as the linear kernels do; border_interp then only ever sees the other borders, which also
        // leaves the code generated for the linear kernels' calls of it unchanged
        int xs[K];
#pragma unroll
        for (int k = 0; k < K; ++k) xs[k] = border == 1 ? min(max(sx + k, 0), sw - 1) : border_interp(sx + k, sw, border);
#pragma unroll
        for (int r = 0; r < K; ++r) {
          const int yr = border == 1 ? min(max(sy + r, 0), sh - 1) : border_interp(sy + r, sh, border);
          if (yr < 0) continue;                            // a constant-border tap outside the slice reads 0
          const uint8_t* row = S0 + yr * sstep;
#pragma unroll
          for (int k = 0; k < K; ++k) {
            if (xs[k] < 0) continue;
            const uint8_t* p = row + xs[k] * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += p[c] * w[r * K + k];
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int r = (acc[c] + (1 << 14)) >> 15;
        px[q * 3 + c] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
      }
    }
  }
  if (PX == 4 && x0 + 4 <= out_w && (out_w & 3) == 0) {
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst);  // 12 aligned bytes
    d32[0] = px[0] | (px[1] << 8) | (px[2] << 16) | ((uint32_t)px[3] << 24);
    d32[1] = px[4] | (px[5] << 8) | (px[6] << 16) | ((uint32_t)px[7] << 24);
    d32[2] = px[8] | (px[9] << 8) | (px[10] << 16) | ((uint32_t)px[11] << 24);
  } else {
    for (int q = 0; q < PX && x0 + q < out_w; ++q) {
      dst[q * 3] = px[q * 3]; dst[q * 3 + 1] = px[q * 3 + 1]; dst[q * 3 + 2] = px[q * 3 + 2];
    }
  }
}

}  // namespace

extern "C" int fcp_estimate_transform_counted(const float* src, const float* dst, int f, int k, int allow_skew,
                                              const int32_t* face_count, double* mat, int32_t* ok,
                                              int64_t* valid_total, fcp_stream_t stream) {
  FCP_REQUIRE(src && dst && mat && ok, "estimate_transform: null pointer");
  FCP_REQUIRE(f > 0 && k >= 2 && k <= 128, "estimate_transform: bad sizes (f=%d, k=%d)", f, k);
  hipLaunchKernelGGL(estimate_transform_kernel, dim3(fcp_cdiv(f, 64)), dim3(64), 0, (hipStream_t)stream, src,
                     dst, f, k, allow_skew, mat, ok, face_count, reinterpret_cast<long long*>(valid_total));
  FCP_LAUNCH_OK();
  return 0;
}

extern "C" int fcp_estimate_transform(const float* src, const float* dst, int f, int k, int allow_skew,
                                      double* mat, int32_t* ok, fcp_stream_t stream) {
  return fcp_estimate_transform_counted(src, dst, f, k, allow_skew, nullptr, mat, ok, nullptr, stream);
}

namespace {

// Groups of PX = 4 pixels, 256 per workgroup, one grid row (blockIdx.y) per face.
template <class Src>
int launch_fixed(const Src& src, const double* mat, const int32_t* ok, int f, int out_h, int out_w, int border, uint8_t* out,
                 fcp_stream_t stream) {
  const int groups = ((out_w + 3) / 4) * out_h;
  hipLaunchKernelGGL((warp_affine_kernel<4, Src>), dim3(fcp_cdiv(groups, 256), f), dim3(256), 0, (hipStream_t)stream, src,
                     mat, ok, out_h, out_w, border, out);
  FCP_LAUNCH_OK();
  return 0;
}

template <class Src>
int launch_float(const Src& src, const double* mat, const int32_t* ok, int f, int out_h, int out_w, int border, uint8_t* out,
                 fcp_stream_t stream) {
  const int groups = ((out_w + 3) / 4) * out_h;
  hipLaunchKernelGGL((warp_affine_float_kernel<4, Src>), dim3(fcp_cdiv(groups, 256), f), dim3(256), 0, (hipStream_t)stream,
                     src, mat, ok, out_h, out_w, border, out);
  FCP_LAUNCH_OK();
  return 0;
}

// The float 1-D table of one method, built once per process on the host (thread-safe static initialisation).
template <int K>
const fcp_interp::Tab1D<K>& interp_tab() {
  static const fcp_interp::Tab1D<K> t = [] {
    fcp_interp::Tab1D<K> v;
    fcp_interp::build_tab1d<K>(v);
    return v;
  }();
  return t;
}

// interp: 2 = cv2.INTER_CUBIC (K = 4), 4 = cv2.INTER_LANCZOS4 (K = 8); checked by the caller.
template <class Src>
int launch_interp(const Src& src, int interp, const double* mat, const int32_t* ok, int f, int out_h, int out_w, int border,
                  uint8_t* out, fcp_stream_t stream) {
  const int groups = ((out_w + 3) / 4) * out_h;
  if (interp == 2)
    hipLaunchKernelGGL((warp_affine_interp_kernel<4, 4, Src>), dim3(fcp_cdiv(groups, 256), f), dim3(256), 0,
                       (hipStream_t)stream, src, interp_tab<4>(), mat, ok, out_h, out_w, border, out);
  else
    hipLaunchKernelGGL((warp_affine_interp_kernel<8, 4, Src>), dim3(fcp_cdiv(groups, 256), f), dim3(256), 0,
                       (hipStream_t)stream, src, interp_tab<8>(), mat, ok, out_h, out_w, border, out);
  FCP_LAUNCH_OK();
  return 0;
}
// Checks of the ragged entry points: every descriptor inside the blob, each image at most 32767 px a side (the fixed
// family saturates source coordinates to short, as cv::warpAffine does).
int check_ragged(const char* what, const uint8_t* blob, int64_t blob_bytes, const fcp_warp_src* srcs_host,
                 const fcp_warp_src* srcs_dev, const double* mat, int f, int out_h, int out_w, int border, uint8_t* out) {
  FCP_REQUIRE(blob && srcs_host && srcs_dev && mat && out, "%s: null pointer", what);
  FCP_REQUIRE(blob_bytes > 0 && f > 0 && out_h > 0 && out_w > 0, "%s: bad sizes", what);
  FCP_REQUIRE(border >= 0 && border <= 4, "%s: unsupported border mode %d", what, border);
  FCP_REQUIRE(f <= 65535, "%s: at most 65535 faces per call", what);
  for (int i = 0; i < f; ++i) {
    const fcp_warp_src& s = srcs_host[i];
    FCP_REQUIRE(s.h > 0 && s.w > 0 && s.h <= 32767 && s.w <= 32767, "%s: face %d: source %dx%d (1..32767 a side)", what, i,
                s.w, s.h);
    FCP_REQUIRE(s.off >= 0 && s.off + (int64_t)s.h * s.w * 3 <= blob_bytes, "%s: face %d: source lies outside the blob", what,
                i);
  }
  return 0;
}

}  // namespace

extern "C" int fcp_warp_affine_u8(const uint8_t* images, int n, int h, int w, const int32_t* img_idx,
                                  const double* mat, const int32_t* ok, const int32_t* paddings, int f,
                                  int out_h, int out_w, int border, uint8_t* out, fcp_stream_t stream) {
  FCP_REQUIRE(images && img_idx && mat && out, "warp_affine: null pointer");
  FCP_REQUIRE(n > 0 && h > 0 && w > 0 && f > 0 && out_h > 0 && out_w > 0, "warp_affine: bad sizes");
  FCP_REQUIRE(border >= 0 && border <= 4, "warp_affine: unsupported border mode %d", border);
  FCP_REQUIRE(f <= 65535, "warp_affine: at most 65535 faces per call");
  FCP_REQUIRE(h <= 32767 && w <= 32767, "warp_affine: images of %dx%d (at most 32767 px a side: source coordinates saturate to short)", w, h);
  return launch_fixed(BatchSource{images, n, h, w, img_idx, paddings}, mat, ok, f, out_h, out_w, border, out, stream);
}

extern "C" int fcp_warp_affine_u8_float(const uint8_t* images, int n, int h, int w, const int32_t* img_idx,
                                        const double* mat, const int32_t* ok, const int32_t* paddings, int f,
                                        int out_h, int out_w, int border, uint8_t* out, fcp_stream_t stream) {
  FCP_REQUIRE(images && img_idx && mat && out, "warp_affine_float: null pointer");
  FCP_REQUIRE(n > 0 && h > 0 && w > 0 && f > 0 && out_h > 0 && out_w > 0, "warp_affine_float: bad sizes");
  FCP_REQUIRE(border >= 0 && border <= 4, "warp_affine_float: unsupported border mode %d", border);
  FCP_REQUIRE(f <= 65535, "warp_affine_float: at most 65535 faces per call");
  FCP_REQUIRE(h <= 32767 && w <= 32767, "warp_affine_float: images of %dx%d (at most 32767 px a side: source coordinates saturate to short)", w, h);
  return launch_float(BatchSource{images, n, h, w, img_idx, paddings}, mat, ok, f, out_h, out_w, border, out, stream);
}

extern "C" int fcp_warp_affine_u8_ragged(const uint8_t* blob, int64_t blob_bytes, const fcp_warp_src* srcs_host,
                                         const fcp_warp_src* srcs_dev, const double* mat, const int32_t* ok, int f,
                                         int out_h, int out_w, int border, uint8_t* out, fcp_stream_t stream) {
  const int rc = check_ragged("warp_affine_ragged", blob, blob_bytes, srcs_host, srcs_dev, mat, f, out_h, out_w, border, out);
  if (rc != 0) return rc;
  return launch_fixed(RaggedSource{blob, (long)blob_bytes, srcs_dev}, mat, ok, f, out_h, out_w, border, out, stream);
}

extern "C" int fcp_warp_affine_u8_float_ragged(const uint8_t* blob, int64_t blob_bytes, const fcp_warp_src* srcs_host,
                                               const fcp_warp_src* srcs_dev, const double* mat, const int32_t* ok, int f,
                                               int out_h, int out_w, int border, uint8_t* out, fcp_stream_t stream) {
  const int rc = check_ragged("warp_affine_float_ragged", blob, blob_bytes, srcs_host, srcs_dev, mat, f, out_h, out_w, border,
                              out);
  if (rc != 0) return rc;
  return launch_float(RaggedSource{blob, (long)blob_bytes, srcs_dev}, mat, ok, f, out_h, out_w, border, out, stream);
}

extern "C" int fcp_warp_affine_u8_interp(const uint8_t* images, int n, int h, int w, const int32_t* img_idx,
                                         const double* mat, const int32_t* ok, const int32_t* paddings, int f,
                                         int out_h, int out_w, int border, int interp, uint8_t* out, fcp_stream_t stream) {
  FCP_REQUIRE(images && img_idx && mat && out, "warp_affine_interp: null pointer");
  FCP_REQUIRE(n > 0 && h > 0 && w > 0 && f > 0 && out_h > 0 && out_w > 0, "warp_affine_interp: bad sizes");
  FCP_REQUIRE(border >= 0 && border <= 4, "warp_affine_interp: unsupported border mode %d", border);
  FCP_REQUIRE(fcp_interp::taps_of(interp) != 0, "warp_affine_interp: unsupported interpolation %d (2 cubic, 4 lanczos4)",
              interp);
  FCP_REQUIRE(f <= 65535, "warp_affine_interp: at most 65535 faces per call");
  FCP_REQUIRE(h <= 32767 && w <= 32767, "warp_affine_interp: images of %dx%d (at most 32767 px a side: source coordinates saturate to short)", w, h);
  return launch_interp(BatchSource{images, n, h, w, img_idx, paddings}, interp, mat, ok, f, out_h, out_w, border, out, stream);
}

extern "C" int fcp_warp_affine_u8_interp_ragged(const uint8_t* blob, int64_t blob_bytes, const fcp_warp_src* srcs_host,
                                                const fcp_warp_src* srcs_dev, const double* mat, const int32_t* ok, int f,
                                                int out_h, int out_w, int border, int interp, uint8_t* out,
                                                fcp_stream_t stream) {
  FCP_REQUIRE(fcp_interp::taps_of(interp) != 0,
              "warp_affine_interp_ragged: unsupported interpolation %d (2 cubic, 4 lanczos4)", interp);
  const int rc = check_ragged("warp_affine_interp_ragged", blob, blob_bytes, srcs_host, srcs_dev, mat, f, out_h, out_w, border,
                              out);
  if (rc != 0) return rc;
  return launch_interp(RaggedSource{blob, (long)blob_bytes, srcs_dev}, interp, mat, ok, f, out_h, out_w, border, out, stream);
}

extern "C" int fcp_warp_interp_weights(int interp, int16_t* out) {
  FCP_REQUIRE(out, "warp_interp_weights: null pointer");
  const int K = fcp_interp::taps_of(interp);
  FCP_REQUIRE(K != 0, "warp_interp_weights: unsupported interpolation %d (2 cubic, 4 lanczos4)", interp);
  const float* tab = K == 4 ? interp_tab<4>().c : interp_tab<8>().c;
  int w[64];
  for (int fy = 0; fy < fcp_interp::TAB; ++fy)
    for (int fx = 0; fx < fcp_interp::TAB; ++fx) {
      if (K == 4) fcp_interp::interp_weights_2d<4>(tab + fy * 4, tab + fx * 4, w);
      else fcp_interp::interp_weights_2d<8>(tab + fy * 8, tab + fx * 8, w);
      for (int k = 0; k < K * K; ++k) out[(fy * fcp_interp::TAB + fx) * K * K + k] = (int16_t)w[k];
    }
  return 0;
}
