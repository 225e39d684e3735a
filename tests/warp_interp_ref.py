"""numpy restatement of cv2.warpAffine(INTER_CUBIC / INTER_LANCZOS4) on uint8 RGB (OpenCV 4.x imgproc/src/imgwarp.cpp:
initInterTab1D, initInterTab2D(fixpt=true), WarpAffineInvoker, remapBicubic / remapLanczos4).  RESTATED FROM THE PUBLISHED
SOURCE, NOT PINNED: no OpenCV build was at hand; tests/test_warp_interp_pins.py compares it with recorded cv2 output once
tools/make_cv2_fixture.py has written tests/golden/opencv_interp.npz.  The yardstick of the HIP kernels.

- coordinates: those of the fixed-point linear warp (``oracle.align_ref.warp_affine``): inverse map in double, AB_BITS = 10,
  round_delta = 16, X, Y >> 5, sx0 = sat_short(X >> 5), table index (Y & 31) * 32 + (X & 31);
- 1-D coefficients for x = i * (1.f/32): interpolateCubic (A = -0.75, float32 op by op, ``oracle.batch_ref._cubic_coeffs``)
  or interpolateLanczos4 (sin / cos in double through the C library, 1e30f at the kernel's zero, float32 1/sum);
- 2-D int16 weights: round-half-even(float(ty * tx) * 32768) saturated to short; a sum other than 32768 is corrected in the
  2 x 2 block at rows / columns K/2, K/2 + 1 (smallest entry when diff > 0, largest when diff < 0);
- per pixel: taps from sx0 - (K/2 - 1), rows and columns through cv::borderInterpolate (a constant-border tap reads 0, a
  pixel whose taps are all outside is 0), int32 sum, saturate((sum + 2**14) >> 15)."""
import math

import numpy as np

from oracle.align_ref import _cv_round, _wrap32, border_interpolate
from oracle.batch_ref import _cubic_coeffs

F32 = np.float32
INTERP = {"cubic": 2, "lanczos4": 4}        # cv2.INTER_CUBIC, cv2.INTER_LANCZOS4
TAPS = {2: 4, 4: 8}
TAB = 32

_S45 = 0.70710678118654752440084436210485
_CS = ((1, 0), (-_S45, -_S45), (0, 1), (_S45, -_S45), (-1, 0), (_S45, _S45), (0, -1), (-_S45, _S45))


def lanczos4_coeffs(x) -> np.ndarray:
    """interpolateLanczos4(x): 8 float32 coefficients."""
    x = F32(x)
    xp3 = F32(x + F32(3))
    y0 = float(-xp3) * math.pi * 0.25
    s0, c0 = math.sin(y0), math.cos(y0)
    c = np.zeros(8, F32)
    total = F32(0)
    for i in range(8):
        t = F32(xp3 - F32(i))
        if abs(t) >= F32(1e-6):
            y = float(-t) * math.pi * 0.25
            c[i] = F32((_CS[i][0] * s0 + _CS[i][1] * c0) / (y * y))
        else:
            c[i] = F32(1e30)
        total = F32(total + c[i])
    total = F32(F32(1) / total)
    return (c * total).astype(F32)


def tab1d(interp: int) -> np.ndarray:
    """initInterTab1D: (32, K) float32."""
    xs = np.arange(TAB, dtype=F32) * F32(1.0 / TAB)
    if interp == 2:
        return _cubic_coeffs(xs)
    if interp == 4:
        return np.stack([lanczos4_coeffs(x) for x in xs]).astype(F32)
    raise ValueError(f"unsupported interpolation {interp}")


def weights_2d(interp: int) -> np.ndarray:
    """initInterTab2D(fixpt=true): (1024, K, K) int16, row fy * 32 + fx."""
    t = tab1d(interp)
    K = t.shape[1]
    v = (t[:, None, :, None] * t[None, :, None, :]).astype(F32) * F32(32768)          # (fy, fx, k1, k2)
    w = np.clip(np.rint(v.astype(F32)), -32768, 32767).astype(np.int64).reshape(TAB * TAB, K, K)
    h = K // 2
    for blk in w:
        diff = int(blk.sum()) - 32768
        if diff == 0:
            continue
        mn = mx = (h, h)
        for k1 in (h, h + 1):
            for k2 in (h, h + 1):
                if blk[k1, k2] < blk[mn]:
                    mn = (k1, k2)
                elif blk[k1, k2] > blk[mx]:
                    mx = (k1, k2)
        at = mx if diff < 0 else mn
        blk[at] = np.int16(np.int64(blk[at]) - diff)
    return w.astype(np.int16)


_W2D = {}


def _weights(interp):
    if interp not in _W2D:
        _W2D[interp] = weights_2d(interp).astype(np.int64)
    return _W2D[interp]


def source_coords(M, dsize):
    """The fixed-point source coordinates of every output pixel: (X, Y) after the >> 5, both (oh, ow) int64."""
    ow, oh = int(dsize[0]), int(dsize[1])
    m = np.asarray(M, np.float64).reshape(6).copy()
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    xs = np.arange(ow, dtype=np.float64)
    ys = np.arange(oh, dtype=np.float64)
    adelta = _cv_round(m[0] * xs * 1024.0)
    bdelta = _cv_round(m[3] * xs * 1024.0)
    X0 = _wrap32(_cv_round((m[1] * ys + m[2]) * 1024.0) + 16)
    Y0 = _wrap32(_cv_round((m[4] * ys + m[5]) * 1024.0) + 16)
    X = _wrap32(X0[:, None] + adelta[None, :]) >> 5
    Y = _wrap32(Y0[:, None] + bdelta[None, :]) >> 5
    return X, Y


def warp_affine_interp(image, M, dsize, border=0, interp=2):
    """image (h,w,3) uint8, M 2x3 forward transform, dsize = (width, height), border a cv2.BORDER_* code (0..4), interp
    2 (cubic) or 4 (Lanczos-4) -> (height, width, 3) uint8."""
    K = TAPS[interp]
    img = np.asarray(image, np.uint8)
    sh, sw = img.shape[:2]
    X, Y = source_coords(M, dsize)
    sx = np.clip(X >> 5, -32768, 32767) - (K // 2 - 1)
    sy = np.clip(Y >> 5, -32768, 32767) - (K // 2 - 1)
    W = _weights(interp)[(Y & 31) * TAB + (X & 31)]                     # (oh, ow, K, K)
    cols = [border_interpolate(sx + k, sw, border) for k in range(K)]
    rows = [border_interpolate(sy + r, sh, border) for r in range(K)]
    S = img.astype(np.int64)
    acc = np.zeros(X.shape + (3,), np.int64)
    for r in range(K):
        for k in range(K):
            okm = (rows[r] >= 0) & (cols[k] >= 0)
            v = S[np.where(okm, rows[r], 0), np.where(okm, cols[k], 0)]
            acc += np.where(okm[..., None], v, 0) * W[..., r, k][..., None]
    assert np.abs(acc).max(initial=0) < 2 ** 31                           # remap accumulates in int32
    out = np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
    if border == 0:
        out[(sx >= sw) | (sx + K <= 0) | (sy >= sh) | (sy + K <= 0)] = 0
    return out


def warp_batch(images, img_idx, mats, ok, paddings, dsize, border=0, interp=2):
    """The batch kernel's contract: face i warps images[img_idx[i]] un-padded by paddings[img] (t, b, l, r) when given;
    faces with ok == 0 are all zeros.  -> (F, height, width, 3) uint8."""
    ow, oh = int(dsize[0]), int(dsize[1])
    out = np.zeros((len(img_idx), oh, ow, 3), np.uint8)
    for i, ii in enumerate(img_idx):
        if ok is not None and not ok[i]:
            continue
        im = images[ii]
        if paddings is not None:
            t, b, l, r = (int(v) for v in paddings[ii])
            im = im[t:im.shape[0] - b, l:im.shape[1] - r]
        out[i] = warp_affine_interp(im, np.asarray(mats[i], np.float64).reshape(2, 3), dsize, border, interp)
    return out


def kernel_f64(interp, d):
    """The continuous kernel the tables sample, in float64, at tap distances d (any shape): Keys cubic with A = -0.75, or
    the Lanczos-4 window sinc(d) sinc(d / 4)."""
    d = np.abs(np.asarray(d, np.float64))
    if interp == 2:
        A = -0.75
        return np.where(d <= 1, ((A + 2) * d - (A + 3)) * d * d + 1,
                        np.where(d < 2, ((A * d - 5 * A) * d + 8 * A) * d - 4 * A, 0.0))
    return np.where(d < 4, np.sinc(d) * np.sinc(d / 4), 0.0)
