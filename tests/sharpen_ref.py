"""numpy reference of Cropper(sharpen=A), written from the definition in INTEGRATION.md section 2q (not from the kernel),
in int64 throughout:

    t[0..r]  : integer taps, t[0] + 2 sum(t[1..r]) == 4096, 1 <= r <= 48
    g        = (9798 R + 19235 G + 3735 B + 16384) >> 15
    coordinates outside the crop are clamped to its edge (np.pad(..., mode="edge")): any H, W >= 1
    Hs(y,x)  = sum_i t|i| g(y, clamp(x + i))
    B(y,x)   = sum_j t|j| Hs(clamp(y + j), x)
    b8       = (B + 32768) >> 16
    d        = (g << 8) - b8
    e        = sign(d) * max(|d| - (T << 8), 0)
    A_q      = floor(256 A + 0.5), 1..1024
    v_c      = (c << 16) + A_q * e + 32768
    out_c    = v_c < 0 ? 0 : min(255, v_c >> 16)

``blur_taps`` is this file's own statement of the host's taps (``matte.blur_taps``), ``unsharp_parts`` returns every
intermediate, ``unsharp_float`` is the same formula in float64 with the same taps."""
import math

import numpy as np

TAP_SUM = 4096
MIN_RADIUS, MAX_RADIUS = 3, 48
DEFAULT_SIGMA = 1.5


def gray(crop):
    c = crop.astype(np.int64)
    return (9798 * c[..., 0] + 19235 * c[..., 1] + 3735 * c[..., 2] + 16384) >> 15


def blur_taps(sigma):
    """sigma -> t[0..r]: r = min(48, max(3, ceil(3 sigma))), g_k = exp(-k^2 / (2 sigma^2)), s = g_0 + 2 sum g_k,
    t_k = max(1, floor(4096 g_k / s)) for k >= 1, t_0 the rest of 4096; float64."""
    sigma = float(sigma)
    r = min(MAX_RADIUS, max(MIN_RADIUS, int(math.ceil(3 * sigma))))
    g = [math.exp(-k * k / (2 * sigma * sigma)) for k in range(r + 1)]
    s = g[0] + 2 * sum(g[1:])
    t = [0] + [max(1, int(math.floor(TAP_SUM * g[k] / s))) for k in range(1, r + 1)]
    t[0] = TAP_SUM - 2 * sum(t[1:])
    return t


def amount_q8(amount):
    return int(math.floor(256.0 * float(amount) + 0.5))


def _check(taps):
    taps = [int(t) for t in taps]
    r = len(taps) - 1
    assert 1 <= r <= MAX_RADIUS and min(taps) >= 0 and taps[0] + 2 * sum(taps[1:]) == TAP_SUM, taps
    return taps, r


def blur(g, taps):
    """The gray plane g (h,w) int64 -> B (h,w) int64, the separable sum with the edge clamped."""
    taps, r = _check(taps)
    h, w = g.shape
    p = np.pad(g, ((0, 0), (r, r)), mode="edge")
    hs = np.zeros((h, w), np.int64)
    for i in range(-r, r + 1):
        hs += taps[abs(i)] * p[:, r + i:r + i + w]
    p = np.pad(hs, ((r, r), (0, 0)), mode="edge")
    b = np.zeros((h, w), np.int64)
    for j in range(-r, r + 1):
        b += taps[abs(j)] * p[r + j:r + j + h, :]
    return b


def unsharp_parts(crop, taps, amount_q, threshold):
    """One crop (h,w,3) uint8 -> a dict of every intermediate (int64) and ``out`` (h,w,3) uint8."""
    assert 1 <= amount_q <= 1024 and 0 <= threshold <= 255
    g = gray(crop)
    b = blur(g, taps)
    b8 = (b + 32768) >> 16
    d = (g << 8) - b8
    e = np.sign(d) * np.maximum(np.abs(d) - (threshold << 8), 0)
    v = (crop.astype(np.int64) << 16) + (amount_q * e)[..., None] + 32768
    out = np.where(v < 0, 0, np.minimum(255, v >> 16)).astype(np.uint8)
    return {"g": g, "B": b, "b8": b8, "d": d, "e": e, "v": v, "out": out}


def unsharp(crops, taps, amount_q, threshold):
    """Crops (F,h,w,3) uint8 -> (F,h,w,3) uint8."""
    crops = np.asarray(crops)
    if len(crops) == 0:
        return np.zeros(crops.shape, np.uint8)
    return np.stack([unsharp_parts(c, taps, amount_q, threshold)["out"] for c in crops])


def sharpen(crops, amount, sigma=DEFAULT_SIGMA, threshold=0):
    return unsharp(crops, blur_taps(sigma), amount_q8(amount), threshold)


def unsharp_float(crop, taps, amount_q, threshold):
    """The same formula in float64 with the same taps, before the final rounding: (h,w,3) float64, unclipped."""
    taps, r = _check(taps)
    g = gray(crop).astype(np.float64)
    b = blur(gray(crop), taps).astype(np.float64) / float(TAP_SUM * TAP_SUM)
    d = g - b
    e = np.sign(d) * np.maximum(np.abs(d) - threshold, 0.0)
    return crop.astype(np.float64) + (amount_q / 256.0) * e[..., None]
