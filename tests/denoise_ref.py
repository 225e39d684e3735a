"""numpy reference of Cropper(denoise=H), written from the definition in INTEGRATION.md section 2p (not from the kernel):

    P = 3, S = 10, ONE = 4096; the crop is extended by reflection (np.pad(..., mode="reflect")), so H, W >= 14
    g        = (9798 R + 19235 G + 3735 B + 16384) >> 15
    d(p,o)   = sum over t in [-P,P]^2 of (g(p + t) - g(p + o + t))^2          for every offset o in [-S,S]^2
    k        = d >> shift;  w(p,o) = min(lut[k], ONE) if k < n, else 0
    W        = sum over o of w(p,o)
    out_c(p) = (sum over o of w(p,o) c(p + o) + (W >> 1)) // W                W == 0 copies the pixel

``nlm`` is the vectorised form (per offset: squared difference, 2-D cumulative sum, box difference), ``nlm_loops`` the plain
per-pixel triple loop it is checked against, ``weight_lut`` this file's own statement of the host's table."""
import math

import numpy as np

P = 3
S = 10
ONE = 4096
MIN_SIDE = P + S + 1
MAX_LUT = 4096
TABLE = {1: (442, 0), 2: (1767, 0), 8: (3533, 3), 12: (3974, 4), 32: (3533, 7)}      # H -> (n, shift), from the issue


def gray(crop):
    c = crop.astype(np.int64)
    return (9798 * c[..., 0] + 19235 * c[..., 1] + 3735 * c[..., 2] + 16384) >> 15


def weight_lut(strength):
    """H -> (uint16 table, shift): cut = floor(ln(2 ONE) 49 H^2); shift the smallest s with (cut >> s) < 4096; n = (cut >>
    shift) + 1; lut[k] = floor(ONE exp(-(k 2^shift) / (49 H^2)) + 0.5), all in float64."""
    scale = 49.0 * float(strength) * float(strength)
    cut = int(math.floor(math.log(2.0 * ONE) * scale))
    shift = 0
    while (cut >> shift) >= MAX_LUT:
        shift += 1
    n = (cut >> shift) + 1
    lut = [int(math.floor(ONE * math.exp(-(k * 2.0 ** shift) / scale) + 0.5)) for k in range(n)]
    return np.array(lut, np.uint16), shift


def _weights(d, lut, shift):
    table = np.minimum(np.asarray(lut).astype(np.int64), ONE)
    k = d >> shift
    return np.where(k < len(table), table[np.minimum(k, len(table) - 1)], 0)


def nlm_one(crop, lut, shift):
    """One crop (h,w,3) uint8 -> (h,w,3) uint8."""
    h, w, _ = crop.shape
    assert h >= MIN_SIDE and w >= MIN_SIDE and 1 <= len(lut) <= MAX_LUT
    g = np.pad(gray(crop), P + S, mode="reflect")                       # g[y + P + S, x + P + S] = gray of (y, x)
    c = np.pad(crop.astype(np.int64), ((S, S), (S, S), (0, 0)), mode="reflect")
    own = g[S:S + h + 2 * P, S:S + w + 2 * P]                           # the patches' pixels around every p, rim P
    total = np.zeros((h, w), np.int64)
    num = np.zeros((h, w, 3), np.int64)
    for oy in range(-S, S + 1):
        for ox in range(-S, S + 1):
            diff = own - g[S + oy:S + oy + h + 2 * P, S + ox:S + ox + w + 2 * P]
            ii = np.zeros((h + 2 * P + 1, w + 2 * P + 1), np.int64)
            ii[1:, 1:] = (diff * diff).cumsum(0).cumsum(1)
            n = 2 * P + 1
            d = ii[n:, n:] - ii[:-n, n:] - ii[n:, :-n] + ii[:-n, :-n]   # (h, w): the 7 x 7 box sums
            wgt = _weights(d, lut, shift)
            total += wgt
            num += wgt[..., None] * c[S + oy:S + oy + h, S + ox:S + ox + w]
    out = (num + (total >> 1)[..., None]) // np.maximum(total, 1)[..., None]
    return np.where((total == 0)[..., None], crop, out).astype(np.uint8)


def nlm(crops, lut, shift):
    """Crops (F,h,w,3) uint8 -> (F,h,w,3) uint8."""
    crops = np.asarray(crops)
    if len(crops) == 0:
        return np.zeros(crops.shape, np.uint8)
    return np.stack([nlm_one(c, lut, shift) for c in crops])


def denoise(crops, strength):
    return nlm(crops, *weight_lut(strength))


def nlm_loops(crop, lut, shift):
    """The definition, pixel by pixel: for tiny crops."""
    h, w, _ = crop.shape
    g = gray(crop)
    n = len(lut)

    def at(v, size):                                                    # BORDER_REFLECT_101
        return -v if v < 0 else (2 * (size - 1) - v if v >= size else v)
    out = np.zeros_like(crop)
    taps = range(-P, P + 1)
    for y in range(h):
        for x in range(w):
            total, num = 0, [0, 0, 0]
            a = g[np.ix_([at(y + t, h) for t in taps], [at(x + t, w) for t in taps])]            # the pixel's own patch
            for oy in range(-S, S + 1):
                for ox in range(-S, S + 1):
                    b = g[np.ix_([at(y + oy + t, h) for t in taps], [at(x + ox + t, w) for t in taps])]
                    d = int(((a - b) ** 2).sum())
                    k = d >> shift
                    wgt = min(int(lut[k]), ONE) if k < n else 0
                    total += wgt
                    q = crop[at(y + oy, h), at(x + ox, w)]
                    for ch in range(3):
                        num[ch] += wgt * int(q[ch])
            out[y, x] = crop[y, x] if total == 0 else [(v + (total >> 1)) // total for v in num]
    return out


def scene(h=96, w=80):
    """A clean synthetic scene (gradients, an ellipse, a checkered band), (h,w,3) uint8."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([40 + 150 * x / (w - 1), 60 + 120 * y / (h - 1), 200 - 100 * (x + y) / (h + w - 2)], -1)
    inside = ((x - 0.45 * w) / (0.28 * w)) ** 2 + ((y - 0.4 * h) / (0.3 * h)) ** 2 <= 1
    img[inside] = (215, 170, 140)
    band = (y >= 0.8 * h) & (y < 0.92 * h)
    check = ((x // 8 + y // 8) % 2 == 0)
    img[band & check] = (30, 30, 40)
    img[band & ~check] = (220, 220, 210)
    return np.rint(img).astype(np.uint8)


def noisy(clean, sigma=10.0, seed=0):
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(clean.astype(np.float64) + rng.normal(0.0, sigma, clean.shape)), 0, 255).astype(np.uint8)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10.0 * math.log10(255.0 ** 2 / mse)
