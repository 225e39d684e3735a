"""Numpy / Python-int restatement of the background replacement, the reference of the matte
tests.  For one crop c (h,w,3), labels l (h,w), class bit set ``bits``, fill b[3] and feather K (r = K // 2):

    m(y,x)  = 255 if l(y,x) < 32 and bit l(y,x) of bits is set, else 0
    k       = K 3: (64,128,64)   5: (16,64,96,64,16)   7: (8,28,56,72,56,28,8)        K 0: alpha = m
    H(y,x)  = sum_i k[i] * m(y, R(x+i-r, w))
    alpha   = (sum_j k[j] * H(R(y+j-r, h), x) + 32768) >> 16
    out_ch  = (c_ch * alpha + b_ch * (255 - alpha) + 127) // 255

R is BORDER_REFLECT_101, iterated for dimensions smaller than the radius.
"""
import numpy as np

TAPS = {3: (64, 128, 64), 5: (16, 64, 96, 64, 16), 7: (8, 28, 56, 72, 56, 28, 8)}
FEATHERS = (0, 3, 5, 7)
DEFAULT_BITS = sum(1 << c for c in range(1, 19))
PIN_SIZES = [(1, 1), (1, 5), (2, 2), (3, 2), (2, 7), (13, 17), (64, 48)]


def reflect101(p, n):
    """R(p, n): R(p, 1) = 0; otherwise, while p is outside [0, n): p = -p if p < 0 else 2 (n - 1) - p."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def mask(labels, bits):
    """(..., h, w) uint8 labels -> uint8 0 / 255."""
    lut = np.array([255 if v < 32 and (bits >> v) & 1 else 0 for v in range(256)], np.uint8)
    return lut[np.asarray(labels)]


def alpha_direct(m, feather):
    """The 2-D sum, pixel by pixel in Python integers: (sum_j sum_i k[j] k[i] m(R(y+j-r), R(x+i-r)) + 32768) >> 16."""
    m = np.asarray(m)
    if feather == 0:
        return m.astype(np.uint8).copy()
    k, r = TAPS[feather], feather // 2
    h, w = m.shape
    ys = [[reflect101(y + j - r, h) for j in range(feather)] for y in range(h)]
    xs = [[reflect101(x + i - r, w) for i in range(feather)] for x in range(w)]
    mm = m.astype(np.int64).tolist()
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            s = 0
            for j, yy in enumerate(ys[y]):
                row = mm[yy]
                s += k[j] * sum(k[i] * row[xx] for i, xx in enumerate(xs[x]))
            out[y, x] = (s + 32768) >> 16
    return out


def alpha_separable(m, feather):
    """The two-pass form: H (16 bits, no rounding), then the vertical pass and one rounding."""
    m = np.asarray(m)
    if feather == 0:
        return m.astype(np.uint8).copy()
    k, r = TAPS[feather], feather // 2
    h, w = m.shape
    m = m.astype(np.int64)
    hs = np.zeros((h, w), np.int64)
    for i in range(feather):
        hs += k[i] * m[:, [reflect101(x + i - r, w) for x in range(w)]]
    assert hs.max(initial=0) <= 65280
    v = np.zeros((h, w), np.int64)
    for j in range(feather):
        v += k[j] * hs[[reflect101(y + j - r, h) for y in range(h)], :]
    return ((v + 32768) >> 16).astype(np.uint8)


def composite(crop, alpha, fill):
    """(..., h, w, 3) uint8 crop, (..., h, w) uint8 alpha, fill (r, g, b) -> (t + 127) // 255."""
    a = np.asarray(alpha).astype(np.int64)[..., None]
    t = np.asarray(crop).astype(np.int64) * a + np.array(fill, np.int64) * (255 - a)
    return ((t + 127) // 255).astype(np.uint8)


def matte(crops, labels, bits, feather, fill):
    """(F,h,w,3) crops, (F,h,w) labels -> (out, alpha), both uint8."""
    alpha = np.stack([alpha_separable(mask(l, bits), feather) for l in labels]) if len(labels) else np.zeros(np.shape(labels), np.uint8)
    return composite(crops, alpha, fill), alpha


def as_fill(background):
    return (background,) * 3 if isinstance(background, int) else tuple(background)


# ---- input builders
def random_mask(rng, h, w):
    return (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)


def random_labels(rng, f, h, w):
    return rng.integers(0, 19, (f, h, w), dtype=np.uint8)


def checker_labels(f, h, w):
    """1-pixel checkerboard of classes 1 and 0 (face k starts with k & 1)."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([((yy + xx + k) & 1).astype(np.uint8) for k in range(f)])


def corner_labels(f, h, w):
    """One foreground pixel (class 17, then 1, ...) in each corner, background (0) elsewhere."""
    out = np.zeros((f, h, w), np.uint8)
    for k in range(f):
        for y in (0, h - 1):
            for x in (0, w - 1):
                out[k, y, x] = 17 if k % 2 == 0 else 1
    return out


def random_crops(rng, f, h, w):
    return rng.integers(0, 256, (f, h, w, 3), dtype=np.uint8)
