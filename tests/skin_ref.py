"""numpy reference of Cropper(smooth_skin=S), written from the definition in INTEGRATION.md section 2s (not from the
kernel).  For one crop c (h,w,3) uint8 and its label map l (h,w) uint8, the class bit set ``bits``, the taps t[0..r], the
range table rng[0..255] and the amount A (1..256):

    g(p)     = (9798 R + 19235 G + 3735 B + 16384) >> 15
    m(p)     = 1 if l(p) < 32 and bit l(p) of bits is set, else 0; m = 0 outside the crop
    s(o)     = (t[|oy|] * t[|ox|] + 2048) >> 12                              o in [-r, r]^2
    w(p, o)  = m(p + o) * ((s(o) * min(rng[|g(p + o) - g(p)|], 4096) + 2048) >> 12)
    W(p)     = sum over o of w(p, o)
    b_c(p)   = (sum over o of w(p, o) c_c(p + o) + (W >> 1)) // W            W == 0: b = c(p)
    alpha(p) = the feather-7 alpha of 255 m, reflect-101 borders: taps (8,28,56,72,56,28,8) both ways, (sum + 32768) >> 16
    e(p)     = max(0, 2 alpha(p) - 255);   E(p) = (e(p) * A + 128) >> 8
    out_c(p) = (b_c E + c_c (255 - E) + 127) // 255 if m(p) == 1, else c_c(p)

``smooth_one`` is the vectorised form (one pass per offset), ``smooth_loops`` the plain per-pixel loop it is checked
against, ``range_lut`` / ``blur_taps`` / ``amount_q8`` this file's own statement of the host's tables, and ``scene`` a
synthetic portrait with a known clean image."""
import math

import numpy as np

ONE = 4096
FEATHER = (8, 28, 56, 72, 56, 28, 8)
DEFAULT_CLASSES = (1, 7, 8, 10, 14)
DEFAULT_BITS = sum(1 << c for c in DEFAULT_CLASSES)
DEFAULT_SIGMA = 3.0
MIN_RADIUS, MAX_RADIUS = 3, 24


def gray(crop):
    c = np.asarray(crop).astype(np.int64)
    return (9798 * c[..., 0] + 19235 * c[..., 1] + 3735 * c[..., 2] + 16384) >> 15


def mask01(labels, bits):
    lut = np.array([1 if v < 32 and (bits >> v) & 1 else 0 for v in range(256)], np.int64)
    return lut[np.asarray(labels)]


def blur_taps(sigma):
    """matte.blur_taps restated: r = max(3, ceil(3 sigma)), t_k = max(1, floor(4096 g_k / sum)), t_0 the rest of 4096."""
    r = max(MIN_RADIUS, math.ceil(3 * sigma))
    g = [math.exp(-k * k / (2.0 * sigma * sigma)) for k in range(r + 1)]
    total = g[0] + 2 * sum(g[1:])
    t = [0] + [max(1, math.floor(ONE * g[k] / total)) for k in range(1, r + 1)]
    t[0] = ONE - 2 * sum(t[1:])
    return t


def range_lut(strength):
    """S -> rng[0..255] uint16: floor(4096 exp(-d^2 / (2 S^2)) + 0.5), in float64."""
    s = float(strength)
    return np.array([int(math.floor(ONE * math.exp(-(d * d) / (2.0 * s * s)) + 0.5)) for d in range(256)], np.uint16)


def amount_q8(amount):
    return int(round(256 * float(amount)))


def spatial(taps):
    """s(o) for o in [-r, r]^2 as a (2r+1, 2r+1) int64 array."""
    t = np.array([int(v) for v in taps], np.int64)
    r = len(t) - 1
    full = t[np.abs(np.arange(-r, r + 1))]
    return (full[:, None] * full[None, :] + 2048) >> 12


def _reflect101(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def feather7(m01):
    """The feather-7 alpha of the 0 / 1 mask, (h,w) int64 0..255."""
    h, w = m01.shape
    m = 255 * m01.astype(np.int64)
    hs = np.zeros((h, w), np.int64)
    for i in range(7):
        hs += FEATHER[i] * m[:, [_reflect101(x + i - 3, w) for x in range(w)]]
    v = np.zeros((h, w), np.int64)
    for j in range(7):
        v += FEATHER[j] * hs[[_reflect101(y + j - 3, h) for y in range(h)], :]
    return (v + 32768) >> 16


def blend(b, c, m01, alpha, amount_q):
    e = np.maximum(0, 2 * alpha - 255)
    big_e = ((e * amount_q + 128) >> 8)[..., None]
    mixed = (b * big_e + c * (255 - big_e) + 127) // 255
    return np.where((m01 == 1)[..., None], mixed, c).astype(np.uint8)


def smooth_one(crop, labels, bits, taps, rng, amount_q):
    """One crop (h,w,3) uint8 and its labels (h,w) uint8 -> (h,w,3) uint8."""
    crop = np.asarray(crop)
    h, w, _ = crop.shape
    r = len(taps) - 1
    assert MIN_RADIUS <= r <= MAX_RADIUS and 1 <= amount_q <= 256 and len(rng) == 256
    table = np.minimum(np.asarray(rng).astype(np.int64), ONE)
    s = spatial(taps)
    c = crop.astype(np.int64)
    g = gray(crop)
    m = mask01(labels, bits)
    if not m.any():                                             # out = c wherever m == 0
        return crop.copy()
    gp = np.pad(g, r)
    mp = np.pad(m, r)                                           # 0 outside the crop: no weight there
    cp = np.pad(c, ((r, r), (r, r), (0, 0)))
    total = np.zeros((h, w), np.int64)
    num = np.zeros((h, w, 3), np.int64)
    for oy in range(-r, r + 1):
        for ox in range(-r, r + 1):
            ys, xs = slice(r + oy, r + oy + h), slice(r + ox, r + ox + w)
            wgt = mp[ys, xs] * ((s[oy + r, ox + r] * table[np.abs(gp[ys, xs] - g)] + 2048) >> 12)
            total += wgt
            num += wgt[..., None] * cp[ys, xs]
    assert num.max(initial=0) + (total.max(initial=0) >> 1) < 2 ** 32
    b = np.where((total == 0)[..., None], c, (num + (total >> 1)[..., None]) // np.maximum(total, 1)[..., None])
    return blend(b, c, m, feather7(m), amount_q)


def smooth(crops, labels, bits, taps, rng, amount_q):
    """Crops (F,h,w,3) uint8 and labels (F,h,w) uint8 -> (F,h,w,3) uint8."""
    crops = np.asarray(crops)
    if len(crops) == 0:
        return np.zeros(crops.shape, np.uint8)
    return np.stack([smooth_one(c, l, bits, taps, rng, amount_q) for c, l in zip(crops, labels)])


def smooth_skin(crops, labels, strength, sigma=DEFAULT_SIGMA, amount=1.0, classes=DEFAULT_CLASSES):
    """The option: host tables from S, sigma and the amount."""
    bits = sum(1 << int(c) for c in set(classes))
    return smooth(crops, labels, bits, blur_taps(sigma), range_lut(strength), amount_q8(amount))


def smooth_loops(crop, labels, bits, taps, rng, amount_q):
    """The definition, pixel by pixel in Python integers: for tiny crops."""
    crop = np.asarray(crop)
    h, w, _ = crop.shape
    r = len(taps) - 1
    g = gray(crop).tolist()
    lab = np.asarray(labels).tolist()

    def skin(y, x):
        if not (0 <= y < h and 0 <= x < w):
            return 0
        v = lab[y][x]
        return 1 if v < 32 and (bits >> v) & 1 else 0
    out = crop.copy()
    for y in range(h):
        for x in range(w):
            if not skin(y, x):
                continue
            total, num = 0, [0, 0, 0]
            for oy in range(-r, r + 1):
                for ox in range(-r, r + 1):
                    if not skin(y + oy, x + ox):
                        continue
                    s = (int(taps[abs(oy)]) * int(taps[abs(ox)]) + 2048) >> 12
                    wgt = (s * min(int(rng[abs(g[y + oy][x + ox] - g[y][x])]), ONE) + 2048) >> 12
                    total += wgt
                    for ch in range(3):
                        num[ch] += wgt * int(crop[y + oy, x + ox, ch])
            b = [int(v) for v in crop[y, x]] if total == 0 else [(v + (total >> 1)) // total for v in num]
            a = 0
            for j in range(7):
                for i in range(7):
                    a += FEATHER[j] * FEATHER[i] * 255 * skin(_reflect101(y + j - 3, h), _reflect101(x + i - 3, w))
            a = (a + 32768) >> 16
            e = ((max(0, 2 * a - 255)) * amount_q + 128) >> 8
            out[y, x] = [(b[ch] * e + int(crop[y, x, ch]) * (255 - e) + 127) // 255 for ch in range(3)]
    return out


# ---------------------------------------------------------------------------------------------------------- the scene
SKIN_TONE = (205, 160, 135)
DARK_TONE = (70, 45, 40)            # brow
LIP_TONE = (165, 70, 80)
HAIR_TONE = (35, 28, 25)
BACK_TONE = (90, 110, 140)


def scene(h=96, w=80, noise=6.0, overshoot=2, seed=0):
    """A synthetic portrait with a known clean image -> dict of
    clean (h,w,3) u8, noisy (h,w,3) u8 (Gaussian noise of sigma ``noise`` on every pixel), labels (h,w) u8 (class 1 over
    the face ellipse, which overshoots the true skin into the brow, the lip and the hair edge by ``overshoot`` pixels;
    17 hair, 0 background), flat (h,w) bool: true skin at least 8 px from every other region, and mislabelled (h,w) bool:
    brow and lip pixels the label map calls skin."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    face = ((x - 0.5 * w) / (0.34 * w)) ** 2 + ((y - 0.52 * h) / (0.38 * h)) ** 2 <= 1
    hair = (y < 0.26 * h) & (((x - 0.5 * w) / (0.42 * w)) ** 2 + ((y - 0.4 * h) / (0.4 * h)) ** 2 <= 1)
    brow = (np.abs(y - 0.40 * h) <= 0.02 * h) & (np.abs(np.abs(x - 0.5 * w) - 0.15 * w) <= 0.08 * w)
    lip = ((x - 0.5 * w) / (0.12 * w)) ** 2 + ((y - 0.72 * h) / (0.035 * h)) ** 2 <= 1
    clean = np.empty((h, w, 3), np.float64)
    clean[:] = BACK_TONE
    clean[face] = SKIN_TONE
    clean[hair] = HAIR_TONE
    clean[brow] = DARK_TONE
    clean[lip] = LIP_TONE
    true_skin = face & ~hair & ~brow & ~lip

    def grow(region, n):
        out = region.copy()
        for _ in range(n):
            p = np.pad(out, 1)
            out = p[1:-1, 1:-1] | p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]
        return out
    inner = lambda region: ~grow(~region, overshoot)            # the region eroded: the label map gives its rim to the skin
    labels = np.zeros((h, w), np.uint8)
    labels[hair & ~(grow(face & ~hair, overshoot))] = 17
    labels[face & ~hair] = 1
    labels[grow(face & ~hair, overshoot) & hair] = 1           # the skin label runs into the hair
    labels[inner(brow)] = 2
    labels[inner(lip)] = 12
    mislabelled = (brow | lip) & (labels == 1)
    flat = ~grow(~true_skin, 8)
    rng = np.random.default_rng(seed)
    noisy = np.clip(np.rint(clean + rng.normal(0.0, noise, clean.shape)), 0, 255).astype(np.uint8)
    return dict(clean=np.rint(clean).astype(np.uint8), noisy=noisy, labels=labels, flat=flat, mislabelled=mislabelled)


def scene_figures(strength=10, sigma=3.0, h=96, w=80):
    """The figures of the README: (std of the error over flat skin before, after, mean |change| of the mislabelled brow
    and lip pixels, their mean |error| against the clean image before, after), in gray levels over the three channels."""
    sc = scene(h, w)
    out = smooth_skin(sc["noisy"][None], sc["labels"][None], strength, sigma)[0].astype(np.float64)
    clean, noisy = sc["clean"].astype(np.float64), sc["noisy"].astype(np.float64)
    before = float((noisy - clean)[sc["flat"]].std())
    after = float((out - clean)[sc["flat"]].std())
    moved = float(np.abs(out - noisy)[sc["mislabelled"]].mean())
    wrong = sc["mislabelled"]
    return before, after, moved, float(np.abs(noisy - clean)[wrong].mean()), float(np.abs(out - clean)[wrong].mean())
