"""Numpy restatement of ``Cropper(clahe=...)``, the reference of the CLAHE tests: integers
and explicit ``np.float32`` operations in the order of the definition.  For one crop (h,w,3) uint8 RGB, grid g, clip c:

1. colour   Y  = (4899 R + 9617 G + 1868 B + 8192) >> 14
            Cr = sat(((R - Y) 11682 + (128 << 14) + 8192) >> 14)       Cb = sat(((B - Y) 9241 + (128 << 14) + 8192) >> 14)
            back: R = sat(Y' + (((Cr - 128) 22987 + 8192) >> 14)),  B = sat(Y' + (((Cb - 128) 29049 + 8192) >> 14)),
                  G = sat(Y' + (((Cb - 128) (-5636) + (Cr - 128) (-11698) + 8192) >> 14));   floor shifts, sat to 0..255
2. tiles    h % g == 0 and w % g == 0: the luma plane as is; else g - h % g rows below and g - w % g columns on the
            right, BORDER_REFLECT_101 (a divisible dimension grows by a full g when the other is not);  th, tw = extended
            size // g;  area = th tw
3. LUT      hist of the tile;  clip = max(int(c area / 256), 1) in double (area or more clips nothing: taken as area);
            bins above clip cut to it, the excess summed into clipped;  batch = clipped // 256 to every bin;  residual =
            clipped - 256 batch;  residual > 0: step = max(256 // residual, 1), bin i gets + 1 iff i % step == 0 and
            i // step < residual;  s = inclusive prefix sum;  lut[i] = sat(rint(float32(s[i]) * scale)),
            scale = float32(255) / float32(area)
4. apply    inv_th = 1.0f / th;  tyf = y inv_th - 0.5f;  ty1 = floor(tyf);  ya = tyf - ty1;  ya1 = 1.0f - ya;  then
            ty2 = min(ty1 + 1, g - 1), ty1 = max(ty1, 0);  the same in x;
            res = (L[ty1][tx1][Y] xa1 + L[ty1][tx2][Y] xa) ya1 + (L[ty2][tx1][Y] xa1 + L[ty2][tx2][Y] xa) ya
            Y'  = sat(rint(res))

It restates ``cv2.createCLAHE(c, (g, g)).apply(Y)`` between ``cv2.cvtColor(COLOR_RGB2YCrCb)`` and ``COLOR_YCrCb2RGB``.
"""
import numpy as np

F32 = np.float32
MAX_GRID = 16
DEFAULT_GRID = 8


def rgb_to_ycrcb(crop):
    """(..., 3) uint8 -> Y, Cr, Cb as int64 arrays in 0..255."""
    c = np.asarray(crop).astype(np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    y = (4899 * r + 9617 * g + 1868 * b + 8192) >> 14
    cr = np.clip(((r - y) * 11682 + (128 << 14) + 8192) >> 14, 0, 255)
    cb = np.clip(((b - y) * 9241 + (128 << 14) + 8192) >> 14, 0, 255)
    return y, cr, cb


def ycrcb_to_rgb_unsaturated(y, cr, cb):
    """int64 planes -> (..., 3) int64 before the clamp (the tests look for values outside 0..255)."""
    r = y + (((cr - 128) * 22987 + 8192) >> 14)
    g = y + (((cb - 128) * -5636 + (cr - 128) * -11698 + 8192) >> 14)
    b = y + (((cb - 128) * 29049 + 8192) >> 14)
    return np.stack([r, g, b], -1)


def ycrcb_to_rgb(y, cr, cb):
    return np.clip(ycrcb_to_rgb_unsaturated(y, cr, cb), 0, 255).astype(np.uint8)


def extend(plane, g):
    """The plane the tiles are cut from: as is when both sides divide by g, else reflected-101 below and on the right."""
    h, w = plane.shape
    if h % g == 0 and w % g == 0:
        return plane
    eh, ew = h + g - h % g, w + g - w % g
    ys = [y if y < h else 2 * (h - 1) - y for y in range(eh)]
    xs = [x if x < w else 2 * (w - 1) - x for x in range(ew)]
    return plane[ys][:, xs]


def tile_lut(tile, c):
    """One tile (th,tw) of luma -> (lut uint8[256], dict(clip, clipped, residual, step)); step is 0 without a residual."""
    area = int(tile.size)
    hist = np.bincount(np.asarray(tile).reshape(-1), minlength=256).astype(np.int64)
    limit = c * area / 256
    clip = area if limit >= area else max(int(limit), 1)
    clipped = int(np.maximum(hist - clip, 0).sum())
    hist = np.minimum(hist, clip)
    batch = clipped // 256
    residual = clipped - 256 * batch
    hist = hist + batch
    step = 0
    if residual > 0:
        step = max(256 // residual, 1)
        i = np.arange(256)
        hist = hist + ((i % step == 0) & (i // step < residual))
    s = np.cumsum(hist)
    assert s[-1] == area and area <= 1 << 24
    scale = F32(255) / F32(area)
    lut = np.clip(np.rint(s.astype(F32) * scale), 0, 255).astype(np.uint8)
    return lut, {"clip": clip, "clipped": clipped, "residual": residual, "step": step}


def _axis(n, t, g):
    """Pixel index 0..n-1 -> (first LUT index, second LUT index, weight of the second, weight of the first)."""
    inv = F32(1.0) / F32(t)
    tf = np.arange(n).astype(F32) * inv - F32(0.5)
    assert tf.dtype == F32
    t1 = np.floor(tf)
    a = tf - t1
    a1 = F32(1.0) - a
    t1 = t1.astype(np.int64)
    assert t1.min() >= -1 and t1.max() <= g - 1
    return np.maximum(t1, 0), np.minimum(t1 + 1, g - 1), a, a1


def clahe_plane(y, c, g):
    """Luma (h,w) int -> (equalised luma uint8 (h,w), luts uint8 (g,g,256), diagnostics [g][g] of dicts)."""
    y = np.asarray(y).astype(np.int64)
    h, w = y.shape
    assert 1 <= g <= MAX_GRID and h >= 2 * g and w >= 2 * g
    e = extend(y, g)
    th, tw = e.shape[0] // g, e.shape[1] // g
    luts = np.zeros((g, g, 256), np.uint8)
    diag = [[None] * g for _ in range(g)]
    for ty in range(g):
        for tx in range(g):
            luts[ty, tx], diag[ty][tx] = tile_lut(e[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw], c)
    ty1, ty2, ya, ya1 = _axis(h, th, g)
    tx1, tx2, xa, xa1 = _axis(w, tw, g)
    L = luts.astype(F32)
    yy1, yy2, xx1, xx2 = ty1[:, None], ty2[:, None], tx1[None, :], tx2[None, :]
    top = L[yy1, xx1, y] * xa1[None, :] + L[yy1, xx2, y] * xa[None, :]
    bottom = L[yy2, xx1, y] * xa1[None, :] + L[yy2, xx2, y] * xa[None, :]
    res = top * ya1[:, None] + bottom * ya[:, None]
    assert res.dtype == F32
    return np.clip(np.rint(res), 0, 255).astype(np.uint8), luts, diag


def clahe_full(crop, c, g=DEFAULT_GRID):
    """One crop (h,w,3) uint8 -> dict(rgb, y, y_eq, luts, diag, unsaturated)."""
    y, cr, cb = rgb_to_ycrcb(crop)
    y_eq, luts, diag = clahe_plane(y, c, g)
    un = ycrcb_to_rgb_unsaturated(y_eq.astype(np.int64), cr, cb)
    return {"rgb": np.clip(un, 0, 255).astype(np.uint8), "y": y.astype(np.uint8), "y_eq": y_eq, "luts": luts, "diag": diag,
            "unsaturated": un}


def clahe(crops, c, g=DEFAULT_GRID):
    """(F,h,w,3) uint8 -> (F,h,w,3) uint8."""
    crops = np.asarray(crops)
    if len(crops) == 0:
        return np.zeros(crops.shape, np.uint8)
    return np.stack([clahe_full(crop, c, g)["rgb"] for crop in crops])


# ---- the inputs of tests/test_clahe_gpu.py; tests/test_clahe_cpu.py shows that they reach every branch
def smooth_crops(seed, f, h, w):
    """Crops with the statistics of a photograph: a few blurred blobs per channel plus noise, so that tiles hold narrow
    histograms (clipping) as well as wide ones."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((f, h, w, 3), np.float64)
    for k in range(f):
        for ch in range(3):
            img = np.full((h, w), rng.uniform(40, 200))
            for _ in range(4):
                cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, max(h, w) / 2)
                img += rng.uniform(-120, 120) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            out[k, ..., ch] = img + rng.normal(0, rng.uniform(1, 12), (h, w))
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def primaries_crop(h=40, w=48):
    """Saturated primaries and their complements in vertical bands, over a luma ramp from top to bottom: equalising moves Y
    far enough that Y' plus the chroma terms leaves 0..255 in both directions."""
    colours = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (255, 255, 255),
                        (0, 0, 0)], np.int64)
    band = colours[(np.arange(w) * len(colours)) // w]                        # (w, 3)
    ramp = (np.arange(h) * 255 // (h - 1))[:, None, None]                      # 0 .. 255 down the rows
    mixed = (band[None] * 3 + ramp) // 4
    return np.clip(mixed, 0, 255).astype(np.uint8)


def gpu_cases():
    """name -> (crops (F,h,w,3) uint8, grid, clip limit): the table of the issue."""
    cases = {
        "64x64_g8_c2": (smooth_crops(11, 3, 64, 64), 8, 2.0),
        "50x37_g8_c40": (smooth_crops(12, 2, 50, 37), 8, 40.0),
        "48x37_g8_view": (smooth_crops(13, 3, 48, 37), 8, 3.0),
        "33x31_g1": (smooth_crops(14, 1, 33, 31), 1, 4.0),
        "32x32_g16": (smooth_crops(15, 1, 32, 32), 16, 2.0),
        "512x512_const_c0.5": (np.full((1, 512, 512, 3), 93, np.uint8), 1, 0.5),
        "512x512_const_c1000": (np.full((1, 512, 512, 3), 93, np.uint8), 1, 1000.0),
        "primaries_g4": (primaries_crop()[None], 4, 8.0),
    }
    return cases
