"""Numpy restatement of the background blur, the reference of the matte-blur tests, written
from the definition as 2-D sums: one explicit loop over the (j, i) offsets of the window, int64 throughout.  For one
crop c (h,w,3), labels l (h,w), class bit set ``bits``, feather K and taps t[0..r]:

    m, alpha  = tests/matte_ref.py's mask and alpha (this module reuses them)
    b(y,x)    = 1 where m == 0, else 0
    D(y,x)    = sum_j sum_i t|j| t|i| b(y+j, x+i)                 over the positions inside the image
    N_ch(y,x) = sum_j sum_i t|j| t|i| b(y+j, x+i) c_ch(y+j, x+i)
    B_ch      = (N_ch + D // 2) // D where D > 0, else c_ch
    out_ch    = (c_ch * alpha + B_ch * (255 - alpha) + 127) // 255

The taps are an argument: ``blur_taps`` below restates how the package makes them from sigma, and the CPU tests compare
the two; kernel and reference are always compared on the same list.
"""
import importlib.util
import math
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("_matte_ref_for_blur", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                  "matte_ref.py"))
MR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MR)

TAP_SUM = 4096
MIN_RADIUS, MAX_RADIUS = 3, 48


def blur_taps(sigma):
    """r = min(48, max(3, ceil(3 sigma))); t_k = max(1, floor(4096 g_k / s)) for k >= 1, t_0 takes the rest."""
    r = min(MAX_RADIUS, max(MIN_RADIUS, math.ceil(3 * sigma)))
    g = [math.exp(-k * k / (2 * sigma * sigma)) for k in range(r + 1)]
    s = g[0] + 2 * sum(g[1:])
    t = [0] + [max(1, math.floor(TAP_SUM * g[k] / s)) for k in range(1, r + 1)]
    t[0] = TAP_SUM - 2 * sum(t[1:])
    return t


def window_sums(planes, taps):
    """(..., h, w, P) int64 planes -> sum_j sum_i t|j| t|i| planes(y+j, x+i), positions outside the image left out."""
    planes = np.asarray(planes, np.int64)
    h, w = planes.shape[-3], planes.shape[-2]
    r = len(taps) - 1
    acc = np.zeros(planes.shape, np.int64)
    for j in range(-min(r, h - 1), min(r, h - 1) + 1):
        # output rows y with 0 <= y + j < h
        ya, yb = max(0, -j), min(h, h - j)
        for i in range(-min(r, w - 1), min(r, w - 1) + 1):
            xa, xb = max(0, -i), min(w, w - i)
            acc[..., ya:yb, xa:xb, :] += taps[abs(j)] * taps[abs(i)] * planes[..., ya + j:yb + j, xa + i:xb + i, :]
    return acc


def background(crops, labels, bits, taps):
    """(F,h,w,3) crops, (F,h,w) labels -> (B (F,h,w,3) uint8, D (F,h,w) int64): the blurred background, defined at every
    pixel (the crop where D == 0), and the weight it was divided by."""
    crops = np.asarray(crops)
    b = (MR.mask(labels, bits) == 0).astype(np.int64)[..., None]
    sums = window_sums(np.concatenate([b, b * crops.astype(np.int64)], axis=-1), taps)
    d, n = sums[..., :1], sums[..., 1:]
    assert n.max(initial=0) + d.max(initial=0) // 2 < 2 ** 32 and (n <= 255 * d).all()
    safe = np.maximum(d, 1)
    bg = np.where(d > 0, (n + d // 2) // safe, crops.astype(np.int64))
    assert bg.max(initial=0) <= 255
    return bg.astype(np.uint8), d[..., 0]


def alpha_of(labels, bits, feather):
    labels = np.asarray(labels)
    if len(labels) == 0:
        return np.zeros(labels.shape, np.uint8)
    return np.stack([MR.alpha_separable(MR.mask(l, bits), feather) for l in labels])


def over(crops, alpha, bg):
    a = np.asarray(alpha).astype(np.int64)[..., None]
    t = np.asarray(crops).astype(np.int64) * a + np.asarray(bg).astype(np.int64) * (255 - a)
    return ((t + 127) // 255).astype(np.uint8)


def matte_blur(crops, labels, bits, feather, taps, bg=None):
    """(F,h,w,3) crops, (F,h,w) labels -> (out, alpha), both uint8.  ``bg`` is ``background(...)[0]`` when the caller
    has it already (it does not depend on the feather)."""
    if bg is None:
        bg = background(crops, labels, bits, taps)[0]
    alpha = alpha_of(labels, bits, feather)
    return over(crops, alpha, bg), alpha


def plain_blur(crops, taps):
    """What the feature is NOT: the same window over every pixel, subject included (the halo)."""
    crops = np.asarray(crops)
    ones = np.ones(crops.shape[:-1] + (1,), np.int64)
    sums = window_sums(np.concatenate([ones, crops.astype(np.int64)], axis=-1), taps)
    d, n = sums[..., :1], sums[..., 1:]
    return ((n + d // 2) // d).astype(np.uint8)


# ---- label patterns of the tests (tests/matte_ref.py's, and three of this feature's own)
PATTERNS = ("random", "checker", "corners", "all_fg", "all_bg", "one_bg")


def labels_of(pattern, rng, f, h, w):
    if pattern == "random":
        return MR.random_labels(rng, f, h, w)
    if pattern == "checker":
        return MR.checker_labels(f, h, w)
    if pattern == "corners":
        return MR.corner_labels(f, h, w)
    if pattern == "all_fg":
        return np.full((f, h, w), 1, np.uint8)
    if pattern == "all_bg":
        return np.zeros((f, h, w), np.uint8)
    if pattern == "one_bg":
        # a single background pixel, in another corner per face
        out = np.full((f, h, w), 1, np.uint8)
        for k in range(f):
            out[k, (h - 1) * (k & 1), (w - 1) * ((k >> 1) & 1)] = 0
        return out
    raise ValueError(pattern)
