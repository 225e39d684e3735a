"""Numpy restatement of the RGBA cut-out and of the subject-colour estimate, the reference
of the cut-out tests: int64 throughout.  The window sums are those of tests/matte_blur_ref.py, taken as a sum over i
inside a sum over j (``window_sums``: the same integers exactly, in 2 (2 r + 1) steps instead of (2 r + 1)^2; the CPU
tests hold the two against each other).  For crops c (F,h,w,3) u8, an alpha plane a (F,h,w) u8 and taps t[0..r]:

    sF(p) = 1 where a(p) == 255 else 0          "certainly subject"
    sB(p) = 1 where a(p) == 0   else 0          "certainly background"
    D_F   = sum_j sum_i t|j| t|i| sF(y+j, x+i)                  taps inside the image only
    N_F,ch= sum_j sum_i t|j| t|i| sF(y+j, x+i) c_ch(y+j, x+i)   the same taps; D_B, N_B,ch with sB
    F^_ch = D_F > 0 ? (N_F,ch + D_F/2) / D_F : c_ch             B^_ch likewise with D_B, N_B
    R_ch  = 255 c_ch - (a F^_ch + (255 - a) B^_ch)              in [-65025, 65025]
    E_ch  = clamp( floor((65025 F^_ch + a R_ch + 32512) / 65025), 0, 255 )
    F_ch  = c_ch where a == 255;  E_ch where 0 < a < 255;  (unused) where a == 0

    rgba, no estimate : (c_r, c_g, c_b, a) where a > 0, (0,0,0,0) where a == 0
    rgba, estimate    : (F_r, F_g, F_b, a) where a > 0, (0,0,0,0) where a == 0
    fill, estimate    : (F_ch a + fill_ch (255 - a) + 127) // 255, three channels

The division of E is Python's floor division.  ``taps`` None means "no estimate".
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("_matte_blur_ref_for_cutout",
                                               os.path.join(os.path.dirname(os.path.abspath(__file__)), "matte_blur_ref.py"))
BR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(BR)
MR = BR.MR

RGBA, FILL = 0, 1
ROW_W, ROW_H = 256, 4                  # kRowTileW, kRowTileH of csrc/fcp_cutout.hip (the rows pass)
COL_W, COL_H = 8, 128                  # kTileW, kTileH of csrc/fcp_cutout.hip (the columns pass)
# (8, 300) is wider than a row tile and (70, 20) taller than the 64 rows of the blur's column tile; the columns pass here
# takes 128 rows, so the last four cross it: a tile boundary exactly, two tiles and a one-row tail, a margin that reaches
# into the tile above (130 and 300 rows at r = 48), three tiles of two groups and a narrow tail
SHAPES = [(1, 1), (5, 6), (17, 9), (37, 53), (96, 80), (8, 300), (70, 20),
          (COL_H, COL_W), (COL_H + 2, 20), (2 * COL_H + 1, COL_W + 1), (300, 12)]
SIGMAS = (0.5, 4, 16)                  # r = 3, 12, 48


def window_sums(planes, taps):
    """(..., h, w, P) int64 planes -> sum_j t|j| sum_i t|i| planes(y+j, x+i), positions outside the image left out."""
    planes = np.asarray(planes, np.int64)
    h, w = planes.shape[-3], planes.shape[-2]
    r = len(taps) - 1
    rows = np.zeros(planes.shape, np.int64)
    for i in range(-min(r, w - 1), min(r, w - 1) + 1):
        xa, xb = max(0, -i), min(w, w - i)
        rows[..., :, xa:xb, :] += taps[abs(i)] * planes[..., :, xa + i:xb + i, :]
    acc = np.zeros(planes.shape, np.int64)
    for j in range(-min(r, h - 1), min(r, h - 1) + 1):
        ya, yb = max(0, -j), min(h, h - j)
        acc[..., ya:yb, :, :] += taps[abs(j)] * rows[..., ya + j:yb + j, :, :]
    return acc


def side_estimate(crops, s, taps):
    """The mask-normalised Gaussian of the crops over the indicator s (F,h,w) of 0 / 1 -> (estimate (F,h,w,3) int64, the
    crop where D == 0; D (F,h,w) int64; the largest N + D // 2)."""
    c = np.asarray(crops).astype(np.int64)
    s = np.asarray(s).astype(np.int64)[..., None]
    sums = window_sums(np.concatenate([s, s * c], axis=-1), taps)
    d, n = sums[..., :1], sums[..., 1:]
    peak = int((n + d // 2).max(initial=0))
    assert peak < 2 ** 32 and (n <= 255 * d).all()
    est = np.where(d > 0, (n + d // 2) // np.maximum(d, 1), c)
    assert est.max(initial=0) <= 255
    return est, d[..., 0], peak


def estimates(crops, alpha, taps):
    """-> (F^, B^, D_F, D_B), int64."""
    alpha = np.asarray(alpha)
    fh, df, _ = side_estimate(crops, alpha == 255, taps)
    bh, db, _ = side_estimate(crops, alpha == 0, taps)
    return fh, bh, df, db


def corrected(crops, alpha, fh, bh):
    """E (F,h,w,3) int64 at every pixel, from F^ and B^."""
    c = np.asarray(crops).astype(np.int64)
    a = np.asarray(alpha).astype(np.int64)[..., None]
    r = 255 * c - (a * fh + (255 - a) * bh)
    assert np.abs(r).max(initial=0) <= 65025
    num = 65025 * fh + a * r + 32512
    assert np.abs(num).max(initial=0) < 2 ** 25
    return np.clip(num // 65025, 0, 255)


def foreground(crops, alpha, taps):
    """F (F,h,w,3) uint8: the crop where a == 255, E where 0 < a < 255, the crop (unused) where a == 0; the crop
    everywhere without taps."""
    crops, alpha = np.asarray(crops), np.asarray(alpha)
    if taps is None or crops.size == 0:
        return crops.copy()
    fh, bh, _, _ = estimates(crops, alpha, taps)
    soft = ((alpha > 0) & (alpha < 255))[..., None]
    return np.where(soft, corrected(crops, alpha, fh, bh), crops.astype(np.int64)).astype(np.uint8)


def rgba(crops, alpha, taps=None, fg=None):
    """-> (F,h,w,4) uint8.  ``fg`` is ``foreground(crops, alpha, taps)`` when the caller has it already."""
    alpha = np.asarray(alpha)
    fg = foreground(crops, alpha, taps) if fg is None else fg
    out = np.concatenate([fg, alpha[..., None]], axis=-1).astype(np.uint8)
    out[alpha == 0] = 0
    return out


def fill(crops, alpha, taps, background, fg=None):
    """-> (F,h,w,3) uint8: the estimated colour over the uniform fill.  ``fg`` as in ``rgba``."""
    a = np.asarray(alpha).astype(np.int64)[..., None]
    f = (foreground(crops, alpha, taps) if fg is None else fg).astype(np.int64)
    b = np.asarray(background, np.int64).reshape(1, 1, 1, 3)
    return ((f * a + b * (255 - a) + 127) // 255).astype(np.uint8)


def cutout(crops, alpha, mode, background, taps):
    return rgba(crops, alpha, taps) if mode == RGBA else fill(crops, alpha, taps, background)


# ---- the synthetic scene of the quality condition
def scene():
    """96 x 80: (c (96,80,3) u8, a (96,80) u8, the true subject colour F (96,80,3) float64)."""
    h, w = 96, 80
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.sqrt((yy - 48) ** 2 / 30.0 ** 2 + (xx - 40) ** 2 / 24.0 ** 2)
    al = np.clip((1 - d) * 6 + 0.5, 0, 1)
    f = np.stack([200 + 20 * np.sin(xx / 5), 60 + 20 * np.cos(yy / 7), np.full((h, w), 50.0)], -1)
    b = np.stack([np.full((h, w), 20.0), 200 + 30 * np.sin(yy / 9), 30 + 20 * np.cos(xx / 4)], -1)
    rng = np.random.default_rng(1)
    f = f + rng.integers(-6, 7, f.shape)
    b = b + rng.integers(-6, 7, b.shape)
    c = np.round(al[..., None] * f + (1 - al[..., None]) * b).clip(0, 255).astype(np.uint8)
    return c, np.round(255 * al).astype(np.uint8), f


# ---- alpha planes and crops of the tests
def disc_labels(f, h, w):
    """(f,h,w) u8 labels, 1 inside an ellipse whose centre moves with the face, else 0."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((f, h, w), np.uint8)
    for k in range(f):
        cy, cx = h / 2.0 + k, w / 2.0 - k
        out[k] = ((yy - cy) ** 2 / max(h * 0.35, 1) ** 2 + (xx - cx) ** 2 / max(w * 0.3, 1) ** 2 <= 1.0)
    return out


def feathered(labels, bits, feather):
    """The alpha of tests/matte_ref.py for a batch of label maps."""
    return BR.alpha_of(labels, bits, feather)


ALPHAS = ("disc0", "disc3", "disc5", "disc7", "random", "ones", "zeros", "mixed0", "mixed1")
MIXED = ("disc5", "random", "ones", "zeros")


def alpha_of(kind, rng, f, h, w):
    """(f,h,w) u8.  The disc kinds are the host's feathered alpha (the GPU tests make the same plane on the device and
    compare); "mixedK" gives a face of each kind in turn, beginning with kind K of ``MIXED``: a batch of 3 of "mixed0"
    and one of "mixed1" hold every kind beside another."""
    if kind.startswith("disc"):
        return feathered(disc_labels(f, h, w), 1 << 1, int(kind[4:]))
    if kind == "random":
        return rng.integers(0, 256, (f, h, w), dtype=np.uint8)
    if kind == "ones":
        return np.full((f, h, w), 255, np.uint8)
    if kind == "zeros":
        return np.zeros((f, h, w), np.uint8)
    if kind.startswith("mixed"):
        return np.concatenate([alpha_of(MIXED[(int(kind[5:]) + k) % len(MIXED)], rng, 1, h, w) for k in range(f)])
    raise ValueError(kind)
