"""Numpy / Python-int restatement of the guided-filter matte edge, the reference of the
matte-refine tests.  For one crop c (h,w,3), labels l (h,w), class bit set ``bits``, radius r and eps, n = (2 r + 1)^2:

    I(y,x)  = (9798 R + 19235 G + 3735 B + 16384) >> 15           the gray of min_sharpness
    p(y,x)  = tests/matte_ref.py's mask (0 / 255)
    box(v)  = the sum of v over the (2 r + 1)^2 window, indices through R (BORDER_REFLECT_101, iterated): n terms everywhere
    S_I, S_p, S_II, S_Ip = box(I), box(p), box(I I), box(I p)
    cov = n S_Ip - S_I S_p      var = n S_II - S_I S_I (>= 0)      den = var + eps n n
    rdiv(u, d) = sign(u) ((|u| + d // 2) // d)                    nearest, ties away from zero
    A = rdiv(4096 cov, den)                                       Q12 slope
    B = rdiv(4096 S_p - A S_I, n)                                 Q12 offset
    q = ((box(A) I + box(B) + 2048 n) >> 12) // n                 arithmetic shift, floor division
    alpha = min(255, max(0, q))
    out_ch = (c_ch alpha + fill_ch (255 - alpha) + 127) // 255    fill: the colour, or B_ch of section 2i

``refine`` is the vectorised form, int64 with an assert on every bound the kernel's widths rest on; ``refine_direct`` is
the same definition pixel by pixel in Python integers, for tiny sizes.
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("_matte_ref_for_refine", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                                    "matte_ref.py"))
MR = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MR)

MIN_RADIUS, MAX_RADIUS = 1, 16
MIN_EPS, MAX_EPS, DEFAULT_EPS = 1, 4096, 64
MAX_N = (2 * MAX_RADIUS + 1) ** 2            # 1089

# the bounds of the definition at r = 16 (the issue's figures, checked by test_matte_refine_cpu.py::test_bounds_arithmetic)
BOUND_S1 = 255 * MAX_N                       # S_I, S_p <= 277 695
BOUND_S2 = 255 * 255 * MAX_N                 # S_II, S_Ip <= 70 812 225
BOUND_COV = 78 * 10 ** 9                     # |cov|, var < 7.8e10
BOUND_DEN = 16 * 10 ** 10                    # den < 1.6e11
BOUND_A = 261121                             # |A| <= 4096 * 127.5 / (2 sqrt(eps)), eps >= 1, rounded
BOUND_B = 68 * 10 ** 6                       # |B| < 6.8e7
BOUND_BOX_A = 29 * 10 ** 7                   # |box(A)| < 2.9e8
BOUND_BOX_B = 75 * 10 ** 9                   # |box(B)| < 7.5e10


def gray(crop):
    """(..., 3) uint8 RGB -> int64 gray 0..255."""
    c = np.asarray(crop).astype(np.int64)
    return (9798 * c[..., 0] + 19235 * c[..., 1] + 3735 * c[..., 2] + 16384) >> 15


def box(v, r):
    """(h,w) int64 -> the (2 r + 1)^2 window sums, reflect-101 iterated."""
    v = np.asarray(v, np.int64)
    h, w = v.shape
    rows = np.zeros((h, w), np.int64)
    for i in range(-r, r + 1):
        rows += v[:, [MR.reflect101(x + i, w) for x in range(w)]]
    out = np.zeros((h, w), np.int64)
    for j in range(-r, r + 1):
        out += rows[[MR.reflect101(y + j, h) for y in range(h)], :]
    return out


def rdiv(u, d):
    """sign(u) ((|u| + d // 2) // d), elementwise in int64."""
    u, d = np.asarray(u, np.int64), np.asarray(d, np.int64)
    return np.sign(u) * ((np.abs(u) + d // 2) // d)


def coefficients(guide, p, r, eps):
    """guide, p (h,w) ints 0..255 -> (A, B) int64, the Q12 slope and offset of every window."""
    assert MIN_RADIUS <= r <= MAX_RADIUS and MIN_EPS <= eps <= MAX_EPS
    I, p = np.asarray(guide, np.int64), np.asarray(p, np.int64)
    n = (2 * r + 1) ** 2
    s_i, s_p, s_ii, s_ip = box(I, r), box(p, r), box(I * I, r), box(I * p, r)
    assert max(s_i.max(), s_p.max()) <= BOUND_S1 and max(s_ii.max(), s_ip.max()) <= BOUND_S2 < 2 ** 32
    cov = n * s_ip - s_i * s_p
    var = n * s_ii - s_i * s_i
    den = var + eps * n * n
    assert var.min() >= 0 and np.abs(cov).max() < BOUND_COV and var.max() < BOUND_COV and den.max() < BOUND_DEN
    assert np.abs(cov).max() * 4096 < 32 * 10 ** 13
    a = rdiv(cov * 4096, den)
    assert np.abs(a).max() <= BOUND_A
    b = rdiv(s_p * 4096 - a * s_i, n)
    assert np.abs(b).max() < BOUND_B
    return a, b


def q_of(guide, a, b, r):
    """The unclamped output ((box(A) I + box(B) + 2048 n) >> 12) // n."""
    n = (2 * r + 1) ** 2
    box_a, box_b = box(a, r), box(b, r)
    assert np.abs(box_a).max() < BOUND_BOX_A < 2 ** 31 and np.abs(box_b).max() < BOUND_BOX_B
    return ((box_a * np.asarray(guide, np.int64) + box_b + n * 2048) >> 12) // n


def refine(guide, p, r, eps):
    """guide, p (h,w) -> alpha (h,w) uint8."""
    a, b = coefficients(guide, p, r, eps)
    return np.clip(q_of(guide, a, b, r), 0, 255).astype(np.uint8)


def _rdiv_int(u, d):
    q = (abs(u) + d // 2) // d
    return -q if u < 0 else q


def refine_direct(guide, p, r, eps):
    """The definition pixel by pixel in Python integers: no array arithmetic, no separable pass."""
    I = [[int(v) for v in row] for row in np.asarray(guide)]
    P = [[int(v) for v in row] for row in np.asarray(p)]
    h, w = len(I), len(I[0])
    n = (2 * r + 1) ** 2
    ys = [[MR.reflect101(y + j, h) for j in range(-r, r + 1)] for y in range(h)]
    xs = [[MR.reflect101(x + i, w) for i in range(-r, r + 1)] for x in range(w)]
    A = [[0] * w for _ in range(h)]
    B = [[0] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            s_i = s_p = s_ii = s_ip = 0
            for yy in ys[y]:
                for xx in xs[x]:
                    s_i += I[yy][xx]
                    s_p += P[yy][xx]
                    s_ii += I[yy][xx] * I[yy][xx]
                    s_ip += I[yy][xx] * P[yy][xx]
            cov, var = n * s_ip - s_i * s_p, n * s_ii - s_i * s_i
            A[y][x] = _rdiv_int(cov * 4096, var + eps * n * n)
            B[y][x] = _rdiv_int(s_p * 4096 - A[y][x] * s_i, n)
    out = np.zeros((h, w), np.uint8)
    for y in range(h):
        for x in range(w):
            box_a = sum(A[yy][xx] for yy in ys[y] for xx in xs[x])
            box_b = sum(B[yy][xx] for yy in ys[y] for xx in xs[x])
            q = ((box_a * I[y][x] + box_b + n * 2048) >> 12) // n
            out[y, x] = min(255, max(0, q))
    return out


def alpha_of(crops, labels, bits, r, eps):
    """(F,h,w,3) crops, (F,h,w) labels -> the refined alpha (F,h,w) uint8."""
    crops, labels = np.asarray(crops), np.asarray(labels)
    if len(labels) == 0:
        return np.zeros(labels.shape, np.uint8)
    return np.stack([refine(gray(c), MR.mask(l, bits), r, eps) for c, l in zip(crops, labels)])


def matte(crops, labels, bits, r, eps, fill):
    """Fill mode: (out, alpha), both uint8."""
    alpha = alpha_of(crops, labels, bits, r, eps)
    return MR.composite(crops, alpha, fill), alpha


# ---- the inputs that expose a narrow accumulator
def stripes(h, w, r):
    """Vertical stripes of width r + 1: (guide 254 / 255, p 0 / 255 following them)."""
    on = ((np.arange(w) // (r + 1)) & 1).astype(np.int64)
    return np.tile(254 + on, (h, 1)), np.tile(255 * on, (h, 1))


def stripe_inputs(f, h, w, r):
    """The stripes as (crops (f,h,w,3) uint8 whose gray is 254 / 255, labels (f,h,w) uint8 0 / 1); face k is shifted by k."""
    crops, labels = np.zeros((f, h, w, 3), np.uint8), np.zeros((f, h, w), np.uint8)
    for k in range(f):
        on = (((np.arange(w) + k) // (r + 1)) & 1).astype(np.uint8)
        crops[k] = (254 + np.tile(on, (h, 1)))[..., None]
        labels[k] = np.tile(on, (h, 1))
    assert set(np.unique(gray(crops))) <= {254, 255}
    return crops, labels
