"""References, bounds and input builders of the align / warp / batch-builder audit (tests/test_align_audit_cpu.py proves
them without a GPU, tests/test_align_audit_gpu.py runs the kernels against them).  Pure numpy / Python.

1. fcp_estimate_transform
-------------------------
``exact_transform`` solves the least-squares similarity / affine in rational arithmetic on the float32 inputs taken as
exact values and rounds each of the six results to float64 once.  ``kernel_order_f64`` restates the kernel's operation
order in numpy float64 (vectorised over faces, sequential over points).  ``transform_bound`` is a first-order forward
error bound of that order, u = 2^-53, k points, derived as follows (hats are computed values):

* mean: k - 1 sequential additions and one division, every partial sum at most S|x| = sum |x_p|:
  |mx^ - mx| <= k u S|x| / k = u S|x| =: e_m (likewise my, MX, MY).
* centred value: x^_p = fl(x_p - mx^), |x^_p - (x_p - mx)| <= e_m + u |x_p - mx| =: ex_p.
* a centred sum of products T = sum_p t_p, t_p = x_p X_p (+ y_p Y_p for the similarity's sums): one rounding per product,
  one for the inner addition, at most k for the accumulation, plus the perturbation of the factors:
  e_T = (k + 2) u sum_p |terms| + sum_p (|X_p| ex_p + |x_p| eX_p [+ |Y_p| ey_p + |y_p| eY_p]).
* similarity: a = sa / sxx: e_a = (e_sa + |a| e_sxx) / sxx + u |a|  (numerator, denominator, the division); b likewise.
* affine: det = sxx syy - sxy^2, two products and a subtraction:
  e_det = 2 u (sxx syy + sxy^2) + syy e_sxx + sxx e_syy + 2 |sxy| e_sxy;
  numerator N = sxX syy - syX sxy: e_N = 2 u (|sxX syy| + |syX sxy|) + syy e_sxX + |sxX| e_syy + |sxy| e_syX + |syX| e_sxy;
  a = N / det: e_a = (e_N + |a| e_det) / |det| + u |a|; b, c, d likewise.  The bound grows like 1 / (determinant ratio).
* translation m2 = MX - p mx - q my (p, q the row's coefficients, signs as written in the kernel), four roundings on
  terms of size |MX|, |p mx|, |q my|, plus the coefficient errors times |mean| and the mean errors times |coefficient|:
  e_m2 = 4 u (|MX| + |p mx| + |q my|) + e_MX + |mx| e_p + |p| e_mx + |my| e_q + |q| e_my.

Second-order terms are below (k + 2) u / ratio times the bound, under 1e-3 of it for every case here; the factor
``SECOND_ORDER`` = 1 + 2^-8 covers them.  Nothing in the bound is taken from a kernel's output.

2. warps
--------
``warp_launches`` is the one edge list every warp kernel sees; ``warp_reference`` evaluates it with the existing oracles
(``oracle.align_ref.warp_affine`` and tests/warp_interp_ref.py).  ``warp_any`` restates all four families in one function
with two hooks for planted mistakes (border index, all-constant early-out); un-planted it must equal the oracles.

3. batch builder and level builder
----------------------------------
``level_cases`` / ``batch_scenes`` build the geometries, ``exact_area`` is the float64 box filter.
"""
from __future__ import annotations

import functools
import importlib.util
import math
import os
from fractions import Fraction

import numpy as np

from oracle import align_ref as A, batch_ref as B


def _load(name, fname):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


W = _load("_warp_interp_ref_for_audit", "warp_interp_ref.py")

U = 2.0 ** -53
SECOND_ORDER = 1.0 + 2.0 ** -8
DET_THRESHOLD = 1e-12


# ===================================================================================================== 1. transforms
def exact_transform(src, dst, allow_skew):
    """src (k,2), dst (k,2) float32 -> dict(m: (6,) float64 or None, accept: bool, ratio: exact |det| / (sxx syy) as a
    float (affine; None when sxx syy == 0), sxx: exact centred sum as a float (similarity))."""
    s = np.asarray(src, np.float32)
    d = np.asarray(dst, np.float32)
    if not np.isfinite(s).all():
        return {"m": None, "accept": False, "ratio": None, "sxx": None}
    k = len(s)
    fx = [Fraction(float(v)) for v in s[:, 0]]; fy = [Fraction(float(v)) for v in s[:, 1]]
    fX = [Fraction(float(v)) for v in d[:, 0]]; fY = [Fraction(float(v)) for v in d[:, 1]]
    mx, my, MX, MY = sum(fx) / k, sum(fy) / k, sum(fX) / k, sum(fY) / k
    x = [v - mx for v in fx]; y = [v - my for v in fy]
    X = [v - MX for v in fX]; Y = [v - MY for v in fY]
    dot = lambda p, q: sum(a * b for a, b in zip(p, q))
    if not allow_skew:
        sxx = dot(x, x) + dot(y, y)
        if sxx <= 0:
            return {"m": None, "accept": False, "ratio": None, "sxx": 0.0}
        a = (dot(x, X) + dot(y, Y)) / sxx
        b = (dot(x, Y) - dot(y, X)) / sxx
        m = [a, -b, MX - a * mx + b * my, b, a, MY - b * mx - a * my]
        return {"m": np.array([float(v) for v in m]), "accept": True, "ratio": None, "sxx": float(sxx)}
    sxx, sxy, syy = dot(x, x), dot(x, y), dot(y, y)
    det = sxx * syy - sxy * sxy
    if sxx * syy == 0:
        return {"m": None, "accept": False, "ratio": None, "sxx": float(sxx)}
    ratio = abs(det) / (sxx * syy)
    if det == 0:
        return {"m": None, "accept": False, "ratio": 0.0, "sxx": float(sxx)}
    sxX, syX, sxY, syY = dot(x, X), dot(y, X), dot(x, Y), dot(y, Y)
    a = (sxX * syy - syX * sxy) / det; b = (syX * sxx - sxX * sxy) / det
    c = (sxY * syy - syY * sxy) / det; e = (syY * sxx - sxY * sxy) / det
    m = [a, b, MX - a * mx - b * my, c, e, MY - c * mx - e * my]
    return {"m": np.array([float(v) for v in m]), "accept": bool(ratio > Fraction(DET_THRESHOLD)), "ratio": float(ratio),
            "sxx": float(sxx)}


def _means(s, d):
    f, k = s.shape[:2]
    mx = np.zeros(f); my = np.zeros(f); MX = 0.0; MY = 0.0
    for p in range(k):
        mx = mx + s[:, p, 0]; my = my + s[:, p, 1]; MX = MX + d[p, 0]; MY = MY + d[p, 1]
    return mx / k, my / k, MX / k, MY / k


def kernel_order_f64(src, dst, allow_skew, centred_dtype=np.float64, centre=True):
    """The kernel's operation order in numpy float64: src (f,k,2) float32, dst (k,2) float32 -> (mat (f,6) float64, ok (f,)
    int32); rejected rows are all zero.  ``centred_dtype=np.float32`` and ``centre=False`` are the two planted mistakes of
    the CPU test (float32 accumulation of the centred sums; uncentred normal equations)."""
    src = np.asarray(src, np.float32)
    s = src.astype(np.float64)
    d = np.asarray(dst, np.float32).astype(np.float64)
    f, k = s.shape[:2]
    finite = np.isfinite(s).all((1, 2))
    T = centred_dtype
    with np.errstate(all="ignore"):
        mx, my, MX, MY = _means(s, d)
        if not centre:
            return _uncentred(s, d, allow_skew, finite)
        z = lambda: np.zeros(f, T)
        m = np.zeros((f, 6))
        if not allow_skew:
            sxx, sa, sb = z(), z(), z()
            for p in range(k):
                x, y = (s[:, p, 0] - mx).astype(T), (s[:, p, 1] - my).astype(T)
                X, Y = T(d[p, 0] - MX), T(d[p, 1] - MY)
                sxx = sxx + (x * x + y * y)
                sa = sa + (x * X + y * Y)
                sb = sb + (x * Y - y * X)
            sxx, sa, sb = sxx.astype(np.float64), sa.astype(np.float64), sb.astype(np.float64)
            good = finite & (sxx > 0.0)
            a, b = sa / sxx, sb / sxx
            m[:, 0] = a; m[:, 1] = -b; m[:, 2] = MX - a * mx + b * my
            m[:, 3] = b; m[:, 4] = a; m[:, 5] = MY - b * mx - a * my
        else:
            sxx, sxy, syy, sxX, syX, sxY, syY = z(), z(), z(), z(), z(), z(), z()
            for p in range(k):
                x, y = (s[:, p, 0] - mx).astype(T), (s[:, p, 1] - my).astype(T)
                X, Y = T(d[p, 0] - MX), T(d[p, 1] - MY)
                sxx = sxx + x * x; sxy = sxy + x * y; syy = syy + y * y
                sxX = sxX + x * X; syX = syX + y * X; sxY = sxY + x * Y; syY = syY + y * Y
            sxx, sxy, syy, sxX, syX, sxY, syY = (v.astype(np.float64) for v in (sxx, sxy, syy, sxX, syX, sxY, syY))
            det = sxx * syy - sxy * sxy
            good = finite & (np.abs(det) > DET_THRESHOLD * (sxx * syy + 1e-300))
            a = (sxX * syy - syX * sxy) / det; b = (syX * sxx - sxX * sxy) / det
            c = (sxY * syy - syY * sxy) / det; e = (syY * sxx - sxY * sxy) / det
            m[:, 0] = a; m[:, 1] = b; m[:, 2] = MX - a * mx - b * my
            m[:, 3] = c; m[:, 4] = e; m[:, 5] = MY - c * mx - e * my
        good = good & np.isfinite(m).all(1)
    m[~good] = 0.0
    return m, good.astype(np.int32)


def _uncentred(s, d, allow_skew, finite):
    """Planted mistake: the same least-squares problem through its uncentred normal equations (float64)."""
    f, k = s.shape[:2]
    m = np.zeros((f, 6))
    ok = np.zeros(f, np.int32)
    for i in range(f):
        if not finite[i]:
            continue
        x, y = s[i, :, 0], s[i, :, 1]
        if allow_skew:
            J = np.stack([x, y, np.ones(k)], 1)
            N = J.T @ J
            try:
                m[i, :3] = np.linalg.solve(N, J.T @ d[:, 0]); m[i, 3:] = np.linalg.solve(N, J.T @ d[:, 1])
            except np.linalg.LinAlgError:
                continue
        else:
            J = np.zeros((2 * k, 4))
            J[0::2] = np.stack([x, -y, np.ones(k), np.zeros(k)], 1)
            J[1::2] = np.stack([y, x, np.zeros(k), np.ones(k)], 1)
            try:
                h = np.linalg.solve(J.T @ J, J.T @ d.reshape(-1))
            except np.linalg.LinAlgError:
                continue
            m[i] = [h[0], -h[1], h[2], h[1], h[0], h[3]]
        ok[i] = 1
    return m, ok


def transform_bound(src, dst, allow_skew):
    """(6,) float64 bound of |kernel_order_f64 - exact_transform| for one accepted face, from the module docstring."""
    s = np.asarray(src, np.float32).astype(np.float64)
    d = np.asarray(dst, np.float32).astype(np.float64)
    k = len(s)
    mx, my, MX, MY = s[:, 0].mean(), s[:, 1].mean(), d[:, 0].mean(), d[:, 1].mean()
    e_mx, e_my = U * np.abs(s[:, 0]).sum(), U * np.abs(s[:, 1]).sum()
    e_MX, e_MY = U * np.abs(d[:, 0]).sum(), U * np.abs(d[:, 1]).sum()
    x, y, X, Y = s[:, 0] - mx, s[:, 1] - my, d[:, 0] - MX, d[:, 1] - MY
    ex, ey, eX, eY = e_mx + U * np.abs(x), e_my + U * np.abs(y), e_MX + U * np.abs(X), e_MY + U * np.abs(Y)

    def esum(*pairs):
        """Error of sum_p of the products (p, ep, q, eq) added up."""
        mag = sum(np.abs(p * q) for p, _, q, _ in pairs).sum()
        pert = sum((np.abs(q) * ep + np.abs(p) * eq) for p, ep, q, eq in pairs).sum()
        return (k + 2) * U * mag + pert

    def trans(M0, e_M0, p, e_p, q, e_q):
        return (4 * U * (abs(M0) + abs(p * mx) + abs(q * my)) + e_M0 + abs(mx) * e_p + abs(p) * e_mx + abs(my) * e_q
                + abs(q) * e_my)

    if not allow_skew:
        sxx, sa, sb = (x * x + y * y).sum(), (x * X + y * Y).sum(), (x * Y - y * X).sum()
        e_sxx = esum((x, ex, x, ex), (y, ey, y, ey))
        e_sa = esum((x, ex, X, eX), (y, ey, Y, eY))
        e_sb = esum((x, ex, Y, eY), (y, ey, X, eX))
        a, b = sa / sxx, sb / sxx
        e_a = (e_sa + abs(a) * e_sxx) / sxx + U * abs(a)
        e_b = (e_sb + abs(b) * e_sxx) / sxx + U * abs(b)
        out = [e_a, e_b, trans(MX, e_MX, a, e_a, b, e_b), e_b, e_a, trans(MY, e_MY, b, e_b, a, e_a)]
        return np.array(out) * SECOND_ORDER
    sxx, sxy, syy = (x * x).sum(), (x * y).sum(), (y * y).sum()
    sxX, syX, sxY, syY = (x * X).sum(), (y * X).sum(), (x * Y).sum(), (y * Y).sum()
    e_sxx, e_sxy, e_syy = esum((x, ex, x, ex)), esum((x, ex, y, ey)), esum((y, ey, y, ey))
    e_sxX, e_syX, e_sxY, e_syY = esum((x, ex, X, eX)), esum((y, ey, X, eX)), esum((x, ex, Y, eY)), esum((y, ey, Y, eY))
    det = sxx * syy - sxy * sxy
    e_det = 2 * U * (sxx * syy + sxy * sxy) + syy * e_sxx + sxx * e_syy + 2 * abs(sxy) * e_sxy

    def coef(n1, e_n1, d1, e_d1, n2, e_n2, d2, e_d2):
        """(n1 d1 - n2 d2) / det and its error."""
        num = n1 * d1 - n2 * d2
        e_num = (2 * U * (abs(n1 * d1) + abs(n2 * d2)) + abs(d1) * e_n1 + abs(n1) * e_d1 + abs(d2) * e_n2
                 + abs(n2) * e_d2)
        v = num / det
        return v, (e_num + abs(v) * e_det) / abs(det) + U * abs(v)

    a, e_a = coef(sxX, e_sxX, syy, e_syy, syX, e_syX, sxy, e_sxy)
    b, e_b = coef(syX, e_syX, sxx, e_sxx, sxX, e_sxX, sxy, e_sxy)
    c, e_c = coef(sxY, e_sxY, syy, e_syy, syY, e_syY, sxy, e_sxy)
    e, e_e = coef(syY, e_syY, sxx, e_sxx, sxY, e_sxY, sxy, e_sxy)
    out = [e_a, e_b, trans(MX, e_MX, a, e_a, b, e_b), e_c, e_e, trans(MY, e_MY, c, e_c, e, e_e)]
    return np.array(out) * SECOND_ORDER


def _near_line(delta):
    """Five points on y = x, x = (-2..2) * 1024, with y[0] += delta, y[1] -= delta: all sums exact in float64 for
    delta >= 2^-12 and the exact determinant ratio is 19 * 2^20 delta^2 / (sxx syy) ~ 0.19 delta^2 / 2^20."""
    x = np.array([-2, -1, 0, 1, 2], np.float64) * 1024
    y = x.copy()
    y[0] += delta; y[1] -= delta
    pts = np.stack([x, y], 1).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64), np.stack([x, y], 1))          # exactly representable
    return pts


# determinant ratios of the nearly collinear rows: ~2.9e-6, ~1.8e-10 (accepted) and ~1.1e-14 (rejected: 92x below the
# threshold, while the kernel's own det error is <= 2 u (sxx syy + sxy^2) ~ 0.05 against a threshold of ~110 absolute)
NEAR_LINE_DELTAS = (4.0, 2.0 ** -5, 2.0 ** -12)
RATIO_MARGIN = 10.0          # every case's exact ratio is outside [threshold / 10, threshold * 10]


@functools.lru_cache(maxsize=None)
def transform_cases():
    """[(name, src (f,k,2) float32, dst (k,2) float32)]; both allow_skew values run on each."""
    rng = np.random.default_rng(20240)
    tgt5 = A.landmarks_target((112, 112), 0.65)
    cases = []

    def faces(f, k, lo, hi, spread=None):
        if spread is None:
            return rng.uniform(lo, hi, (f, k, 2)).astype(np.float32)
        c = rng.uniform(lo, hi - spread, (f, 1, 2))
        return (c + rng.uniform(0, spread, (f, k, 2))).astype(np.float32)

    for f in (1, 63, 64, 65, 200):                         # valid and invalid rows interleaved
        s = faces(f, 5, 0, 640)
        bad = (np.arange(f) % 3 == 1) if f > 1 else np.zeros(1, bool)
        s[bad] = s[bad][:, :1]                            # k identical points: rejected by both
        if f > 4:
            s[3, 2, 1] = np.nan                           # a NaN in an otherwise valid row
        cases.append((f"f{f}", s, tgt5))
    for k in (2, 3, 68, 128):
        tgt = tgt5 if k == 5 else rng.uniform(10, 100, (k, 2)).astype(np.float32)
        s = faces(8, k, 0, 640)
        s[3] = s[3][:1]                                    # identical points
        cases.append((f"k{k}", s, tgt))
    cases.append(("full_res", faces(16, 5, 30000, 32767), tgt5))
    cases.append(("full_res_small", faces(8, 5, 30000, 32767, spread=40.0), tgt5))
    cases.append(("under_2px", faces(16, 5, 100, 600, spread=2.0), tgt5))
    line = np.stack([np.arange(5) * 7 + 3, np.arange(5) * 14 - 5], 1).astype(np.float32)    # exactly collinear integers
    special = [line] + [_near_line(dl) for dl in NEAR_LINE_DELTAS]
    for bad in (np.nan, np.inf, -np.inf):
        s = faces(1, 5, 0, 640)[0]
        s[3, 0] = bad
        special.append(s)
    special.append(faces(1, 5, 0, 640)[0])
    cases.append(("special", np.stack(special), tgt5))
    return cases


@functools.lru_cache(maxsize=None)
def transform_expected(name, allow_skew):
    """(exact (f,6) float64 with zeros for rejected rows, accept (f,) bool, bound (f,6) with inf for rejected rows,
    ratios list) of one case."""
    src, dst = next((s, d) for n, s, d in transform_cases() if n == name)
    f = len(src)
    exact, accept, bound, ratios = np.zeros((f, 6)), np.zeros(f, bool), np.full((f, 6), np.inf), []
    for i in range(f):
        r = exact_transform(src[i], dst, allow_skew)
        ratios.append(r["ratio"])
        accept[i] = r["accept"]
        if r["accept"]:
            exact[i] = r["m"]
            bound[i] = transform_bound(src[i], dst, allow_skew)
    return exact, accept, bound, ratios


# ========================================================================================================== 2. warps
FAMILIES = ("fixed", "float32", "cubic", "lanczos4")
BORDERS = {"constant": 0, "replicate": 1, "reflect": 2, "wrap": 3, "reflect_101": 4}
TAPS = {"fixed": 2, "float32": 2, "cubic": 4, "lanczos4": 8}
OUT_SIZES = [(1, 1), (2, 3), (3, 1), (4, 1), (5, 2), (7, 5), (8, 8), (64, 1), (48, 64)]     # (w, h)
SHORT_RANGE = [[0.001, 0, 0, 0, -0.002, 0], [0.0007, 0.0003, 2.5, -0.0003, 0.0007, 31.7], [1, 0, 40000.5, 0, 1, -40000.25]]
# inverse coefficients of 1e7 (cv_round(. * 1024) saturates) and of 1.5e6 with an offset of 1e6 (X0 + adelta wraps)
SATURATING = [[1e-7, 0, 0, 0, 1e-7, 0], [1 / 1.5e6, 0, -2 / 3, 0, 1 / 1.5e6, 1 / 3], [2e-7, 1e-7, 3.5, -1e-7, 2e-7, -1.25]]
SINGULAR = [[1, 2, 3, 2, 4, 5], [0, 0, 0, 0, 0, 0]]
NON_FINITE = [[np.nan, 0, 0, 0, 1, 0], [1, 0, np.inf, 0, 1, 0], [1, 0, 0, 0, 1, -np.inf], [1, 0, 0, np.inf, 1, 0],
              [np.nan] * 6]


def _sim(s, th, tx=0.0, ty=0.0):
    a, b = s * math.cos(th), s * math.sin(th)
    return np.array([a, -b, tx, b, a, ty], np.float64)


def _centred(s, th, hw, wh, dx=0.0, dy=0.0):
    M = _sim(s, th).reshape(2, 3)
    c = M[:, :2] @ np.array([(hw[1] - 1) / 2 + dx, (hw[0] - 1) / 2 + dy])
    M[:, 2] = np.array([(wh[0] - 1) / 2, (wh[1] - 1) / 2]) - c
    return M.reshape(6)


def _shift(tx, ty):
    return np.array([1, 0, tx, 0, 1, ty], np.float64)


def face_matrices(hw, wh):
    """The finite, well-conditioned matrices every family sees for a (h, w) slice and a (w, h) output."""
    sh, sw = hw
    ow, oh = wh
    K = 8
    mats = [_shift(0, 0), _shift(2, -1), _shift(0.37, -0.61), _shift(-(sw - ow), -(sh - oh)),          # corner to corner
            _shift(-(sw - ow) - 0.5, -(sh - oh) - 0.25),
            _centred(0.25, 0.1, hw, wh, 0.3, -0.2), _centred(1.7, 0.45, hw, wh, 0.37, 0.61), _centred(6.0, 1.2, hw, wh, -0.45, 0.3),
            # wholly outside on each side (beyond every family's taps)
            _shift(ow + K + 2, 0), _shift(-(sw + K + 2), 0), _shift(0, oh + K + 2), _shift(0, -(sh + K + 2)),
            # straddling each edge by less than one tap
            _shift(0.5, 0), _shift(-(sw - ow) - 0.5, 0), _shift(0, 0.75), _shift(0, -(sh - oh) - 0.25)]
    return mats


@functools.lru_cache(maxsize=None)
def warp_scenes():
    """[(name, batch (n,H,W,3) u8, pads (n,4) int32 (t,b,l,r))]: the slice of image i is the source of its faces, in the
    batch through ``pads`` and in the ragged blob as an image of its own.  "main": slices 40x52, 1x1, 1x7, 7x1, 2x2, 3x5,
    7x9 and the whole last image; "wide": one 97 x 131 image; "tail0..3": three 9 x (12 + j) images, so that the batch's byte count is j mod 4."""
    rng = np.random.default_rng(77)
    main = rng.integers(0, 256, (8, 40, 52, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:40, 0:52]
    main[7] = np.stack([(xx * 5) % 256, (yy * 7) % 256, (xx * 3 + yy * 4) % 256], -1)
    pads = np.array([[0, 0, 0, 0], [20, 19, 30, 21], [39, 0, 45, 0], [0, 33, 0, 51], [38, 0, 50, 0], [10, 27, 4, 43],
                     [1, 32, 40, 3], [0, 0, 0, 0]], np.int32)
    scenes = [("main", main, pads)]
    scenes.append(("wide", rng.integers(0, 256, (1, 97, 131, 3), dtype=np.uint8), np.zeros((1, 4), np.int32)))
    for j in range(4):
        scenes.append((f"tail{j}", rng.integers(0, 256, (3, 9, 12 + j, 3), dtype=np.uint8),
                       np.array([[0, 0, 0, 0], [1, 0, 3, 0], [0, 0, 0, 0]], np.int32)))
    return scenes


def scene_slices(batch, pads):
    return [np.ascontiguousarray(batch[i, t:batch.shape[1] - b, l:batch.shape[2] - r]) for i, (t, b, l, r) in enumerate(pads)]


def ragged_blob(batch, pads):
    """The slices back to back behind one odd byte, ending exactly at the blob's end: (blob u8, srcs (n,3) int64)."""
    parts, srcs, off = [np.array([7], np.uint8)], [], 1
    for sl in scene_slices(batch, pads):
        srcs.append((off, sl.shape[0], sl.shape[1]))
        parts.append(sl.reshape(-1))
        off += sl.size
    return np.concatenate(parts), np.array(srcs, np.int64)


@functools.lru_cache(maxsize=None)
def warp_launches(family):
    """The edge list as launches: [(scene name, (w, h), img (f,) int32, mats (f,6) float64, ok (f,) int32 or None)].
    ``family`` only decides whether the saturating and non-finite matrices are included (not for float32)."""
    integer_path = family != "float32"
    out = []
    nan6 = np.full(6, np.nan)
    for name, batch, pads in warp_scenes():
        slices = scene_slices(batch, pads)
        last = len(slices) - 1
        if name == "main":
            for wh in OUT_SIZES:
                ordinary = wh == (48, 64)
                # f = 1: the last image, corner to corner with a fractional shift (the end of the allocation)
                hw = slices[last].shape[:2]
                out.append((name, wh, [last], [face_matrices(hw, wh)[4]], None))
                # f = 9: one face per slice, the matrix rotating through the list, one ok == 0 row with a NaN matrix
                idx, mats, ok = [], [], []
                for i, sl in enumerate(slices):
                    fm = face_matrices(sl.shape[:2], wh)
                    idx.append(i); mats.append(fm[(i * 5 + wh[0]) % len(fm)]); ok.append(1)
                idx.append(0); mats.append(nan6); ok.append(0)
                out.append((name, wh, idx, mats, ok))
                if ordinary or wh == (7, 5):
                    # every matrix on the large, the 7x9 and the last slice; the small slices take them in turn
                    idx, mats, ok = [], [], []
                    for i in (0, 6, last):
                        for m in face_matrices(slices[i].shape[:2], wh):
                            idx.append(i); mats.append(m); ok.append(1)
                    out.append((name, wh, idx, mats, ok))
                    idx, mats, ok = [], [], []
                    for j, m in enumerate(face_matrices((7, 9), wh)):
                        for i in (1, 2, 3, 4, 5):
                            if (i + j) % 2 == 0:
                                idx.append(i); mats.append(face_matrices(slices[i].shape[:2], wh)[j]); ok.append(1)
                        if j % 5 == 0:
                            idx.append(j % 8); mats.append(nan6); ok.append(0)
                    out.append((name, wh, idx, mats, ok))
                if wh in ((7, 5), (8, 8)):
                    # ok == NULL: the singular and the zero matrix (and, integer families, the all-NaN one) on every slice
                    ms = SINGULAR + ([NON_FINITE[-1]] if integer_path else [])
                    idx = [i for i in range(len(slices)) for _ in ms]
                    out.append((name, wh, idx, [np.array(m, np.float64) for _ in slices for m in ms], None))
        elif name == "wide":
            # ok == NULL: short-range and (integer families) saturating / non-finite matrices.  They send taps to +-32768,
            # where the reference's reflect loop needs 32768 / side passes: hence the widest source and small outputs.
            ms = SINGULAR + SHORT_RANGE + (SATURATING + NON_FINITE if integer_path else [])
            out.append((name, (7, 5), [0] * len(ms), [np.array(m, np.float64) for m in ms], None))
            ms = [SHORT_RANGE[2]] + (SATURATING[1:2] + NON_FINITE[1:2] if integer_path else [])      # the packed store
            out.append((name, (8, 8), [0] * len(ms), [np.array(m, np.float64) for m in ms], None))
        else:
            for wh in ((8, 8), (7, 5), (4, 1), (16, 9)):
                idx, mats = [], []
                for i in (last, 1):
                    hw = slices[i].shape[:2]
                    fm = face_matrices(hw, wh)
                    for m in (fm[0], fm[3], fm[4], _shift(-(hw[1] - wh[0]) + 0.25, -(hw[0] - wh[1]) + 0.5)):
                        idx.append(i); mats.append(m)
                out.append((name, wh, idx, mats, None))
    return [(n, wh, np.array(i, np.int32), np.stack(m).reshape(-1, 6), None if o is None else np.array(o, np.int32))
            for n, wh, i, m, o in out]


def oracle_warp(img, M, wh, border, family):
    """The existing oracle of one family."""
    with np.errstate(all="ignore"):
        if family in ("fixed", "float32"):
            return A.warp_affine(img, np.asarray(M).reshape(2, 3), wh, border, variant=family)
        return W.warp_affine_interp(img, np.asarray(M).reshape(2, 3), wh, border, W.INTERP[family])


@functools.lru_cache(maxsize=None)
def warp_reference(family, border):
    """Expected bytes of every launch of ``warp_launches(family)``: a list of (f, h, w, 3) uint8, shared by the batch and
    ragged sources and by both boundaries."""
    scenes = {n: scene_slices(b, p) for n, b, p in warp_scenes()}
    return [launch_reference(scenes[name], wh, idx, mats, ok, border, family, oracle_warp)
            for name, wh, idx, mats, ok in warp_launches(family)]


def launch_reference(slices, wh, idx, mats, ok, border, family, fn):
    ref = np.zeros((len(idx), wh[1], wh[0], 3), np.uint8)
    for j in range(len(idx)):
        if ok is None or ok[j]:
            ref[j] = fn(slices[idx[j]], mats[j], wh, border, family)
    return ref


def _inverse(M):
    m = np.asarray(M, np.float64).reshape(6).copy()
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[4] * D, m[0] * D
    m[0] = A11; m[1] *= -D; m[3] *= -D; m[4] = A22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def planted_border_index(p, n, border):
    """cv::borderInterpolate with an off-by-one: constant takes p == n for inside, replicate clamps to n - 2, reflect and
    reflect_101 swap their deltas, wrap is shifted by one past the end."""
    p = np.asarray(p, np.int64)
    if border == 0:
        return np.where((p >= 0) & (p <= n), np.minimum(p, n - 1), -1)
    if border == 1:
        return np.clip(p, 0, max(n - 2, 0))
    if border in (2, 4):
        return A.border_interpolate(p, n, 6 - border)
    return np.where(p >= n, np.mod(p + 1, n), np.mod(p, n))


def warp_any(img, M, wh, border, family, plant=None):
    """All four families in one restatement: coordinates (fixed point or float32), K taps a side through the border
    index, the family's blend, the all-constant early-out.  ``plant``: None, "border" (``planted_border_index``) or
    "early_out" (the constant border's all-outside test one pixel too eager: sx + K - 1 <= 0 instead of sx + K <= 0)."""
    img = np.asarray(img, np.uint8)
    sh, sw = img.shape[:2]
    ow, oh = wh
    K = TAPS[family]
    f32 = np.float32
    with np.errstate(all="ignore"):
        if family == "float32":
            m = _inverse(M).astype(f32)
            xs, ys = np.arange(ow, dtype=f32)[None, :], np.arange(oh, dtype=f32)[:, None]
            sxf = (xs * m[0] + (ys * m[1] + m[2]).astype(f32)).astype(f32)
            syf = (xs * m[3] + (ys * m[4] + m[5]).astype(f32)).astype(f32)
            ixf, iyf = np.floor(sxf), np.floor(syf)
            ax, ay = (sxf - ixf).astype(f32)[..., None], (syf - iyf).astype(f32)[..., None]
            sx, sy = np.clip(ixf, -32768, 32767).astype(np.int64), np.clip(iyf, -32768, 32767).astype(np.int64)
        else:
            X, Y = W.source_coords(np.asarray(M, np.float64).reshape(2, 3), wh)
            sx = np.clip(X >> 5, -32768, 32767) - (K // 2 - 1)
            sy = np.clip(Y >> 5, -32768, 32767) - (K // 2 - 1)
    bi = planted_border_index if plant == "border" else A.border_interpolate
    cols = [bi(sx + k, sw, border) for k in range(K)]
    rows = [bi(sy + r, sh, border) for r in range(K)]

    def tap(r, k, dtype):
        okm = (rows[r] >= 0) & (cols[k] >= 0)
        v = img[np.where(okm, rows[r], 0), np.where(okm, cols[k], 0)].astype(dtype)
        return np.where(okm[..., None], v, dtype(0))

    if family == "float32":
        p00, p01, p10, p11 = tap(0, 0, f32), tap(0, 1, f32), tap(1, 0, f32), tap(1, 1, f32)
        v0 = (p00 + ax * (p01 - p00)).astype(f32)
        v1 = (p10 + ax * (p11 - p10)).astype(f32)
        out = np.clip(np.rint((v0 + ay * (v1 - v0)).astype(f32)), 0, 255).astype(np.uint8)
    else:
        fx, fy = X & 31, Y & 31
        if family == "fixed":
            wt = np.stack([np.stack([(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32], -1),
                           np.stack([fy * (32 - fx) * 32, fy * fx * 32], -1)], -2)                 # (oh, ow, r, k)
        else:
            wt = W._weights(W.INTERP[family])[fy * 32 + fx]
        acc = np.zeros(sx.shape + (3,), np.int64)
        for r in range(K):
            for k in range(K):
                acc += tap(r, k, np.int64) * wt[..., r, k][..., None]
        out = np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
    if border == 0:
        lim = K - 1 if plant == "early_out" else K
        out[(sx >= sw) | (sx + lim <= 0) | (sy >= sh) | (sy + lim <= 0)] = 0
    return out


def resample_f64(img, M, wh, family):
    """float64 resampling of the float64 inverse map with replicated edges: bilinear, Keys cubic (A = -0.75) or Lanczos-4
    (weights normalised to sum 1).  -> ((oh, ow, 3) float64, sx, sy float64 source coordinates)."""
    img = np.asarray(img, np.float64)
    sh, sw = img.shape[:2]
    Minv = np.linalg.inv(np.vstack([np.asarray(M, np.float64).reshape(2, 3), [0, 0, 1]]))[:2]
    ys, xs = np.mgrid[0:wh[1], 0:wh[0]].astype(np.float64)
    sx = Minv[0, 0] * xs + Minv[0, 1] * ys + Minv[0, 2]
    sy = Minv[1, 0] * xs + Minv[1, 1] * ys + Minv[1, 2]
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    K = TAPS[family]
    taps = np.arange(K) - (K // 2 - 1)
    if K == 2:
        kern = lambda d: np.clip(1 - np.abs(d), 0, None)
    else:
        kern = lambda d: W.kernel_f64(W.INTERP[family], d)
    wx, wy = kern((sx - x0)[..., None] - taps), kern((sy - y0)[..., None] - taps)
    wx /= wx.sum(-1, keepdims=True); wy /= wy.sum(-1, keepdims=True)
    acc = np.zeros(sx.shape + (3,))
    for r in range(K):
        for k in range(K):
            v = img[np.clip(y0 + taps[r], 0, sh - 1), np.clip(x0 + taps[k], 0, sw - 1)]
            acc += v * (wy[..., r] * wx[..., k])[..., None]
    return acc, sx, sy


# ===================================================================================== 3. batch builder, level builder
# (sw, sh) -> (dw, dh), ordered large, tiny, large
LEVEL_CASES = [((135, 240), (36, 64)),      # non-integral on both axes
               ((7, 5), (1, 1)),            # one destination pixel
               ((64, 90), (32, 40)),        # integral in x, non-integral in y: the general-table path
               ((3, 9), (1, 5)),            # dw = 1, npx % 4 == 1
               ((5, 7), (2, 3)),            # dw = 2, npx % 4 == 2
               ((7, 5), (3, 1)),            # dw = 3, npx % 4 == 3
               ((11, 9), (5, 4)),           # dw = 5, npx % 4 == 0
               ((13, 7), (13, 7)),          # same size: copy
               ((20, 14), (10, 7)), ((21, 15), (7, 5)), ((36, 24), (9, 12)),      # integral 2x2, 3x3, 4x2
               ((63, 40), (21, 17)),        # integral in x, non-integral in y
               ((41, 53), (40, 52)),        # ratios just above 1
               ((100, 37), (33, 17))]       # the last x cell is clipped by ssize - fsx1
MIXED_AND_CLIPPED = [((64, 90), (32, 40)), ((63, 40), (21, 17)), ((100, 37), (33, 17))]


def level_image(k):
    (sw, sh), _ = LEVEL_CASES[k]
    return np.random.default_rng(500 + k).integers(0, 256, (sh, sw, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def level_plan():
    """-> (src blob u8 with the sources back to back behind one odd byte and ending at its end, levels (n,6) int64 of
    (src_off, sh, sw, dst_off, dh, dw), dst bytes, expected [(dst_off, (dh,dw,3) u8)]).  Destinations are 16 bytes or more
    apart, the first 16 bytes in, and 16 bytes are left after the last."""
    parts, levels, exp, off, pos = [np.array([9], np.uint8)], [], [], 1, 16
    for k, ((sw, sh), (dw, dh)) in enumerate(LEVEL_CASES):
        img = level_image(k)
        parts.append(img.reshape(-1))
        levels.append((off, sh, sw, pos, dh, dw))
        exp.append((pos, B.resize_u8(img, dw, dh, "area")))
        off += img.size
        pos = (pos + dh * dw * 3 + 3) // 4 * 4 + 16
    return np.concatenate(parts), np.array(levels, np.int64), pos, exp


def exact_area(img, dw, dh):
    """float64 box filter: every destination pixel is the mean of the source over its (scale_x x scale_y) cell."""
    sh, sw = img.shape[:2]

    def weights(ss, ds):
        scale = ss / ds
        Wt = np.zeros((ds, ss))
        for d in range(ds):
            a, b = d * scale, min((d + 1) * scale, ss)
            for s in range(int(np.floor(a)), int(np.ceil(b))):
                Wt[d, s] = max(0.0, min(b, s + 1) - max(a, s))
            Wt[d] /= Wt[d].sum()
        return Wt
    return np.einsum("ys,stc,xt->yxc", weights(sh, dh), img.astype(np.float64), weights(sw, dw))


AREA_BOUND = 0.5 + 2e-3        # float32 tables against float64, as tests/test_batch_oracle.py


def planted_area_fast_path(img, dw, dh):
    """Planted mistake: the integral box-sum path taken although only one axis is integral (the other ratio rounded)."""
    sh, sw = img.shape[:2]
    isx, isy = int(np.rint(sw / dw)), int(np.rint(sh / dh))
    out = np.zeros((dh, dw, 3), np.uint8)
    inv = np.float32(1.0) / np.float32(isx * isy)
    for y in range(dh):
        for x in range(dw):
            cell = img[min(y * isy, sh - 1):y * isy + isy, min(x * isx, sw - 1):x * isx + isx].astype(np.int64).sum((0, 1))
            out[y, x] = np.clip(np.rint(cell.astype(np.float32) * inv), 0, 255)
    return out


def _items_for(W_, H_, rng):
    """Nine items (source (sw, sh), (dw, dh), interp 0 cubic / 1 area) that fit a (W_, H_) slot: copy, cubic from 1x1, 1x9
    and 2x2 sources, cubic enlarging x while shrinking y, area 2x2, 4x2, mixed integral / non-integral and general;
    destinations of one pixel a side where the slot allows."""
    h2, w2 = max(1, H_ // 2), max(1, W_ // 2)
    w4 = max(1, W_ // 4)
    items = [((min(W_, 3), min(H_, 2)), (min(W_, 3), min(H_, 2)), 0),
             ((1, 1), (W_, H_), 0), ((1, 9), (min(W_, 4), H_), 0), ((2, 2), (W_, min(H_, 4)), 0),
             ((3, 2 * H_ + 1), (min(W_, 5), H_), 0),
             ((2 * w2, 2 * h2), (w2, h2), 1), ((4 * w4, 2 * h2), (w4, h2), 1),
             ((3 * w4, max(2 * h2 - 1, 1)), (w4, h2), 1), ((2 * w2 + 1, 2 * H_ + 1), (1, H_), 1)]
    return items


@functools.lru_cache(maxsize=None)
def batch_scenes():
    """[(name, W, H, images [(sh,sw,3) u8], items [(sw, sh, dw, dh, top, left, interp)])]: the four slot sizes that straddle
    the 64 x 4 thread tile with generated items, and one 43 x 66 slot holding the level builder's area cases."""
    rng = np.random.default_rng(900)
    scenes = []
    for W_, H_ in ((5, 3), (64, 4), (65, 5), (130, 9)):
        imgs, items = [], []
        for j, ((sw, sh), (dw, dh), interp) in enumerate(_items_for(W_, H_, rng)):
            imgs.append(rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8))
            top, left = ((H_ - dh) * (j % 3)) // 2, ((W_ - dw) * ((j + 1) % 3)) // 2
            items.append((sw, sh, dw, dh, top, left, interp))
        scenes.append((f"slot{W_}x{H_}", W_, H_, imgs, items))
    imgs, items = [], []
    for k, ((sw, sh), (dw, dh)) in enumerate(LEVEL_CASES):
        imgs.append(level_image(k))
        items.append((sw, sh, dw, dh, ((66 - dh) * (k % 3)) // 2, ((43 - dw) * ((k + 2) % 3)) // 2, 1))
    scenes.append(("area43x66", 43, 66, imgs, items))
    return scenes


def batch_expected(W_, H_, imgs, items, mode):
    """(n, H, W, 3) uint8 through oracle.batch_ref: resize, then copyMakeBorder into the slot."""
    out = np.zeros((len(items), H_, W_, 3), np.uint8)
    for i, (img, (sw, sh, dw, dh, top, left, interp)) in enumerate(zip(imgs, items)):
        r = B.resize_u8(img, dw, dh, "area" if interp == 1 else "cubic")
        t, b, l, rr = top, H_ - top - dh, left, W_ - left - dw
        if mode != "constant":          # batch_ref.border_index gives up after 64 reflections: make sure it got there
            for n, lo, hi in ((dh, -t, dh + b), (dw, -l, dw + rr)):
                q = B.border_index(np.arange(lo, hi), n, mode)
                assert ((q >= 0) & (q < n)).all()
        out[i] = B.copy_make_border(r, t, b, l, rr, mode)
    return out
