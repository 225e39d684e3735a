"""References of the RetinaFace post-processing kernels (test helper, not a test module).

``fcp_retina_post.hip`` decodes, thresholds, sorts, suppresses and selects in float32, op by op in the reference's order
(built with -ffp-contract=off, no fast-math).  This file restates each stage independently:

* ``priors64`` / ``score64`` / ``decode64``: PriorBox from exact rationals ``(j + 0.5) * step / w`` and ``min_size / w``,
  the two-class softmax and the box / landmark decode, all in float64.  tests/test_retina_post_ref_cpu.py checks them
  against a float64 ``torch`` evaluation of the reference's formulas and against ``oracle.retinaface_ref``.
* ``score_bound`` / ``decode_bound``: the largest |f32 - ref64| the kernel's float32 order can produce (``face_score`` and
  ``decode_prior``), 0.5 ulp (``U`` times the magnitude) per rounded op, derived next to each function.  ``expf`` is not
  correctly rounded: the bound allows ``EXP_ULP`` ulp for it (OCML documents 1 ulp for ``expf``; numpy's float32 ``exp``
  that the oracle uses is within 1 ulp too; 2 leaves room for both).  ``SLACK`` covers second-order terms.
* ``threshold_audit``: the strict ``score > vis`` decision against the float64 score and its bound.
* ``nms_audit``: an independent float64 check of a keep list: its order, and for every pair the float64 IoU with the
  error ``iou_delta`` of the float32 IoU formula.  Division is correctly rounded, so the float32 ``ovr <= thr`` test
  is exactly ``q < T`` on the unrounded quotient q, where T is the midpoint between ``thr`` and the next float32 (a
  midpoint rounds to the even one); only the rounding of the operations before the division blurs it (``iou_delta``),
  and operations whose exact result is a float32 (integer boxes) add no error, so IoU == 0.4 from integer boxes is
  decided exactly.
* ``largest_ref``: ``take_by_strategy("largest")``: ``torch.argmax`` of the +1-convention float32 areas (NaN is maximal).

The input generators at the end are shared by the CPU and GPU tests, so the planted-mistake checks run on the very inputs
the device sees.  Plain numpy / torch on the host; nothing here calls the library.
"""
from __future__ import annotations

from math import ceil

import numpy as np
import torch

f32, f64 = np.float32, np.float64
U = 2.0 ** -24           # float32 unit roundoff
SLACK = 1.01             # second-order terms of the first-order bounds below
EXP_ULP = 2              # ulp allowed for expf (device, OCML: 1 ulp) and np.exp (host, float32)
TINY = 2.0 ** -125       # absolute floor of the score bound: exp(d) for d < -87 is subnormal or zero in float32
STEPS = (8, 16, 32)
MIN_SIZES = ((16, 32), (64, 128), (256, 512))
VAR = (f32(0.1), f32(0.2))   # the variances as the kernel receives them (float32 arguments)


def prior_count(h: int, w: int) -> int:
    return sum(2 * ceil(h / s) * ceil(w / s) for s in STEPS)


# ------------------------------------------------------------------------------------------------------------- decode
def priors64(h: int, w: int, centre: float = 0.5) -> np.ndarray:
    """(P, 4) float64 (cx, cy, pw, ph): the exact rationals of PriorBox (``centre`` is the +0.5 of the cell centre)."""
    out = []
    for s, ms in zip(STEPS, MIN_SIZES):
        fh, fw = ceil(h / s), ceil(w / s)
        i = np.arange(fh, dtype=f64)[:, None, None]
        j = np.arange(fw, dtype=f64)[None, :, None]
        m = np.array(ms, dtype=f64)[None, None, :]
        out.append(np.stack([np.broadcast_to((j + centre) * s / w, (fh, fw, 2)),
                             np.broadcast_to((i + centre) * s / h, (fh, fw, 2)),
                             np.broadcast_to(m / w, (fh, fw, 2)), np.broadcast_to(m / h, (fh, fw, 2))], -1).reshape(-1, 4))
    return np.concatenate(out, 0)


def score64(logits: np.ndarray) -> np.ndarray:
    """softmax(logits)[..., 1] in float64: 1 / (1 + exp(l0 - l1))."""
    lg = logits.astype(f64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(lg[..., 0] - lg[..., 1]))


def score_bound(logits: np.ndarray) -> np.ndarray:
    """|face_score - score64|.  face_score: mx = max(l0, l1); d = RN(l_other - mx) <= 0 (|err| <= U|d|); E = expf(d)
    (relative error rE <= U|d| + 2 U EXP_ULP, one ulp <= 2 U relative); the other exponent is expf(0) = 1 exactly.
    l1 >= l0: s = RN(1 / RN(1 + E)), relative error <= E / (1 + E) rE + 2U.
    l0 > l1:  s = RN(E * RN(1 / RN(1 + E))), relative error <= rE / (1 + E) + 3U.
    l0 == l1: s = 1 / 2 exactly (bound 0).  ``TINY`` covers a subnormal or flushed E."""
    lg = logits.astype(f64)
    d = -np.abs(lg[..., 0] - lg[..., 1])
    s = score64(logits)
    E = np.exp(d)
    rE = U * np.abs(d) + 2 * U * EXP_ULP
    rel = np.where(lg[..., 1] >= lg[..., 0], E / (1 + E) * rE + 2 * U, rE / (1 + E) + 3 * U)
    return np.where(d == 0, 0.0, SLACK * rel * s + TINY)


def decode64(loc: np.ndarray, ldm: np.ndarray, pri: np.ndarray, h: int, w: int, var=VAR):
    """decode_bboxes / decode_landms + the (w, h) scaling in float64 -> boxes (..., 4), landmarks (..., 10)."""
    v0, v1 = f64(var[0]), f64(var[1])
    loc, ldm = loc.astype(f64), ldm.astype(f64)
    pxy, pwh = pri[:, :2], pri[:, 2:]
    cxy = pxy + loc[..., :2] * v0 * pwh
    with np.errstate(over="ignore"):
        wh = pwh * np.exp(loc[..., 2:] * v1)
    x1y1 = cxy - wh / 2
    boxes = np.concatenate([x1y1, x1y1 + wh], -1) * np.array([w, h, w, h], f64)
    pts = [pxy + ldm[..., 2 * k:2 * k + 2] * v0 * pwh for k in range(5)]
    return boxes, np.concatenate(pts, -1) * np.array([w, h] * 5, f64)


def decode_bound(loc: np.ndarray, ldm: np.ndarray, pri: np.ndarray, h: int, w: int, var=VAR):
    """|decode_prior - decode64| per output, in pixels.  Per axis (scale S = w or h, prior centre c, size p, all >= 0):
      c, p          = RN(exact rational)                          err U c, U p
      t             = RN(RN(b0 * v0) * p)                         err 3U |t|           (two roundings + the error of p)
      cx            = RN(c + t)                                   err U c + 3U|t| + U(c + |t|)
      bw            = RN(p * expf(RN(b2 * v1)))                   rel U|b2 v1| + 2U EXP_ULP + 2U
      x1            = RN(cx - bw / 2)     (/2 exact)              err e_cx + e_bw / 2 + U(|cx| + bw / 2)
      x2            = RN(bw + x1)                                 err e_bw + e_x1 + U(bw + |x1|)
      X             = RN(x * S)                                   err S e_x + U S |x|
      landmark      = RN(RN(c + t_k) * S)                         err S(U c + 3U|t_k| + U(c + |t_k|)) + U S (c + |t_k|)
    Magnitudes are bounded by c + |t| (+ bw / 2), so the bound grows with |loc| * var * prior size and with the frame."""
    v0, v1 = f64(var[0]), f64(var[1])
    loc, ldm = loc.astype(f64), ldm.astype(f64)
    bb = []
    for ax, S in ((0, w), (1, h)):
        c, p = pri[:, ax], pri[:, 2 + ax]
        t = np.abs(loc[..., ax] * v0 * p)
        e_cx = U * c + 3 * U * t + U * (c + t)
        with np.errstate(over="ignore"):
            bw = p * np.exp(loc[..., 2 + ax] * v1)
        e_bw = (U * np.abs(loc[..., 2 + ax] * v1) + 2 * U * EXP_ULP + 2 * U) * bw
        m_x1 = c + t + bw / 2
        e_x1 = e_cx + e_bw / 2 + U * m_x1
        e_x2 = e_bw + e_x1 + U * (bw + m_x1)
        bb.append((S * e_x1 + U * S * m_x1, S * e_x2 + U * S * (bw + m_x1)))
    box_b = SLACK * np.stack([bb[0][0], bb[1][0], bb[0][1], bb[1][1]], -1)
    lb = []
    for k in range(10):
        ax = k & 1
        S = w if ax == 0 else h
        c, p = pri[:, ax], pri[:, 2 + ax]
        t = np.abs(ldm[..., k] * v0 * p)
        lb.append(S * (U * c + 3 * U * t + U * (c + t)) + U * S * (c + t))
    return box_b, SLACK * np.stack(lb, -1)


def err_ratio(got: np.ndarray, ref: np.ndarray, bound: np.ndarray) -> float:
    """max |got - ref| / bound over the auditable entries: a finite bound and a float64 value inside float32's range (an
    expf that overflows in float32 is compared with the oracle bit for bit instead).  A zero bound demands equality."""
    got = got.astype(f64)
    ok = np.isfinite(bound) & (np.abs(ref) < 1e37)
    err = np.abs(got - ref)[ok]
    b = bound[ok]
    if err.size == 0:
        return 0.0
    if np.isnan(err).any():
        return float("inf")
    r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def auditable(ref: np.ndarray, bound: np.ndarray) -> np.ndarray:
    return np.isfinite(bound) & (np.abs(ref) < 1e37)


# ---------------------------------------------------------------------------------------------------------- threshold
def threshold_audit(cand: np.ndarray, s64: np.ndarray, sb: np.ndarray, vis, score32: np.ndarray,
                    oracle32: np.ndarray) -> dict:
    """Strict ``score > vis`` of one image's P priors.  ``cand``: bool (P,) the kernel's candidate set; ``score32``: the
    kernel's float32 scores; ``oracle32``: the oracle's.  A prior more than its bound above vis must be a candidate, one
    at least its bound below must not be; inside the band the kernel's decision must be its own float32 ``score > vis``,
    and the oracle's wherever the two float32 scores agree."""
    thr = f64(f32(vis))
    must, must_not = s64 - sb > thr, s64 + sb <= thr
    band = ~must & ~must_not
    same = score32 == oracle32
    bad = (must & ~cand) | (must_not & cand) | (band & (cand != (score32 > f32(vis)))) \
        | (band & same & (cand != (oracle32 > f32(vis))))
    return dict(bad=np.flatnonzero(bad), band=int(band.sum()), band_differs=int((band & ~same).sum()),
                must=int(must.sum()), must_not=int(must_not.sum()))


# ---------------------------------------------------------------------------------------------------------------- NMS
def _rnd(v, e_in):
    """Error of one float32 rounding of v (exact result of the op on the float32 inputs) given the inputs' error e_in:
    none when the inputs are exact and v is a float32."""
    exact = (e_in == 0) & (v.astype(f32).astype(f64) == v)
    return np.where(exact, 0.0, U * np.abs(v))


def _side(a, b, one):
    """RN(RN(a - b) + one) and its error (a, b exact float32 values in float64)."""
    d = a - b
    e = _rnd(d, np.zeros_like(d))
    v = d + one
    return v, e + _rnd(v, e)


def iou_delta(kb: np.ndarray, b: np.ndarray, one: float = 1.0):
    """float64 IoU of boxes kb (..., 4) against b (..., 4) (broadcast; float32 values) with the +``one`` convention of
    ``suppressed`` / ``nms_single``, and delta: |q - iou| of the unrounded float32 quotient q = a / (ka + area - a).
      w  = max(0, RN(RN(xx2 - xx1) + 1))  (max / min / the clamp are exact)       err e_w (from _side)
      a  = RN(w h)                                                               err w e_h + h e_w + e_w e_h + RN
      ka, area likewise;  dn = RN(RN(ka + area) - a)                            err e_ka + e_ar + 2 e_a + 2 RN
      delta = (e_a + q e_dn) / (dn - e_dn)
    Pairs with a non-finite or huge coordinate (float32 overflow would make the two evaluations differ) get delta = inf."""
    kb, b = kb.astype(f64), b.astype(f64)
    xx1, yy1 = np.maximum(kb[..., 0], b[..., 0]), np.maximum(kb[..., 1], b[..., 1])
    xx2, yy2 = np.minimum(kb[..., 2], b[..., 2]), np.minimum(kb[..., 3], b[..., 3])

    def area(x1, y1, x2, y2, clamp):
        wv, ew = _side(x2, x1, one)
        hv, eh = _side(y2, y1, one)
        if clamp:
            wv, hv = np.maximum(0.0, wv), np.maximum(0.0, hv)
        a = wv * hv
        ea = np.abs(wv) * eh + np.abs(hv) * ew + ew * eh
        return a, ea + _rnd(a, ea)

    a, ea = area(xx1, yy1, xx2, yy2, True)
    ka, eka = area(kb[..., 0], kb[..., 1], kb[..., 2], kb[..., 3], False)
    ar, ear = area(b[..., 0], b[..., 1], b[..., 2], b[..., 3], False)
    s = ka + ar
    es = eka + ear + _rnd(s, eka + ear)
    dn = s - a
    edn = es + ea + _rnd(dn, es + ea)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iou = a / dn
        delta = (ea + np.abs(iou) * edn) / (dn - edn) + 4e-16 * np.abs(iou)
    huge = ~(np.isfinite(kb).all(-1) & np.isfinite(b).all(-1) & (np.abs(kb).max(-1) < 1e15) & (np.abs(b).max(-1) < 1e15))
    delta = np.where(huge | ~(dn - edn > 0), np.inf, delta)
    return iou, delta


def survive_split(thr: float):
    """(T, tie_survives): float32 ``RN(q) <= thr`` is ``q < T``, or ``q <= T`` when a midpoint rounds down to thr."""
    t = f32(thr)
    up = np.nextafter(t, f32(np.inf))
    T = (f64(t) + f64(up)) / 2
    return T, (t.view(np.uint32) & 1) == 0


def pair_decided(kb, b, thr, one=1.0):
    """(surely_survives, surely_suppressed) of b against kept box kb, from the float64 IoU and its delta."""
    iou, d = iou_delta(kb, b, one)
    T, tie = survive_split(thr)
    lo, hi = iou + d, iou - d
    surv = (lo < T) | (tie & (lo == T))
    supp = (hi > T) | (~tie & (hi == T))
    return surv & np.isfinite(d), supp & np.isfinite(d)


def _touching(kb, b):
    """False only where the pair surely survives without evaluating the IoU: finite boxes of positive +1 extent whose
    +1-extended ranges are disjoint on an axis (the clamped intersection is 0, the union positive, so ovr = 0)."""
    def pos(x):
        return np.isfinite(x).all(-1) & (x[..., 2] - x[..., 0] > -1) & (x[..., 3] - x[..., 1] > -1)
    apart = (kb[..., 0] > b[..., 2] + 1) | (b[..., 0] > kb[..., 2] + 1) | (kb[..., 1] > b[..., 3] + 1) \
        | (b[..., 1] > kb[..., 3] + 1)
    return ~(apart & pos(kb) & pos(b))


def sort_order(scores: np.ndarray, desc_pos: bool = False) -> np.ndarray:
    """Score descending, then position ascending (``desc_pos``: the planted mistake of descending position)."""
    pos = np.arange(len(scores))
    return np.lexsort((-pos if desc_pos else pos, -scores.astype(f64)))


def nms_audit(boxes: np.ndarray, scores: np.ndarray, keep, thr: float = 0.4, one: float = 1.0) -> list[str]:
    """Independent float64 check of a greedy NMS keep list over K candidates; returns the violations found (empty: ok).
      * keep is ordered by score descending, then position ascending;
      * no kept box is surely suppressed by a box kept before it;
      * every other candidate could have been suppressed by some box kept before it in the sort order."""
    K = len(scores)
    keep = np.asarray(keep, dtype=np.int64)
    errs = []
    if K == 0:
        return [] if keep.size == 0 else ["keep list of an empty image"]
    if len(np.unique(keep)) != len(keep) or (keep.size and (keep.min() < 0 or keep.max() >= K)):
        return ["keep list holds duplicates or positions out of range"]
    rank = np.empty(K, np.int64)
    rank[sort_order(scores)] = np.arange(K)
    if np.any(np.diff(rank[keep]) <= 0):
        errs.append("keep list is not in (score desc, position asc) order")
    kb = boxes[keep]
    for r0 in range(1, len(keep), 256):
        rows = np.arange(r0, min(r0 + 256, len(keep)))
        ii, jj = np.nonzero(_touching(kb[None, :rows[-1]], kb[rows, None]) & (np.arange(rows[-1])[None, :] < rows[:, None]))
        _, supp = pair_decided(kb[jj], kb[rows[ii]], thr, one)
        if supp.any():
            i, j = rows[ii[supp][0]], jj[supp][0]
            errs.append(f"kept #{i} (pos {keep[i]}) is surely suppressed by kept #{j} (pos {keep[j]})")
            break
    pend = np.setdiff1d(np.arange(K), keep)
    pend = pend[np.argsort(rank[pend], kind="stable")]
    for k0 in range(0, len(keep), 32):
        if pend.size == 0:
            break
        kk = keep[k0:k0 + 32]
        explained = np.zeros(pend.size, bool)
        for c0 in range(0, pend.size, 1 << 17):
            c = pend[c0:c0 + (1 << 17)]
            ii, jj = np.nonzero(_touching(boxes[kk][:, None], boxes[c][None]) & (rank[kk][:, None] < rank[c][None]))
            surv, _ = pair_decided(boxes[kk[ii]], boxes[c[jj]], thr, one)
            explained[c0 + jj[~surv]] = True
        pend = pend[~explained]
    if pend.size:
        errs.append(f"{pend.size} suppressed candidates (first pos {pend[0]}) survive every box kept before them")
    return errs


def nms_f32(boxes: np.ndarray, scores: np.ndarray, thr: float = 0.4, one: float = 1.0, le: bool = True,
            desc_pos: bool = False) -> list[int]:
    """``oracle.retinaface_ref.nms_single`` with knobs for planted mistakes (+``one`` area, ``<=`` survival, tie order)."""
    boxes = boxes.astype(f32)
    o = f32(one)
    area = (boxes[:, 2] - boxes[:, 0] + o) * (boxes[:, 3] - boxes[:, 1] + o)
    order = sort_order(scores, desc_pos)
    t = f32(thr)
    keep = []
    while order.size:
        j = order[0]
        keep.append(int(j))
        rest = order[1:]
        xy1 = np.maximum(boxes[j, :2], boxes[rest, :2])
        xy2 = np.minimum(boxes[j, 2:], boxes[rest, 2:])
        wv = np.maximum(f32(0), xy2[:, 0] - xy1[:, 0] + o)
        hv = np.maximum(f32(0), xy2[:, 1] - xy1[:, 1] + o)
        a = wv * hv
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            ovr = a / (area[j] + area[rest] - a)
        order = rest[ovr <= t] if le else rest[ovr < t]
    return keep


def largest_ref(kept_boxes: np.ndarray, one: float = 1.0) -> int:
    """Rank in the keep list that "largest" selects: torch.argmax (first maximum, NaN maximal) of the float32 areas."""
    b = kept_boxes.astype(f32)
    o = f32(one)
    with np.errstate(over="ignore", invalid="ignore"):
        areas = (b[:, 2] - b[:, 0] + o) * (b[:, 3] - b[:, 1] + o)
    return int(torch.argmax(torch.from_numpy(np.ascontiguousarray(areas))))


# --------------------------------------------------------------------------------------------------------- generators
def head_inputs(n: int, h: int, w: int, seed: int, edges: bool = True):
    """Random (logits (n,P,2), loc (n,P,4), ldm (n,P,10)) float32; ``edges`` plants rows the kernel can get wrong:
    equal logits (score exactly 1/2), logits of +-80 and beyond (softmax saturation), l0 - l1 = ln(2^-23) (score
    exactly 1 - 2^-23 after the roundings), and loc whose expf overflows (inf / nan boxes)."""
    rng = np.random.default_rng(seed)
    P = prior_count(h, w)
    logits = rng.normal(0, 2.5, (n, P, 2)).astype(f32)
    loc = rng.normal(0, 1.0, (n, P, 4)).astype(f32)
    ldm = rng.normal(0, 1.5, (n, P, 10)).astype(f32)
    if edges and P >= 16:
        for i in range(n):
            r = rng.choice(P, 16, replace=False)
            logits[i, r[0]] = (1.5, 1.5)
            logits[i, r[1]] = (-3.25, -3.25)
            logits[i, r[2]] = (-80.0, 80.0)
            logits[i, r[3]] = (80.0, -80.0)
            logits[i, r[4]] = (-1e4, 200.0)
            logits[i, r[5]] = (150.0, -90.0)
            logits[i, r[6]] = (f32(-23 * np.log(2)), 0.0)
            logits[i, r[7]] = (f32(-30.0), 0.0)
            loc[i, r[8], 2] = 500.0                          # expf(100): inf width
            loc[i, r[9], 3] = 460.0                          # expf(92): inf height
            loc[i, r[10], 2:] = -600.0                       # expf underflows: zero-size box
            loc[i, r[11], :2] = 3e4                          # far outside the frame
    return logits, loc, ldm


def cluster_boxes(K: int, clusters: int, seed: int, spread: float = 4000.0):
    """K candidates in ``clusters`` tight groups (each suppressed by its best box: a few hundred keeps for any K),
    scores with many exact ties.  -> boxes (K, 4), scores (K,) float32."""
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(0, spread, (clusters, 2))
    sz = rng.uniform(20, 60, (clusters, 1))
    g = rng.integers(0, clusters, K)
    c = ctr[g] + rng.normal(0, 0.6, (K, 2))
    s = sz[g] * rng.uniform(0.97, 1.03, (K, 1))
    boxes = np.concatenate([c - s / 2, c + s / 2], -1).astype(f32)
    scores = (0.6 + np.round(rng.uniform(0, 0.4, K) * 4096) / 4096 * 0.999).astype(f32)
    return boxes, scores


def grid_boxes(rows: int, cols: int, seed: int):
    """A grid of well separated boxes: every one of rows * cols candidates survives NMS."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols].reshape(2, -1).astype(f64) * 40.0
    s = rng.uniform(10, 30, (x.size, 2))
    boxes = np.stack([x, y, x + s[:, 0], y + s[:, 1]], -1).astype(f32)
    scores = rng.uniform(0.61, 1.0, x.size).astype(f32)
    return boxes, scores


def iou_edge_boxes():
    """Integer boxes (+1 convention) whose IoU decisions are exact: box 0 = [0,0,9,9] (area 100); box 1 = [0,0,9,3]
    inside it (area 40: IoU exactly 0.4, survives ``<=``); box 2 = [0,0,9,4] (IoU 0.5, suppressed); box 3 = [20,0,29,9]
    vs box 4 = [24,0,33,9] (60 / 140 = 3/7); boxes 5 = [40,0,49,9] and 6 = [42,0,51,9] tie on score (80 / 120);
    box 7 = [60,0,69,9] vs box 8 = [60,0,75,9] tie on score (100 / 160)."""
    boxes = np.array([[0, 0, 9, 9], [0, 0, 9, 3], [0, 0, 9, 4], [20, 0, 29, 9], [24, 0, 33, 9], [40, 0, 49, 9],
                      [42, 0, 51, 9], [60, 0, 69, 9], [60, 0, 75, 9]], f32)
    scores = np.array([0.99, 0.98, 0.97, 0.9, 0.8, 0.9, 0.9, 0.7, 0.7], f32)
    return boxes, scores
