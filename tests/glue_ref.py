"""References of the BiSeNet / RRDB / input glue kernels (test helper, not a test module).

Two independent statements of every kernel of ``fcp_parse_enhance.hip`` and of the input converters and the range guard of
``fcp_elementwise.hip``:

* ``*_ref64``: the operation ``include/fcp_hip.h`` documents, accumulated in float64.  Index and weight math follows ATen
  (``area_pixel_compute_scale`` / ``area_pixel_compute_source_index`` / ``nearest_idx`` of ATen/native/UpSample.h): scales,
  source indices and interpolation weights are float32, exactly as ``F.interpolate`` computes them for a float32 tensor.
  tests/test_glue_ref_cpu.py checks these against ``torch.nn.functional`` in float64.
* ``*_f32``: the kernel's documented float32 operation order, op by op (the library is built with -ffp-contract=off and
  without fast-math, and numpy rounds every float32 ufunc once), so the device must match it bit for bit.  The only
  exception is ``expf`` in the sigmoid, which is not correctly rounded on either side (``EXP_ULP``).

``*_bound`` functions give the largest |f32 - ref64| the float32 order can produce, derived from its arithmetic (the
derivation is next to each).  ``U`` is the float32 unit roundoff; the factor ``SLACK`` covers the second-order terms
(products of two roundoffs) the first-order bounds leave out.

The input generators at the end are shared by the CPU and GPU tests, so the planted-mistake checks run on the very inputs
the device sees.  Plain numpy / torch on the host; nothing here calls the library.
"""
from __future__ import annotations

import numpy as np
import torch

f32 = np.float32
U = 2.0 ** -24           # float32 unit roundoff
SLACK = 1.01             # second-order terms of the first-order error bounds below
EXP_ULP = 4              # ulp allowed for expf (device) and np.exp (host, float32) in the sigmoid
BISE_MEAN = (0.485, 0.456, 0.406)        # oracle.bisenet_ref.MEAN / STD (bise.py hands them to the kernel as float32)
BISE_STD = (0.229, 0.224, 0.225)
CUBIC_W = (-3 / 32, 19 / 32, 19 / 32, -3 / 32)   # cubic convolution (A = -0.75) at t = 0.5: exact binary fractions


# ------------------------------------------------------------------------------------------------ ATen index math (float32)
def linear_src(in_size: int, out_size: int, align_corners: bool):
    """Source indices and weights of a linear resize along one axis, as ATen computes them for float32:
    (i0, i1, l0, l1), int64 / float32 arrays of length out_size."""
    dst = np.arange(out_size)
    if align_corners:
        scale = f32(in_size - 1) / f32(out_size - 1) if out_size > 1 else f32(0)
        src = scale * dst.astype(f32)
    else:
        scale = f32(in_size) / f32(out_size)
        src = scale * (dst.astype(f32) + f32(0.5)) - f32(0.5)
        src = np.where(src < f32(0), f32(0), src).astype(f32)
    i0 = src.astype(np.int64)                      # src >= 0: truncation is floor
    i1 = i0 + (i0 < in_size - 1)
    l1 = (src - i0.astype(f32)).astype(f32)
    l0 = (f32(1) - l1).astype(f32)
    return i0, i1, l0, l1


def nearest_idx(in_size: int, out_size: int) -> np.ndarray:
    """ATen ``nearest_idx`` (mode="nearest"), including its out == in and out == 2 * in branches."""
    dst = np.arange(out_size)
    if out_size == in_size:
        return dst
    if out_size == 2 * in_size:
        return dst >> 1
    scale = f32(in_size) / f32(out_size)
    return np.minimum(np.floor(dst.astype(f32) * scale).astype(np.int64), in_size - 1)


def nearest_idx_kernel(in_size: int, out_size: int) -> np.ndarray:
    """The parse-tail kernel's nearest index: min(floorf(dst * (in / out)), in - 1) with no special cases (the two ATen
    branches give the same integers: dst * 1 and dst * 0.5 are exact)."""
    scale = f32(in_size) / f32(out_size)
    return np.minimum(np.floor(np.arange(out_size).astype(f32) * scale).astype(np.int64), in_size - 1)


# ---------------------------------------------------------------------------------------------------- bise_preprocess
def preprocess_ref64(faces: np.ndarray, oh: int, ow: int, mean=BISE_MEAN, std=BISE_STD, align_corners=False):
    """(f, h, w, 3) uint8 -> (f, oh, ow, 3) float64: /255, bilinear (align_corners=False), (x - mean) / std."""
    _, h, w, _ = faces.shape
    y0, y1, hy0, hy1 = linear_src(h, oh, align_corners)
    x0, x1, wx0, wx1 = linear_src(w, ow, align_corners)
    v = faces.astype(np.float64) / 255.0
    hy0, hy1 = hy0.astype(np.float64)[:, None, None], hy1.astype(np.float64)[:, None, None]
    wx0, wx1 = wx0.astype(np.float64)[:, None], wx1.astype(np.float64)[:, None]
    r0, r1 = v[:, y0], v[:, y1]
    val = hy0 * (wx0 * r0[:, :, x0] + wx1 * r0[:, :, x1]) + hy1 * (wx0 * r1[:, :, x0] + wx1 * r1[:, :, x1])
    m = np.asarray(mean, np.float32).astype(np.float64)
    s = np.asarray(std, np.float32).astype(np.float64)
    return (val - m) / s


def preprocess_f32(faces: np.ndarray, oh: int, ow: int, mean=BISE_MEAN, std=BISE_STD, align_corners=False):
    """bise_preprocess_kernel's order: v = (float)u8 / 255.0f; hy0 * (wx0 * v00 + wx1 * v01) + hy1 * (wx0 * v10 + wx1 * v11);
    (v - mean) / std."""
    _, h, w, _ = faces.shape
    y0, y1, hy0, hy1 = linear_src(h, oh, align_corners)
    x0, x1, wx0, wx1 = linear_src(w, ow, align_corners)
    v = faces.astype(f32) / f32(255)
    hy0, hy1, wx0, wx1 = hy0[:, None, None], hy1[:, None, None], wx0[:, None], wx1[:, None]
    r0, r1 = v[:, y0], v[:, y1]
    val = hy0 * (wx0 * r0[:, :, x0] + wx1 * r0[:, :, x1]) + hy1 * (wx0 * r1[:, :, x0] + wx1 * r1[:, :, x1])
    return ((val - np.asarray(mean, f32)) / np.asarray(std, f32)).astype(f32)


def preprocess_bound(out64: np.ndarray, std=BISE_STD) -> np.ndarray:
    """|f32 - ref64|.  Both sides use the same float32 weights.  Every intermediate up to the mean subtraction has magnitude
    <= 1 (pixels / 255 in [0, 1], non-negative weights summing to 1 within u), and the longest chain rounds six times (/255,
    product, sum, product, sum, - mean): <= 6u absolute.  Division by std scales that by 1/std and rounds once more
    (u |out|)."""
    s = np.asarray(std, np.float32).astype(np.float64)
    return SLACK * (6 * U / s + U * np.abs(out64))


# ------------------------------------------------------------------------------------------------------------- avgpool
def avgpool_ref64(x: np.ndarray, c: int) -> np.ndarray:
    """x (n, hw, ld) float32, channels [0, c) -> (n, c) float64 mean over hw."""
    return x[:, :, :c].astype(np.float64).mean(1)


def avgpool_f32(x: np.ndarray, c: int, drop_last=False) -> np.ndarray:
    """avgpool_kernel's order: wave `part` sums pixels part, part + 4, ... ascending; ((r0 + r1) + r2) + r3; / hw."""
    n, hw, _ = x.shape
    xs = x[:, :, :c]
    last = hw - 1 if drop_last else hw
    parts = []
    for part in range(4):
        acc = np.zeros((n, c), f32)
        for p in range(part, last, 4):
            acc = acc + xs[:, p]
        parts.append(acc)
    return (((parts[0] + parts[1]) + parts[2]) + parts[3]) / f32(hw)


def avgpool_bound(x: np.ndarray, c: int, out64: np.ndarray) -> np.ndarray:
    """A wave's chain of m = ceil(hw / 4) additions (the first onto 0 is exact) and the three additions of the partial sums:
    <= (m + 2) u sum |x|; the division rounds once (u |mean|)."""
    hw = x.shape[1]
    m = -(-hw // 4)
    sabs = np.abs(x[:, :, :c].astype(np.float64)).sum(1)
    return SLACK * U * ((m + 2) * sabs / hw + np.abs(out64))


# ------------------------------------------------------------------------------------------------------------------ fc
def _act64(v, act):
    if act == 1:
        return np.maximum(v, 0.0)
    if act == 2:
        return 1.0 / (1.0 + np.exp(-v))
    return v


def fc_ref64(x, w, scale, shift, act):
    """out[n][co] = act(scale[co] * dot(w[co, :], x[n, :]) + shift[co]) in float64; scale / shift may be None."""
    v = x.astype(np.float64) @ w.astype(np.float64).T
    if scale is not None:
        v = v * scale.astype(np.float64)
    if shift is not None:
        v = v + shift.astype(np.float64)
    return _act64(v, act)


def fc_f32(x, w, scale, shift, act, skip_last=False):
    """fc_kernel's order: lane k sums products k, k + 64, ... ascending; shfl_down tree 32, 16, ..., 1 (lane 0's value);
    * scale; + shift; act (sigmoid: 1 / (1 + exp(-v)))."""
    n, cin = x.shape
    cout = w.shape[0]
    last = cin - 1 if skip_last else cin
    acc = np.zeros((n, cout, 64), f32)
    for k0 in range(0, last, 64):
        k1 = min(k0 + 64, last)
        acc[:, :, :k1 - k0] = acc[:, :, :k1 - k0] + w[None, :, k0:k1] * x[:, None, k0:k1]
    off = 32
    while off > 0:
        acc[:, :, :off] = acc[:, :, :off] + acc[:, :, off:2 * off]
        off >>= 1
    v = acc[:, :, 0]
    if scale is not None:
        v = v * scale
    if shift is not None:
        v = v + shift
    if act == 1:
        v = np.where(v > 0, v, f32(0))
    elif act == 2:
        v = f32(1) / (f32(1) + np.exp(-v))
    return v.astype(f32)


def fc_bound(x, w, scale, shift, act, out64):
    """Lane chains of m = ceil(cin / 64) products and sums, then six tree levels: <= (m + 6) u sum |w x|.  * scale rounds once
    (u |scale dot|), + shift once (u |pre|).  ReLU is 1-Lipschitz.  The sigmoid is 1/4-Lipschitz; expf's EXP_ULP ulp
    (<= 2 EXP_ULP u relative) and the two float32 operations after it add (2 EXP_ULP + 2) u |out|."""
    cin = x.shape[1]
    m = -(-cin // 64)
    sabs = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    dot = x.astype(np.float64) @ w.astype(np.float64).T
    sc = np.abs(scale.astype(np.float64)) if scale is not None else 1.0
    e = (m + 6) * U * sabs * sc
    pre = dot * (scale.astype(np.float64) if scale is not None else 1.0)
    if scale is not None:
        e = e + U * np.abs(pre)
    if shift is not None:
        pre = pre + shift.astype(np.float64)
        e = e + U * np.abs(pre)
    if act == 2:
        e = 0.25 * e + (2 * EXP_ULP + 2) * U * np.abs(out64)
    return SLACK * e


# ----------------------------------------------------------------------------------------------------------- scale_add
def scale_add_ref64(x, s, addv, addt):
    """out = x * s[n, c] (+ addv[n, c]) (+ addt[n, h, w, c]); x / addt (n, hw, c), s / addv (n, c)."""
    v = x.astype(np.float64) * s.astype(np.float64)[:, None]
    if addv is not None:
        v = v + addv.astype(np.float64)[:, None]
    if addt is not None:
        v = v + addt.astype(np.float64)
    return v


def scale_add_f32(x, s, addv, addt):
    v = x * s[:, None]
    if addv is not None:
        v = v + addv[:, None]
    if addt is not None:
        v = v + addt
    return v.astype(f32)


def scale_add_bound(x, s, addv, addt):
    """At most three roundings, each of a partial result no larger than the sum of the absolute terms."""
    t = np.abs(x.astype(np.float64) * s.astype(np.float64)[:, None])
    if addv is not None:
        t = t + np.abs(addv.astype(np.float64))[:, None]
    if addt is not None:
        t = t + np.abs(addt.astype(np.float64))
    return SLACK * 3 * U * t


# ---------------------------------------------------------------------------------------------------------- parse tail
def parse_values(logits, ncls, mid_h, mid_w, oh, ow, dtype, align_corners=True, nearest=nearest_idx):
    """Class scores at every output pixel: bilinear (align_corners) of (f, lh, lw, ld) logits to (mid_h, mid_w), nearest to
    (oh, ow).  Evaluated only at the mid rows / columns the nearest map keeps.  dtype float32: the kernel's order
    hy0 * (wx0 * p00 + wx1 * p01) + hy1 * (wx0 * p10 + wx1 * p11); float64: the same weights, float64 arithmetic.
    Returns (f, oh, ow, ncls)."""
    _, lh, lw, _ = logits.shape
    my, mx = nearest(mid_h, oh), nearest(mid_w, ow)
    y0, y1, hy0, hy1 = (a[my] for a in linear_src(lh, mid_h, align_corners))
    x0, x1, wx0, wx1 = (a[mx] for a in linear_src(lw, mid_w, align_corners))
    lg = logits[..., :ncls].astype(dtype)
    hy0, hy1 = hy0.astype(dtype)[:, None, None], hy1.astype(dtype)[:, None, None]
    wx0, wx1 = wx0.astype(dtype)[:, None], wx1.astype(dtype)[:, None]
    r0, r1 = lg[:, y0], lg[:, y1]
    with np.errstate(invalid="ignore"):
        return hy0 * (wx0 * r0[:, :, x0] + wx1 * r0[:, :, x1]) + hy1 * (wx0 * r1[:, :, x0] + wx1 * r1[:, :, x1])


def first_argmax(v: np.ndarray) -> np.ndarray:
    """torch.argmax over the last axis: the first maximum; the first NaN if there is one."""
    return np.argmax(v, -1)


def parse_tail_f32(logits, ncls, mid_h, mid_w, oh, ow, align_corners=True):
    """parse_tail_kernel: labels (f, oh, ow) uint8 in the kernel's float32 order and nearest formula."""
    return first_argmax(parse_values(logits, ncls, mid_h, mid_w, oh, ow, np.float32, align_corners,
                                     nearest_idx_kernel)).astype(np.uint8)


def parse_value_bound(logits, ncls) -> float:
    """One interpolated score: both sides share the float32 weights (non-negative, summing to 1 within u); the float32 order
    rounds four times on its longest chain (product, sum, product, sum) a quantity <= max |logit|: <= 4u max |logit|."""
    a = np.abs(logits[..., :ncls].astype(np.float64))
    return SLACK * 4 * U * float(np.nanmax(np.where(np.isinf(a), 0, a)))


def parse_label_violations(labels, logits, ncls, mid_h, mid_w, oh, ow, worst=False):
    """Pixels whose label is wrong by the float64 reference: a NaN score must give the first NaN class; otherwise the label's
    float64 score must lie within 2 * parse_value_bound of the float64 maximum (each of the two float32 scores the kernel
    compared may be off by one bound).  Returns a boolean (f, oh, ow) map; worst=True: also the largest
    (max - score of the label) / (2 * parse_value_bound) over the pixels without NaN."""
    v = parse_values(logits, ncls, mid_h, mid_w, oh, ow, np.float64)
    tol = 2 * parse_value_bound(logits, ncls)
    lab = labels.astype(np.int64)
    nan = np.isnan(v)
    any_nan = nan.any(-1)
    first_nan = np.argmax(nan, -1)
    vmax = np.where(nan, -np.inf, v).max(-1)
    got = np.take_along_axis(np.where(nan, -np.inf, v), lab[..., None], -1)[..., 0]
    bad_nan = any_nan & (lab != first_nan)
    bad_val = ~any_nan & ~(got >= vmax - tol)
    if worst:
        gap = np.where(any_nan, 0.0, vmax - got)
        return bad_nan | bad_val, float(gap.max() / tol) if gap.size else 0.0
    return bad_nan | bad_val


# ------------------------------------------------------------------------------------------------- histogram and masks
def label_counts(labels: np.ndarray, ncls: int) -> np.ndarray:
    return np.stack([np.bincount(l.reshape(-1), minlength=ncls)[:ncls] for l in labels]).astype(np.int32)


def label_mask(labels: np.ndarray, class_bits: int) -> np.ndarray:
    bit = (np.uint64(class_bits) >> (labels.astype(np.uint64) & np.uint64(31))) & np.uint64(1)
    return np.where(bit == 1, 255, 0).astype(np.uint8)


# -------------------------------------------------------------------------------------------------------- bicubic x0.25
def _taps(x4, h, w, r, q, shift):
    """Channels 0..2 of tap (r, q) of every output pixel: x4[4y + r + shift, 4x + q + shift], clamped to the image."""
    ih, iw = x4.shape[0], x4.shape[1]
    ys = np.minimum(4 * np.arange(h) + r + shift, ih - 1)
    xs = np.minimum(4 * np.arange(w) + q + shift, iw - 1)
    if shift == 0:
        return x4[r::4, q::4, :3][:h, :w]
    return x4[ys][:, xs, :3]


def bicubic_ref64(x4: np.ndarray, h: int, w: int, shift: int = 0) -> np.ndarray:
    """(4h, 4w, ld) float32 -> (h, w, 3) float64 bicubic x0.25 before the clamp (align_corners=False, A=-0.75: source
    4x + 1.5, taps 4x .. 4x + 3 with weights CUBIC_W)."""
    acc = np.zeros((h, w, 3))
    for r in range(4):
        row = np.zeros((h, w, 3))
        for q in range(4):
            row += CUBIC_W[q] * _taps(x4, h, w, r, q, shift).astype(np.float64)
        acc += CUBIC_W[r] * row
    return acc


def to_u8(v):
    """clamp(0, 1) * 255, round half to even."""
    v = np.clip(v, 0, 1)
    return np.rint(v * (f32(255) if v.dtype == np.float32 else 255.0)).astype(np.uint8)


def bicubic_f32(x4: np.ndarray, h: int, w: int, shift: int = 0) -> np.ndarray:
    """bicubic_down4_kernel's order: row_r = ((p0 w0 + p1 w1) + p2 w2) + p3 w3; acc = ((row0 w0 + row1 w1) + ...);
    clamp; * 255.0f; rintf."""
    wt = [f32(c) for c in CUBIC_W]
    acc = None
    for r in range(4):
        row = None
        for q in range(4):
            t = _taps(x4, h, w, r, q, shift) * wt[q]
            row = t if row is None else row + t
        t = row * wt[r]
        acc = t if acc is None else acc + t
    return to_u8(acc.astype(f32))


def bicubic_window(x4: np.ndarray) -> float:
    """|255 * clamp(acc32) - 255 * clamp(ref64)| before rounding to a byte.  Products by the binary-fraction weights round
    once each; a row is four products and three sums: <= 4u sum_q |w_q p| <= 4u * 1.375 M (M = max |x4|).  The column
    rounds the same way over rows that are themselves off: 4u * 1.375 * (1.375 M) + 1.375 * (4u * 1.375 M).  The clamp does
    not widen it, * 255 multiplies by 255 and rounds once (<= 255u after the clamp)."""
    mx = float(np.abs(x4[..., :3]).max())
    e_acc = 8 * U * 1.375 * 1.375 * mx
    return SLACK * 255 * (e_acc + U)


def bicubic_violations(out: np.ndarray, ref64: np.ndarray, window: float) -> np.ndarray:
    """Bytes that differ from the float64 reference's byte where 255 * clamp(ref64) is not within `window` of a .5 boundary."""
    t = np.clip(ref64, 0, 1) * 255.0
    near_half = np.abs(t - np.floor(t) - 0.5) <= window
    return (out != np.rint(t).astype(np.uint8)) & ~near_half


# -------------------------------------------------------------------------------------------------------------- absmax
def absmax_ref(vals: np.ndarray) -> np.float32:
    """max |x| over the view (float32 values), NaN counted as +inf, starting from the caller's 0."""
    a = np.abs(vals.astype(np.float32))
    a = np.where(np.isnan(a), np.float32(np.inf), a)
    return np.float32(max(0.0, float(a.max()))) if a.size else np.float32(0)


def split32_decode(raw: np.ndarray) -> np.ndarray:
    """split32 storage (..., c) float32 -> float32 values: per 32 channels, 32 binary16 hi parts then 32 lo parts;
    hi + lo is exact in float32."""
    c = raw.shape[-1]
    h = np.ascontiguousarray(raw).view(np.float16).reshape(*raw.shape[:-1], c // 32, 2, 32).astype(np.float32)
    return (h[..., 0, :] + h[..., 1, :]).reshape(*raw.shape[:-1], c)


# ------------------------------------------------------------------------------------------------------ input converters
def u8_to_nhwc4_f32(img: np.ndarray, sub, div) -> np.ndarray:
    """(npix, 3) uint8 or float32 -> (npix, 4) float32: (x - sub) / div (no division when div == 1), channel 3 = 0."""
    v = img.astype(f32) - np.asarray(sub, f32)
    if f32(div) != f32(1):
        v = v / f32(div)
    return np.concatenate([v, np.zeros((v.shape[0], 1), f32)], 1)


# ------------------------------------------------------------------------------------------------------ shared inputs
def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def faces_u8(f, h, w, seed) -> np.ndarray:
    return torch.randint(0, 256, (f, h, w, 3), generator=gen(seed), dtype=torch.uint8).numpy()


PREPROCESS_SIZES = [(1, 1), (1, 37), (41, 1), (64, 64), (100, 72), (511, 511), (512, 512), (700, 900), (1024, 1024)]
PREPROCESS_RESIZED = [(64, 64), (100, 72), (511, 511), (700, 900), (1024, 1024)]   # sizes where align_corners matters


def avgpool_input(n, hw, ld, seed) -> np.ndarray:
    """(n, hw, ld) float32, magnitudes in [0.5, 1.5) with random signs (every pixel matters to the mean)."""
    g = gen(seed)
    mag = torch.rand(n, hw, ld, generator=g) + 0.5
    sgn = torch.randint(0, 2, (n, hw, ld), generator=g) * 2 - 1
    return (mag * sgn).numpy().astype(f32)


AVGPOOL_HW = [1, 3, 124, 125, 128, 129, 256, 1024, 4096]
AVGPOOL_C = [4, 19, 64, 65, 128, 512]
AVGPOOL_SHIPPED = [(256, 512), (256, 128), (1024, 128), (4096, 256)]


def fc_input(n, cin, cout, seed):
    """x (n, cin), w (cout, cin) / sqrt(cin), scale in [0.5, 1.5), shift ~ N(0, 1)/4: pre-activations O(1)."""
    g = gen(seed)
    x = torch.randn(n, cin, generator=g)
    w = torch.randn(cout, cin, generator=g) / cin ** 0.5
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g) / 4
    return tuple(t.numpy().astype(f32) for t in (x, w, sc, sh))


FC_CIN = [1, 63, 64, 65, 128, 256, 512]
FC_COUT = [1, 19, 64, 256]
FC_N = [1, 3, 32]


def logits_input(f, lh, lw, ld, seed, ties=None, nan_at=None) -> np.ndarray:
    """(f, lh, lw, ld) float32 logits ~ N(0, 1), padding channels (ncls..ld) = 1e30 (a kernel that read them would pick
    them).  ties=(a, b): class b becomes a copy of class a, raised by 3 so the pair wins most pixels; nan_at=(fi, y, x, c):
    NaN in classes c and c + 1 of that logit pixel."""
    x = torch.randn(f, lh, lw, ld, generator=gen(seed)).numpy().astype(f32)
    if ties is not None:
        a, b = ties
        x[..., a] += 3
        x[..., b] = x[..., a]
    if nan_at is not None:
        fi, y, xx, c = nan_at
        x[fi, y, xx, c] = np.nan
        x[fi, y, xx, c + 1] = np.nan
    return x


def pad_logits(x: np.ndarray, ncls: int) -> np.ndarray:
    out = x.copy()
    out[..., ncls:] = np.float32(1e30)
    return out


PARSE_OUT = [(1, 1), (37, 29), (64, 64), (255, 257), (256, 256), (512, 512), (1024, 1024)]


def bicubic_input(h, w, ld, seed) -> np.ndarray:
    """(4h, 4w, ld) float32 in [-0.2, 1.2); with more than one output pixel, the first one's 4 x 4 taps are 1.2 and the
    last one's -0.2, so both clamps fire."""
    x = (torch.rand(4 * h, 4 * w, ld, generator=gen(seed)) * 1.4 - 0.2).numpy().astype(f32)
    if h * w > 1:
        x[-4:, -4:] = f32(-0.2)
        x[:4, :4] = f32(1.2)
    return x


BICUBIC_HW = [(1, 1), (2, 2), (3, 3), (17, 17), (20, 24), (256, 256)]
BICUBIC_LD = [3, 4, 32]
