"""5-point align + crop on device (reference ``Cropper.crop_align``,
cropper.py:441-552, whose arithmetic is cv2.estimateAffine*2D + cv2.warpAffine)."""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _native as N
from . import torch_ops as T

BORDER_MODES = {"constant": 0, "replicate": 1, "reflect": 2, "wrap": 3, "reflect_101": 4,
                "reflect101": 4, "default": 4}

STANDARD_LANDMARKS_5 = np.float32([
    [0.31556875000000000, 0.4615741071428571],
    [0.68262291666666670, 0.4615741071428571],
    [0.50026249999999990, 0.6405053571428571],
    [0.34947187500000004, 0.8246919642857142],
    [0.65343645833333330, 0.8246919642857142],
])


def border_code(padding: str) -> int:
    """``getattr(cv2, f"BORDER_{padding.upper()}")`` (cropper.py:512)."""
    key = padding.lower()
    if key not in BORDER_MODES:
        raise AttributeError(f"module 'cv2' has no attribute 'BORDER_{padding.upper()}'")
    return BORDER_MODES[key]


def estimate_transform(landmarks: torch.Tensor, target: torch.Tensor, allow_skew: bool = False,
                       face_count: torch.Tensor | None = None, valid_total: torch.Tensor | None = None):
    """landmarks (F,k,2) f32 device, target (k,2) f32 device -> (mat (F,6) f64, ok (F,) i32).
    ``face_count``: device int32 scalar (view), live rows of a fixed-capacity face array — rows beyond it get ok = 0;
    ``valid_total``: device int64 scalar the number of ok faces is added to (both optional, no host read-back)."""
    f, k = landmarks.shape[0], landmarks.shape[1]
    dev = landmarks.device
    if T.ENABLED:
        mat, ok = T.load().similarity_from_5pt(landmarks.contiguous(), target.contiguous(), bool(allow_skew), face_count,
                                               valid_total)
        return mat.view(f, 6), ok
    mat = torch.empty((f, 6), dtype=torch.float64, device=dev)
    ok = torch.empty((f,), dtype=torch.int32, device=dev)
    N.check(N.lib().fcp_estimate_transform_counted(N.ptr(landmarks.contiguous()), N.ptr(target.contiguous()), f, k,
                                                   int(bool(allow_skew)), N.ptr(face_count), N.ptr(mat), N.ptr(ok),
                                                   N.ptr(valid_total), N.stream_ptr()),
            "fcp_estimate_transform")
    return mat, ok


# The two algorithm families of cv2.warpAffine(INTER_LINEAR) the device implements byte for byte: "fixed" (OpenCV's classic
# 5-bit-fraction / 15-bit-weight tables, the default) and "float32" (the float SIMD linear warp of newer OpenCV builds).
WARP_FAMILIES = ("fixed", "float32")
_WARP_ENTRY = {"fixed": "warp_affine_u8", "float32": "warp_affine_u8_float"}


def _check_family(family):
    if family not in WARP_FAMILIES:
        raise ValueError(f"unknown warpAffine family {family!r}: choose one of {WARP_FAMILIES}")


# The warpAffine filters: "linear" (INTER_LINEAR, in either family) and OpenCV's fixed-point INTER_CUBIC / INTER_LANCZOS4
# warps, which have one family only; the values are the cv2.INTER_* codes of the C ABI.
INTERPOLATIONS = ("linear", "cubic", "lanczos4")
_INTERP_CODE = {"cubic": 2, "lanczos4": 4}


def check_interpolation(interpolation, family="fixed"):
    """Raise ValueError for an unknown ``interpolation`` or for cubic / Lanczos-4 asked of the float32 family."""
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"unknown interpolation {interpolation!r}: choose one of {INTERPOLATIONS}")
    if interpolation != "linear" and family == "float32":
        raise ValueError(f"interpolation={interpolation!r} has no float32 family: OpenCV warps cubic and Lanczos-4 with "
                         f"fixed-point tables only (use warp_family 'fixed' or 'auto')")


def warp_affine(images_u8: torch.Tensor, img_idx: torch.Tensor, mat: torch.Tensor, ok: torch.Tensor | None,
                paddings: torch.Tensor | None, output_size, border: int = 0, family: str = "fixed",
                interpolation: str = "linear") -> torch.Tensor:
    """images (n,h,w,3) u8 device; output_size = (width, height) like cv2's dsize; ``family``: one of ``WARP_FAMILIES``;
    ``interpolation``: one of ``INTERPOLATIONS`` ("cubic" / "lanczos4" only with the "fixed" family)."""
    _check_family(family)
    check_interpolation(interpolation, family)
    assert images_u8.dtype == torch.uint8 and images_u8.is_contiguous() and images_u8.shape[3] == 3
    n, h, w, _ = images_u8.shape
    f = img_idx.shape[0]
    ow, oh = int(output_size[0]), int(output_size[1])
    if interpolation != "linear":
        code = _INTERP_CODE[interpolation]
        if T.ENABLED:
            return T.load().warp_affine_u8_interp(images_u8, img_idx, mat.contiguous().view(f, 2, 3), ok, paddings, ow, oh,
                                                  int(border), code)
        out = torch.empty((f, oh, ow, 3), dtype=torch.uint8, device=images_u8.device)
        N.check(N.lib().fcp_warp_affine_u8_interp(N.ptr(images_u8), n, h, w, N.ptr(img_idx), N.ptr(mat), N.ptr(ok),
                                                  N.ptr(paddings), f, oh, ow, int(border), code, N.ptr(out), N.stream_ptr()),
                "fcp_warp_affine_u8_interp")
        return out
    entry = _WARP_ENTRY[family]
    if T.ENABLED:
        return getattr(T.load(), entry)(images_u8, img_idx, mat.contiguous().view(f, 2, 3), ok, paddings, ow, oh, int(border))
    out = torch.empty((f, oh, ow, 3), dtype=torch.uint8, device=images_u8.device)
    N.check(getattr(N.lib(), "fcp_" + entry)(N.ptr(images_u8), n, h, w, N.ptr(img_idx), N.ptr(mat), N.ptr(ok),
                                             N.ptr(paddings), f, oh, ow, int(border), N.ptr(out), N.stream_ptr()),
            "fcp_" + entry)
    return out


_AUTO_FAMILY = {}     # (cv2.__version__, border code) -> family chosen by the probe, for the life of the process


def resolve_warp_family(value, border, device=None) -> str:
    """The warpAffine family a ``Cropper`` uses: ``"fixed"`` or ``"float32"``.  ``value``: ``None`` (``$FCP_WARP_FAMILY``,
    else ``"fixed"``), ``"fixed"``, ``"float32"`` or ``"auto"``: the family whose device output equals the installed
    ``cv2.warpAffine``'s byte for byte on a small probe with this ``border`` (a cv2 border code or a padding name);
    ``"fixed"`` when cv2 cannot be imported, and ``"fixed"`` with a warning when neither family matches."""
    if value is None:
        value = os.environ.get("FCP_WARP_FAMILY") or "fixed"
    if value == "auto":
        return _auto_family(border, device)
    if value not in WARP_FAMILIES:
        raise ValueError(f"unknown warp_family {value!r}: choose one of {WARP_FAMILIES + ('auto',)} (or None)")
    return value


def _probe_case():
    """A 64 x 80 RGB image of integer patterns (edges and texture of every contrast) and four forward transforms: rotation
    with a non-integer scale and sub-pixel shift, a downscale, an upscale, and one that reaches outside the image."""
    y, x, c = np.meshgrid(np.arange(64), np.arange(80), np.arange(3), indexing="ij")
    img = ((x * 37 + y * 91 + c * 53 + (x * y) % 29 * 7 + ((x // 5 + y // 7) % 2) * 128) % 256).astype(np.uint8)

    def fwd(scale, theta, tx, ty):
        a, b = scale * np.cos(theta), scale * np.sin(theta)
        return np.array([[a, -b, tx], [b, a, ty]], np.float64)

    mats = [fwd(0.83, 0.37, 7.3, -4.6), fwd(0.45, -0.12, 3.25, 6.7), fwd(2.3, 0.21, -30.7, -41.3), fwd(1.1, -0.9, -40.4, 51.9)]
    return img, mats, (56, 48)


def _auto_family(border, device) -> str:
    try:
        import cv2
    except ImportError:
        return "fixed"
    border = border_code(border) if isinstance(border, str) else int(border)
    key = (str(cv2.__version__), border)
    if key in _AUTO_FAMILY:
        return _AUTO_FAMILY[key]
    img, mats, dsize = _probe_case()
    want = np.stack([cv2.warpAffine(img, m, dsize, borderMode=border) for m in mats]).astype(np.int64)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        images = torch.from_numpy(img)[None].to(dev)
        idx = torch.zeros(len(mats), dtype=torch.int32, device=dev)
        mat = torch.from_numpy(np.stack(mats).reshape(-1, 6)).to(dev)
        diff = {fam: int(np.abs(warp_affine(images, idx, mat, None, None, dsize, border, fam).cpu().numpy() - want).max())
                for fam in WARP_FAMILIES}
    family = next((fam for fam in WARP_FAMILIES if diff[fam] == 0), None)
    if family is None:
        import warnings
        warnings.warn(f"warp_family='auto': cv2 {cv2.__version__} warpAffine (border {border}) matches neither device family "
                      f"(max |diff|: " + ", ".join(f"{k} {v}" for k, v in diff.items()) + "); using 'fixed'")
        family = "fixed"
    _AUTO_FAMILY[key] = family
    return family


def crop_align(images_u8, img_idx, landmarks, target, output_size, border=0, allow_skew=False, paddings=None,
               face_count=None, valid_total=None, family="fixed", interpolation="linear"):
    """Device crop_align: -> (crops (F,oh,ow,3) u8, ok (F,) i32, mat (F,6) f64).  Faces
    with ok == 0 (degenerate transform) are dropped by the caller like cropper.py:529-531.
    ``face_count`` / ``valid_total``: see ``estimate_transform``; ``family``, ``interpolation``: see ``warp_affine``."""
    _check_family(family)
    check_interpolation(interpolation, family)
    dev = images_u8.device
    landmarks = landmarks.to(device=dev, dtype=torch.float32)
    if not isinstance(target, torch.Tensor):
        target = torch.from_numpy(np.ascontiguousarray(target, dtype=np.float32))
    target = target.to(dev)
    img_idx = img_idx.to(device=dev, dtype=torch.int32).contiguous()
    if paddings is not None:
        paddings = paddings.to(device=dev, dtype=torch.int32).contiguous()
    mat, ok = estimate_transform(landmarks, target, allow_skew, face_count, valid_total)
    crops = warp_affine(images_u8, img_idx, mat, ok, paddings, output_size, border, family, interpolation)
    return crops, ok, mat


# ------------------------------------------------------------------ sharpness (Cropper(min_sharpness=...))
# Variance of the Laplacian of the crops' gray image, cv2.Laplacian(cv2.cvtColor(crop, cv2.COLOR_RGB2GRAY), cv2.CV_64F).var(),
# from exact integer sums: the device adds, the host divides once.

def sharpness_sums(crops_dev: torch.Tensor, ok: torch.Tensor | None = None) -> torch.Tensor:
    """crops (F,H,W,3) u8 device -> (F,2) int64 device: S1 = sum L and S2 = sum L*L of every crop's Laplacian L (gray
    ``(9798 R + 19235 G + 3735 B + 16384) >> 15``, 4-neighbour kernel, BORDER_REFLECT_101).  Crops with ``ok == 0`` are
    skipped, their sums are 0.  One launch; W <= 8192."""
    assert crops_dev.dtype == torch.uint8 and crops_dev.is_contiguous() and crops_dev.dim() == 4 and crops_dev.shape[3] == 3
    if T.ENABLED:
        return T.load().crop_sharpness(crops_dev, ok)
    f, h, w, _ = crops_dev.shape
    sums = torch.empty((f, 2), dtype=torch.int64, device=crops_dev.device)
    N.check(N.lib().fcp_crop_sharpness_u8(N.ptr(crops_dev), f, h, w, N.ptr(ok), N.ptr(sums), N.stream_ptr()),
            "fcp_crop_sharpness_u8")
    return sums


def sharpness_score(sums, n_pixels: int) -> np.ndarray:
    """(F,2) sums of ``sharpness_sums`` (a host array, or a device tensor, read back once) and N = H*W -> (F,) float64
    population variance ``(N*S2 - S1*S1) / (N*N)``: the numerator in Python integers (it passes 2^63 beyond 1024^2
    crops), then one correctly rounded division, so the score does not depend on any summation order."""
    if isinstance(sums, torch.Tensor):
        sums = sums.cpu().numpy()
    n = int(n_pixels)
    return np.array([(n * int(s2) - int(s1) * int(s1)) / (n * n) for s1, s2 in np.asarray(sums).reshape(-1, 2)], np.float64)


# ------------------------------------------------------------------ crop_source="original"
# Crops sampled from the decoded files instead of the resized batch.  A face whose crop would minify the file by 2 or more
# is sampled from a power-of-two INTER_AREA level of it instead (cv2.resize(O, (w >> L, h >> L), INTER_AREA)), so that the
# final bilinear warp never minifies below 0.5.  Every step is a composition of OpenCV calls.

_WARP_FAMILY_CODE = {"fixed": 0, "float32": 1}
WARP_SRC_DTYPE = np.dtype([("off", "<i8"), ("h", "<i4"), ("w", "<i4")])                           # fcp_warp_src
AREA_LEVEL_DTYPE = np.dtype([("src_off", "<i8"), ("sh", "<i4"), ("sw", "<i4"), ("dst_off", "<i8"), ("dh", "<i4"),
                             ("dw", "<i4")])                                                     # fcp_area_level
MAX_SOURCE_SIDE = 32767      # the fixed-point warp saturates source coordinates to short, as cv2.warpAffine does


def source_landmarks(landmarks, w, h, ww, hh, left, top):
    """Batch landmarks (F,k,2) float32 (the detector's, before un-padding) -> the same points in the decoded (h,w) image:
    ``(x - left + 0.5) * (w / ww) - 0.5`` (and likewise y), float64 in that order, then float32 — the pixel-centre
    convention of cv2.resize.  ``w, h, ww, hh, left, top``: scalars or per-face (F,) arrays of the image size, the resized
    size in the batch and the batch padding in front of it (``batch.batch_geometry``)."""
    lm = np.asarray(landmarks, np.float32).astype(np.float64)
    col = lambda v: np.asarray(v, np.float64).reshape(-1, 1) if np.ndim(v) else np.float64(v)
    rx = col(np.asarray(w, np.float64) / np.asarray(ww, np.float64))
    ry = col(np.asarray(h, np.float64) / np.asarray(hh, np.float64))
    out = np.empty(lm.shape, np.float32)
    out[..., 0] = ((lm[..., 0] - col(left) + 0.5) * rx - 0.5).astype(np.float32)
    out[..., 1] = ((lm[..., 1] - col(top) + 0.5) * ry - 0.5).astype(np.float32)
    return out


def pyramid_level(mat, w: int, h: int) -> int:
    """The level L a face is cropped from: the largest L with ``s * 2**L <= 1``, s = sqrt(|det M[:, :2]|) the crop pixels
    per source pixel (L = 0 when s > 0.5), capped so that the level keeps at least one pixel a side."""
    m = np.asarray(mat, np.float64).reshape(6)
    s = float(np.sqrt(abs(m[0] * m[4] - m[1] * m[3])))
    if not (s > 0.0 and np.isfinite(s)):
        return 0
    lv = 0
    while s * float(1 << (lv + 1)) <= 1.0 and (w >> (lv + 1)) >= 1 and (h >> (lv + 1)) >= 1:
        lv += 1
    return lv


def compose_level(mat, w: int, h: int, level: int) -> np.ndarray:
    """The forward transform M (2x3) re-expressed on level ``level`` of a (h,w) image, pixel-centre aligned:
    M_L = M . [(x_L + 0.5) / sx - 0.5] with sx = (w >> L) / w, sy = (h >> L) / h.  M itself at level 0."""
    m = np.asarray(mat, np.float64).reshape(2, 3)
    if level == 0:
        return m.copy()
    sx, sy = (w >> level) / w, (h >> level) / h
    out = np.empty((2, 3), np.float64)
    for r in range(2):
        out[r, 0] = m[r, 0] / sx
        out[r, 1] = m[r, 1] / sy
        out[r, 2] = m[r, 2] + m[r, 0] * (0.5 / sx - 0.5) + m[r, 1] * (0.5 / sy - 0.5)
    return out


def warp_affine_ragged(blob: torch.Tensor, srcs, mat: torch.Tensor, ok: torch.Tensor | None, output_size, border: int = 0,
                       family: str = "fixed", interpolation: str = "linear") -> torch.Tensor:
    """One crop per face from its own (h,w,3) image inside the device uint8 ``blob``: ``srcs`` (F,3) int64 host array of
    (byte offset, h, w) per face; ``mat`` (F,6) f64 device forward transforms; -> (F,oh,ow,3) u8.  ``family``,
    ``interpolation``: see ``warp_affine``."""
    _check_family(family)
    check_interpolation(interpolation, family)
    assert blob.dtype == torch.uint8 and blob.is_contiguous() and blob.dim() == 1
    srcs = np.asarray(srcs, np.int64).reshape(-1, 3)
    f = srcs.shape[0]
    rec = np.zeros(f, WARP_SRC_DTYPE)
    rec["off"], rec["h"], rec["w"] = srcs[:, 0], srcs[:, 1], srcs[:, 2]
    ow, oh = int(output_size[0]), int(output_size[1])
    mat = mat.contiguous()
    if interpolation != "linear":
        code = _INTERP_CODE[interpolation]
        if T.ENABLED:
            return T.load().warp_affine_u8_interp_ragged(blob, torch.from_numpy(rec.view(np.int64).reshape(f, 2)), mat, ok, ow,
                                                         oh, int(border), code)
        out = torch.empty((f, oh, ow, 3), dtype=torch.uint8, device=blob.device)
        rec_dev = torch.from_numpy(rec.view(np.uint8)).to(blob.device)
        N.check(N.lib().fcp_warp_affine_u8_interp_ragged(N.ptr(blob), blob.numel(), rec.ctypes.data, N.ptr(rec_dev), N.ptr(mat),
                                                         N.ptr(ok), f, oh, ow, int(border), code, N.ptr(out), N.stream_ptr()),
                "fcp_warp_affine_u8_interp_ragged")
        return out
    if T.ENABLED:
        return T.load().warp_affine_u8_ragged(blob, torch.from_numpy(rec.view(np.int64).reshape(f, 2)), mat, ok, ow, oh,
                                              int(border), _WARP_FAMILY_CODE[family])
    out = torch.empty((f, oh, ow, 3), dtype=torch.uint8, device=blob.device)
    rec_dev = torch.from_numpy(rec.view(np.uint8)).to(blob.device)
    entry = "fcp_warp_affine_u8_ragged" if family == "fixed" else "fcp_warp_affine_u8_float_ragged"
    N.check(getattr(N.lib(), entry)(N.ptr(blob), blob.numel(), rec.ctypes.data, N.ptr(rec_dev), N.ptr(mat), N.ptr(ok), f, oh,
                                    ow, int(border), N.ptr(out), N.stream_ptr()), entry)
    return out


def resize_area_ragged(src: torch.Tensor, levels, dst: torch.Tensor) -> None:
    """cv2.resize(INTER_AREA) of every row of ``levels`` ((n,6) int64 host array of (src_off, sh, sw, dst_off, dh, dw)):
    the (sh,sw,3) image at src_off of the device uint8 blob ``src`` into the (dh,dw,3) image at dst_off of ``dst``
    (dst_off a multiple of 4), one launch.  ``dst`` may be ``src`` itself when the regions do not overlap."""
    levels = np.asarray(levels, np.int64).reshape(-1, 6)
    n = levels.shape[0]
    if n == 0:
        return
    rec = np.zeros(n, AREA_LEVEL_DTYPE)
    for k, name in enumerate(AREA_LEVEL_DTYPE.names):
        rec[name] = levels[:, k]
    if T.ENABLED:
        T.load().resize_area_u8_ragged(src, torch.from_numpy(rec.view(np.int64).reshape(n, 4)), dst)
        return
    rec_dev = torch.from_numpy(rec.view(np.uint8)).to(src.device)
    N.check(N.lib().fcp_resize_area_ragged_u8(N.ptr(src), src.numel(), rec.ctypes.data, N.ptr(rec_dev), n, N.ptr(dst),
                                              dst.numel(), N.stream_ptr()), "fcp_resize_area_ragged_u8")


def plan_sources(table, idx, mats, ok):
    """Host plan of ``crop_align_sources`` for F faces: ``table`` (N,3) (offset, h, w) of the sources, ``idx`` (F,) image of
    each face, ``mats`` (F,6) forward transforms, ``ok`` (F,) flags.  -> (level jobs for ``resize_area_ragged``: one per
    distinct (image, L >= 1), packed after the last source at 16-byte aligned offsets; (F,3) source of each face for
    ``warp_affine_ragged``; (F,6) matrices on those sources; (F,) levels; bytes of the blob the plan needs)."""
    f = len(idx)
    levels = np.zeros(f, np.int64)
    for k in range(f):
        if ok[k]:
            levels[k] = pyramid_level(mats[k], int(table[idx[k], 2]), int(table[idx[k], 1]))
    pos = (int((table[:, 0] + table[:, 1] * table[:, 2] * 3).max()) + 15) // 16 * 16 if len(table) else 0
    slots, jobs = {}, []
    for i, lv in sorted({(int(i), int(lv)) for i, lv in zip(idx, levels) if lv > 0}):
        off, h, w = (int(v) for v in table[i])
        hl, wl = h >> lv, w >> lv
        slots[(i, lv)] = pos
        jobs.append((off, h, w, pos, hl, wl))
        pos += (hl * wl * 3 + 15) // 16 * 16
    srcs = np.zeros((f, 3), np.int64)
    mat_l = np.zeros((f, 6), np.float64)
    for k in range(f):
        off, h, w = (int(v) for v in table[idx[k]])
        lv = int(levels[k])
        srcs[k] = (off, h, w) if lv == 0 else (slots[(int(idx[k]), lv)], h >> lv, w >> lv)
        mat_l[k] = compose_level(mats[k], w, h, lv).reshape(6)
    return jobs, srcs, mat_l, levels, pos


def crop_align_sources(blob: torch.Tensor, table, img_idx, landmarks, target, output_size, border=0, allow_skew=False,
                       family="fixed", interpolation="linear"):
    """Device crop_align from the decoded originals (crop_source="original").  ``blob``, ``table``: the sources as
    ``batch.upload_sources`` / ``build_batch(keep_sources=True)`` return them (the blob has room for the levels after the
    last source); ``img_idx`` (F,) image of each face; ``landmarks`` (F,k,2) in source pixel coordinates.
    -> (crops (F,oh,ow,3) u8, ok (F,) i32 device, mat_L (F,6) f64 device: the transform applied to each face's level,
    level (F,) int64 host).  The matrices come back to the host once (with ok) to pick the levels; the level images
    are built in one launch, the crops in another.  ``family``, ``interpolation``: see ``warp_affine``; the levels are the
    same for every interpolation (they exist to shrink), the chosen filter then samples the level."""
    _check_family(family)
    check_interpolation(interpolation, family)
    dev = blob.device
    table = np.asarray(table, np.int64).reshape(-1, 3)
    if len(table) and int(table[:, 1:].max()) > MAX_SOURCE_SIDE:
        raise ValueError(f"crop_source='original' supports images of at most {MAX_SOURCE_SIDE} px a side")
    idx = np.asarray(img_idx.cpu() if isinstance(img_idx, torch.Tensor) else img_idx, np.int64).reshape(-1)
    f = len(idx)
    if f == 0:
        ow, oh = int(output_size[0]), int(output_size[1])
        return (torch.empty((0, oh, ow, 3), dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty((0, 6), dtype=torch.float64, device=dev), np.zeros(0, np.int64))
    landmarks = torch.as_tensor(landmarks).to(device=dev, dtype=torch.float32)
    if not isinstance(target, torch.Tensor):
        target = torch.from_numpy(np.ascontiguousarray(target, dtype=np.float32))
    mat, ok = estimate_transform(landmarks, target.to(dev), allow_skew)
    both = torch.cat([mat, ok.to(torch.float64)[:, None]], 1).cpu().numpy()      # one read-back: matrices and ok
    jobs, srcs, mat_l, levels, need = plan_sources(table, idx, both[:, :6], both[:, 6] != 0)
    if need > blob.numel():
        raise ValueError(f"the source blob ({blob.numel()} bytes) has no room for the levels ({need} bytes needed): "
                         f"upload the sources with batch.upload_sources or build_batch(keep_sources=True)")
    resize_area_ragged(blob, jobs, blob)
    mat_l_dev = torch.from_numpy(mat_l).to(dev)
    crops = warp_affine_ragged(blob, srcs, mat_l_dev, ok, output_size, border, family, interpolation)
    return crops, ok, mat_l_dev, levels
