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


def warp_affine(images_u8: torch.Tensor, img_idx: torch.Tensor, mat: torch.Tensor, ok: torch.Tensor | None,
                paddings: torch.Tensor | None, output_size, border: int = 0, family: str = "fixed") -> torch.Tensor:
    """images (n,h,w,3) u8 device; output_size = (width, height) like cv2's dsize; ``family``: one of ``WARP_FAMILIES``."""
    _check_family(family)
    assert images_u8.dtype == torch.uint8 and images_u8.is_contiguous() and images_u8.shape[3] == 3
    n, h, w, _ = images_u8.shape
    f = img_idx.shape[0]
    ow, oh = int(output_size[0]), int(output_size[1])
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
               face_count=None, valid_total=None, family="fixed"):
    """Device crop_align: -> (crops (F,oh,ow,3) u8, ok (F,) i32, mat (F,6) f64).  Faces
    with ok == 0 (degenerate transform) are dropped by the caller like cropper.py:529-531.
    ``face_count`` / ``valid_total``: see ``estimate_transform``; ``family``: see ``warp_affine``."""
    _check_family(family)
    dev = images_u8.device
    landmarks = landmarks.to(device=dev, dtype=torch.float32)
    if not isinstance(target, torch.Tensor):
        target = torch.from_numpy(np.ascontiguousarray(target, dtype=np.float32))
    target = target.to(dev)
    img_idx = img_idx.to(device=dev, dtype=torch.int32).contiguous()
    if paddings is not None:
        paddings = paddings.to(device=dev, dtype=torch.int32).contiguous()
    mat, ok = estimate_transform(landmarks, target, allow_skew, face_count, valid_total)
    crops = warp_affine(images_u8, img_idx, mat, ok, paddings, output_size, border, family)
    return crops, ok, mat
