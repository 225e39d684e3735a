"""Background replacement of aligned crops (``Cropper(background=...)``): label map -> soft
alpha -> composite over a uniform fill, in integers from end to end, as one launch on the crops and the label map that
are on the device already (``fcp_matte_u8`` / ``torch.ops.fcp.matte``).

    m     = 255 where the label is one of the foreground classes, else 0
    alpha = m (feather 0), or cv2.GaussianBlur(m, (feather, feather), 0) restated: the 8.8 fixed-point taps of ksize 3,
            5 or 7, two passes, one rounding ``(sum + 32768) >> 16``, BORDER_REFLECT_101
    out   = (crop * alpha + fill * (255 - alpha) + 127) // 255
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from . import torch_ops as T

FEATHERS = (0, 3, 5, 7)
DEFAULT_FEATHER = 5
NUM_CLASSES = 19            # bise.NUM_CLASSES: the label maps are BiSeNet's


def _is_int(v) -> bool:
    if isinstance(v, (bool, np.bool_)):
        return False
    return isinstance(v, (int, np.integer)) or (isinstance(v, (float, np.floating)) and np.isfinite(v) and float(v) == int(v))


def check_background(background):
    """``background`` of the Cropper -> None (off) or the fill (r, g, b): an int 0..255 (gray) or three of them."""
    if background is None:
        return None
    values = [background] * 3 if _is_int(background) else background
    if isinstance(values, (str, bytes)) or not hasattr(values, "__len__") or len(values) != 3 or not all(_is_int(v) for v in values):
        raise ValueError(f"background must be None, an int 0..255 or three of them (R, G, B), not {background!r}")
    fill = tuple(int(v) for v in values)
    if min(fill) < 0 or max(fill) > 255:
        raise ValueError(f"background components must be 0..255, not {background!r}")
    return fill


def check_foreground(foreground) -> int:
    """``foreground`` of the Cropper -> the class bit set: None is every class but 0 (1..18)."""
    if foreground is None:
        return sum(1 << c for c in range(1, NUM_CLASSES))
    try:
        classes = list(foreground)
    except TypeError:
        raise ValueError(f"foreground must be an iterable of class indices 0..{NUM_CLASSES - 1}, not {foreground!r}") from None
    if len(classes) == 0 or not all(_is_int(c) and 0 <= int(c) < NUM_CLASSES for c in classes):
        raise ValueError(f"foreground must name at least one class, each 0..{NUM_CLASSES - 1}, not {foreground!r}")
    bits = 0
    for c in classes:
        bits |= 1 << int(c)
    return bits


def check_feather(feather) -> int:
    """``feather`` of the Cropper -> 0, 3, 5 or 7 (None: 5)."""
    if feather is None:
        return DEFAULT_FEATHER
    if not _is_int(feather) or int(feather) not in FEATHERS:
        raise ValueError(f"feather must be one of {FEATHERS} or None, not {feather!r}")
    return int(feather)


def matte(crops_dev: torch.Tensor, labels_dev: torch.Tensor, class_bits: int, feather: int, fill, with_alpha: bool = False):
    """crops (F,H,W,3) u8 and labels (F,H,W) u8, device -> (out (F,H,W,3) u8, alpha (F,H,W) u8 or None), device.  One
    launch; H, W <= 8192."""
    assert crops_dev.dtype == torch.uint8 and crops_dev.is_contiguous() and crops_dev.dim() == 4 and crops_dev.shape[3] == 3
    assert labels_dev.dtype == torch.uint8 and labels_dev.is_contiguous() and tuple(labels_dev.shape) == tuple(crops_dev.shape[:3])
    r, g, b = (int(v) for v in fill)
    if T.ENABLED:
        out, alpha = T.load().matte(crops_dev, labels_dev, int(class_bits), int(feather), r, g, b, bool(with_alpha))
        return out, (alpha if with_alpha else None)
    f, h, w, _ = crops_dev.shape
    out = torch.empty_like(crops_dev)
    alpha = torch.empty((f, h, w), dtype=torch.uint8, device=crops_dev.device) if with_alpha else None
    N.check(N.lib().fcp_matte_u8(N.ptr(crops_dev), N.ptr(labels_dev), f, h, w, int(class_bits), int(feather), r, g, b,
                                 N.ptr(out), N.ptr(alpha), N.stream_ptr()), "fcp_matte_u8")
    return out, alpha
