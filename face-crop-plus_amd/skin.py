"""Parser-guided skin smoothing of aligned crops (``Cropper(smooth_skin=S)``): a bilateral
filter that changes only the pixels the face parser labels skin, averages only over such pixels and leaves every other
pixel of the crop byte-identical, so that eyes, brows, lips and hair keep their detail and their colour does not bleed
into the cheek; in integers, as one launch on the crops and the label maps that are on the device already
(``fcp_skin_smooth_u8`` / ``torch.ops.fcp.skin_smooth``).  The arithmetic is this project's own definition, held byte for
byte to ``tests/skin_ref.py``:

    t[0..r]  : integer taps, each <= 4096, 3 <= r <= 24.  The option uses matte.blur_taps(smooth_sigma).
    rng      : the range table, 256 x uint16.  The option uses range_lut(S).
    g(p)     = (9798 R + 19235 G + 3735 B + 16384) >> 15                    the gray of min_sharpness
    m(p)     = 1 if l(p) < 32 and bit l(p) of the class bits is set, else 0; m = 0 outside the crop (no reflection)
    s(o)     = (t[|oy|] * t[|ox|] + 2048) >> 12                             o in [-r, r]^2
    w(p, o)  = m(p + o) * ((s(o) * min(rng[|g(p + o) - g(p)|], 4096) + 2048) >> 12)
    W(p)     = sum over o of w(p, o)
    b_c(p)   = (sum over o of w(p, o) c_c(p + o) + (W >> 1)) // W           c = R, G, B; W == 0: b = c(p)
    alpha(p) = matte.feather_alpha(l, bits, 7)                              the shared feather, reflect-101 borders
    e(p)     = max(0, 2 alpha(p) - 255);   E(p) = (e(p) * A + 128) >> 8     A = round(256 smooth_amount), 1..256
    out_c(p) = (b_c E + c_c (255 - E) + 127) // 255 if m(p) == 1, else c_c(p)

The ramp ``e`` goes from 0 at the edge of the skin region to 255 about three pixels inside it, so the jagged, slightly
misplaced label boundary does not show as a seam.  ``range_lut`` builds the table of a strength on the host, in float64,
once; the taps are host data and travel in the kernel's argument block.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _native as N
from . import matte as matting
from . import torch_ops as T

MIN_STRENGTH, MAX_STRENGTH = 1, 64
MIN_SIGMA, MAX_SIGMA = 0.5, 8
DEFAULT_SIGMA = 3.0
MIN_AMOUNT, MAX_AMOUNT = 0.05, 1
DEFAULT_CLASSES = (1, 7, 8, 10, 14)      # BiSeNet: skin, both ears, nose, neck
MIN_RADIUS, MAX_RADIUS = 3, 24
ONE = 4096
RANGE = 256
FEATHER = 7

_tables = {}                             # (device, S) -> the range table on the device
_taps = {}                               # sigma -> matte.blur_taps(sigma)


def _is_number(v) -> bool:
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def check_smooth_skin(smooth_skin):
    """``smooth_skin`` of the Cropper -> None (off) or the range strength S, in gray levels, as a float: finite, 1..64."""
    if smooth_skin is None:
        return None
    if not _is_number(smooth_skin) or not np.isfinite(smooth_skin) or not MIN_STRENGTH <= smooth_skin <= MAX_STRENGTH:
        raise ValueError(f"smooth_skin must be None or a finite range strength {MIN_STRENGTH}..{MAX_STRENGTH} (gray levels), "
                         f"not {smooth_skin!r}")
    return float(smooth_skin)


def check_sigma(smooth_sigma) -> float:
    """``smooth_sigma`` of the Cropper -> the spatial sigma in output pixels as a float (None: 3.0): finite, 0.5..8."""
    if smooth_sigma is None:
        return DEFAULT_SIGMA
    if not _is_number(smooth_sigma) or not np.isfinite(smooth_sigma) or not MIN_SIGMA <= smooth_sigma <= MAX_SIGMA:
        raise ValueError(f"smooth_sigma must be None or a finite sigma in [{MIN_SIGMA}, {MAX_SIGMA}] pixels, not {smooth_sigma!r}")
    return float(smooth_sigma)


def check_amount(smooth_amount) -> float:
    """``smooth_amount`` of the Cropper -> how much of the smoothed skin replaces the crop's, a float (None: 1.0): finite,
    0.05..1."""
    if smooth_amount is None:
        return 1.0
    if not _is_number(smooth_amount) or not np.isfinite(smooth_amount) or not MIN_AMOUNT <= smooth_amount <= MAX_AMOUNT:
        raise ValueError(f"smooth_amount must be None or a finite amount in [{MIN_AMOUNT}, {MAX_AMOUNT}], not {smooth_amount!r}")
    return float(smooth_amount)


def check_classes(skin_classes) -> int:
    """``skin_classes`` of the Cropper -> the class bit set: None is (1, 7, 8, 10, 14); else at least one class, each
    0..18, as ``foreground`` has it."""
    if skin_classes is None:
        return sum(1 << c for c in DEFAULT_CLASSES)
    try:
        classes = list(skin_classes)
    except TypeError:
        raise ValueError(f"skin_classes must be an iterable of class indices 0..{matting.NUM_CLASSES - 1}, not {skin_classes!r}") from None
    if len(classes) == 0 or not all(matting._is_int(c) and 0 <= int(c) < matting.NUM_CLASSES for c in classes):
        raise ValueError(f"skin_classes must name at least one class, each 0..{matting.NUM_CLASSES - 1}, not {skin_classes!r}")
    bits = 0
    for c in classes:
        bits |= 1 << int(c)
    return bits


def range_lut(strength: float):
    """The range strength S -> rng[0..255] as uint16: rng[d] = floor(4096 exp(-d^2 / (2 S^2)) + 0.5), in float64.
    rng[0] == 4096 and the table never increases."""
    d = np.arange(RANGE, dtype=np.float64)
    return np.floor(ONE * np.exp(-(d * d) / (2.0 * float(strength) * float(strength))) + 0.5).astype(np.uint16)


def amount_q8(amount) -> int:
    """The amount -> A = round(256 amount), 13..256 over the range of ``smooth_amount``."""
    return int(round(256 * float(amount)))


def taps_of(sigma) -> list:
    """``matte.blur_taps(sigma)``, made once per sigma: r = max(3, ceil(3 sigma)) = 3..24 over the range of
    ``smooth_sigma``."""
    key = float(sigma)
    if key not in _taps:
        _taps[key] = matting.blur_taps(key)
    return _taps[key]


def skin_smooth(crops_dev: torch.Tensor, labels_dev: torch.Tensor, class_bits: int, taps, lut_dev: torch.Tensor,
                amount_q8: int) -> torch.Tensor:
    """crops (F,H,W,3) u8 and labels (F,H,W) u8, device; any taps t[0..r] (integers <= 4096, host), 3 <= r <= 24; any
    table lut (256,) uint16, device; amount_q8 1..256 -> the smoothed crops (F,H,W,3) u8, device.  One launch;
    1 <= H, W <= 8192."""
    assert crops_dev.dtype == torch.uint8 and crops_dev.is_contiguous() and crops_dev.dim() == 4 and crops_dev.shape[3] == 3
    assert labels_dev.dtype == torch.uint8 and labels_dev.is_contiguous() and tuple(labels_dev.shape) == tuple(crops_dev.shape[:3])
    assert labels_dev.device == crops_dev.device
    assert lut_dev.dtype == torch.uint16 and lut_dev.is_contiguous() and tuple(lut_dev.shape) == (RANGE,) and lut_dev.device == crops_dev.device
    taps = [int(t) for t in taps]
    if T.ENABLED:
        return T.load().skin_smooth(crops_dev, labels_dev, int(class_bits), taps, lut_dev, int(amount_q8))
    if not MIN_RADIUS + 1 <= len(taps) <= MAX_RADIUS + 1 or min(taps) < 0 or max(taps) > 65535:
        raise RuntimeError(f"fcp_skin_smooth_u8: taps must be t[0..radius] with radius {MIN_RADIUS}..{MAX_RADIUS}, each 16 bits "
                           f"(got {len(taps)} taps)")
    f, h, w, _ = crops_dev.shape
    out = torch.empty_like(crops_dev)
    t16 = (ctypes.c_uint16 * len(taps))(*taps)
    N.check(N.lib().fcp_skin_smooth_u8(N.ptr(crops_dev), N.ptr(labels_dev), f, h, w, int(class_bits), t16, len(taps) - 1,
                                       N.ptr(lut_dev), int(amount_q8), N.ptr(out), N.stream_ptr()), "fcp_skin_smooth_u8")
    return out


def smooth(crops_dev: torch.Tensor, labels_dev: torch.Tensor, strength: float, sigma: float = DEFAULT_SIGMA, amount: float = 1.0,
           class_bits: int | None = None) -> torch.Tensor:
    """crops (F,H,W,3) u8 and their label maps (F,H,W) u8, device -> the crops with the skin (``class_bits``; None: the
    default classes) smoothed at range strength S (``range_lut``), spatial sigma ``sigma`` (``matte.blur_taps``) and
    ``amount``, device.  The table is uploaded once per (device, S) and reused."""
    key = (crops_dev.device, float(strength))
    if key not in _tables:
        _tables[key] = torch.from_numpy(range_lut(strength)).to(crops_dev.device)
    bits = check_classes(None) if class_bits is None else int(class_bits)
    return skin_smooth(crops_dev, labels_dev, bits, taps_of(sigma), _tables[key], amount_q8(amount))
