"""Non-local-means noise removal of aligned crops (``Cropper(denoise=H)``): every pixel becomes
the weighted mean of the 21 x 21 pixels around it, each weighted by how much its 7 x 7 gray patch resembles the pixel's
own, in integers, as one launch on the crops that are on the device already (``fcp_nlm_denoise_u8`` /
``torch.ops.fcp.nlm_denoise``).  The window sizes are the defaults of ``cv2.fastNlMeansDenoising``; the arithmetic is this
project's own definition, held byte for byte to ``tests/denoise_ref.py``:

    P = 3, S = 10, ONE = 4096; coordinates outside the crop are reflected (BORDER_REFLECT_101): H, W >= 14
    g        = (9798 R + 19235 G + 3735 B + 16384) >> 15                      the gray of min_sharpness
    d(p,o)   = sum over t in [-P,P]^2 of (g(p + t) - g(p + o + t))^2          for every offset o in [-S,S]^2
    k        = d >> shift;  w(p,o) = min(lut[k], ONE) if k < n, else 0
    W        = sum over o of w(p,o)
    out_c(p) = (sum over o of w(p,o) c(p + o) + (W >> 1)) // W                c = R, G, B; W == 0 copies the pixel

The weights come from the gray alone and the three channels are averaged with them, so pure chroma noise is reduced less
than luma noise.  ``weight_lut`` builds the table of a filter strength on the host, in float64, once.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native as N
from . import torch_ops as T

PATCH_RADIUS = 3
SEARCH_RADIUS = 10
MIN_SIDE = PATCH_RADIUS + SEARCH_RADIUS + 1
ONE = 4096
MAX_LUT = 4096
MIN_STRENGTH, MAX_STRENGTH = 1, 32

_PATCH = (2 * PATCH_RADIUS + 1) ** 2
_tables = {}                             # (device, H) -> (table on the device, shift)


def _is_number(v) -> bool:
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def check_denoise(denoise):
    """``denoise`` of the Cropper -> None (off) or the filter strength H, in gray levels, as a float: finite, 1..32."""
    if denoise is None:
        return None
    if not _is_number(denoise) or not np.isfinite(denoise) or not MIN_STRENGTH <= denoise <= MAX_STRENGTH:
        raise ValueError(f"denoise must be None or a finite filter strength {MIN_STRENGTH}..{MAX_STRENGTH} (gray levels), not {denoise!r}")
    return float(denoise)


def check_size(output_size):
    """The ``output_size`` (w, h) of a Cropper with ``denoise``: at least 14 x 14, so that one reflection reaches every
    coordinate of a window."""
    if min(output_size) < MIN_SIDE:
        raise ValueError(f"denoise needs an output_size of at least {MIN_SIDE} x {MIN_SIDE}, not {tuple(output_size)}")


def weight_lut(strength: float):
    """The filter strength H -> (lut, shift): lut[k] = floor(ONE exp(-(k 2^shift) / (49 H^2)) + 0.5) as uint16, for every
    k up to where the weight falls below one half; ``shift`` is the least that keeps the table within 4096 entries.
    lut[0] == ONE, the table never increases and every entry is at least 1."""
    scale = float(_PATCH) * float(strength) * float(strength)
    cut = int(math.floor(math.log(2.0 * ONE) * scale))
    shift = 0
    while (cut >> shift) >= MAX_LUT:
        shift += 1
    k = np.arange((cut >> shift) + 1, dtype=np.float64)
    return np.floor(ONE * np.exp(-(k * float(1 << shift)) / scale) + 0.5).astype(np.uint16), shift


def nlm(crops_dev: torch.Tensor, lut_dev: torch.Tensor, shift: int) -> torch.Tensor:
    """crops (F,H,W,3) u8, device; any table lut (n,) uint16, device, n 1..4096; shift 0..10 -> the denoised crops
    (F,H,W,3) u8, device.  One launch; 14 <= H, W <= 8192."""
    assert crops_dev.dtype == torch.uint8 and crops_dev.is_contiguous() and crops_dev.dim() == 4 and crops_dev.shape[3] == 3
    assert lut_dev.dtype == torch.uint16 and lut_dev.is_contiguous() and lut_dev.dim() == 1 and lut_dev.device == crops_dev.device
    if T.ENABLED:
        return T.load().nlm_denoise(crops_dev, lut_dev, int(shift))
    f, h, w, _ = crops_dev.shape
    out = torch.empty_like(crops_dev)
    N.check(N.lib().fcp_nlm_denoise_u8(N.ptr(crops_dev), f, h, w, N.ptr(lut_dev), lut_dev.shape[0], int(shift), N.ptr(out),
                                       N.stream_ptr()), "fcp_nlm_denoise_u8")
    return out


def denoise(crops_dev: torch.Tensor, strength: float) -> torch.Tensor:
    """crops (F,H,W,3) u8, device -> the crops denoised at filter strength H (``weight_lut``), device.  The table is
    uploaded once per (device, H) and reused."""
    key = (crops_dev.device, float(strength))
    if key not in _tables:
        lut, shift = weight_lut(strength)
        _tables[key] = (torch.from_numpy(lut).to(crops_dev.device), shift)
    return nlm(crops_dev, *_tables[key])
