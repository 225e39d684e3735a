"""Unsharp-mask sharpening of aligned crops (``Cropper(sharpen=A)``): the gray's difference
from its own Gaussian blur, cored by a threshold and scaled by the amount, is added to all three channels alike, so there
are no colour fringes; in integers, as one launch on the crops that are on the device already (``fcp_unsharp_u8`` /
``torch.ops.fcp.unsharp``).  The arithmetic is this project's own definition, held byte for byte to
``tests/sharpen_ref.py``:

    t[0..r]  : integer taps, t[0] + 2 sum(t[1..r]) == 4096, 1 <= r <= 48.  The option uses matte.blur_taps(S).
    g        = (9798 R + 19235 G + 3735 B + 16384) >> 15          the gray of min_sharpness
    coordinates outside the crop are clamped to its edge          BORDER_REPLICATE: any H, W >= 1
    Hs(y,x)  = sum_i t|i| g(y, clamp(x + i))                      <= 255 * 4096
    B(y,x)   = sum_j t|j| Hs(clamp(y + j), x)                     <= 255 * 2^24 < 2^32, unsigned
    b8       = (B + 32768) >> 16                                  the blurred gray with 8 fraction bits
    d        = (g << 8) - b8                                      |d| <= 65280
    e        = sign(d) * max(|d| - (T << 8), 0)                   soft threshold (coring), T = 0..255 gray levels
    A_q      = floor(256 A + 0.5), 1..1024                        the amount: 1.0 adds the whole difference
    v_c      = (c << 16) + A_q * e + 32768                        c = R, G, B; |A_q e| <= 66 846 720: signed 32 bits
    out_c    = v_c < 0 ? 0 : min(255, v_c >> 16)

``T = 255`` copies the crop, and so do the taps ``[4096, 0, 0, 0]``.  The taps are host data: they travel in the kernel's
argument block, so ``sharpen`` makes those of a sigma once and uploads nothing.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _native as N
from . import matte as matting
from . import torch_ops as T

MIN_AMOUNT, MAX_AMOUNT = 0.05, 4
DEFAULT_SIGMA = 1.5
MIN_SIGMA, MAX_SIGMA = matting.MIN_SIGMA, matting.MAX_SIGMA
MAX_RADIUS = 48
TAP_SUM = 4096

_taps = {}                               # sigma -> matte.blur_taps(sigma)


def _is_number(v) -> bool:
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def check_sharpen(sharpen):
    """``sharpen`` of the Cropper -> None (off) or the amount A as a float: finite, 0.05..4; 1.0 adds the whole difference
    between the gray and its blur."""
    if sharpen is None:
        return None
    if not _is_number(sharpen) or not np.isfinite(sharpen) or not MIN_AMOUNT <= sharpen <= MAX_AMOUNT:
        raise ValueError(f"sharpen must be None or a finite amount in [{MIN_AMOUNT}, {MAX_AMOUNT}], not {sharpen!r}")
    return float(sharpen)


def check_sigma(sharpen_sigma) -> float:
    """``sharpen_sigma`` of the Cropper -> the sigma of the blur in output pixels as a float (None: 1.5): finite, 0.5..16,
    the range of ``background_blur`` (the taps are ``matte.blur_taps``')."""
    if sharpen_sigma is None:
        return DEFAULT_SIGMA
    if not _is_number(sharpen_sigma) or not np.isfinite(sharpen_sigma) or not MIN_SIGMA <= sharpen_sigma <= MAX_SIGMA:
        raise ValueError(f"sharpen_sigma must be None or a finite sigma in [{MIN_SIGMA}, {MAX_SIGMA}] pixels, not {sharpen_sigma!r}")
    return float(sharpen_sigma)


def check_threshold(sharpen_threshold) -> int:
    """``sharpen_threshold`` of the Cropper -> the coring threshold T in gray levels, an int 0..255 (None: 0)."""
    if sharpen_threshold is None:
        return 0
    if isinstance(sharpen_threshold, (bool, np.bool_)) or not isinstance(sharpen_threshold, (int, np.integer)) or \
            not 0 <= int(sharpen_threshold) <= 255:
        raise ValueError(f"sharpen_threshold must be None or an int 0..255 (gray levels), not {sharpen_threshold!r}")
    return int(sharpen_threshold)


def amount_q8(amount) -> int:
    """The amount A -> A_q = floor(256 A + 0.5), 13..1024 over the range of ``sharpen``."""
    return int(math.floor(256.0 * float(amount) + 0.5))


def unsharp(crops_dev: torch.Tensor, taps, amount_q8: int, threshold: int) -> torch.Tensor:
    """crops (F,H,W,3) u8, device; any taps t[0..r] (integers, host), 1 <= r <= 48, that sum to 4096 over the window;
    amount_q8 1..1024; threshold 0..255 -> the sharpened crops (F,H,W,3) u8, device.  One launch; H, W <= 8192."""
    assert crops_dev.dtype == torch.uint8 and crops_dev.is_contiguous() and crops_dev.dim() == 4 and crops_dev.shape[3] == 3
    taps = [int(t) for t in taps]
    if T.ENABLED:
        return T.load().unsharp(crops_dev, taps, int(amount_q8), int(threshold))
    if not 2 <= len(taps) <= MAX_RADIUS + 1 or min(taps) < 0 or max(taps) > 65535:
        raise RuntimeError(f"fcp_unsharp_u8: taps must be t[0..radius] with radius 1..{MAX_RADIUS}, each 16 bits (got {len(taps)} taps)")
    f, h, w, _ = crops_dev.shape
    out = torch.empty_like(crops_dev)
    t16 = (ctypes.c_uint16 * len(taps))(*taps)
    N.check(N.lib().fcp_unsharp_u8(N.ptr(crops_dev), f, h, w, t16, len(taps) - 1, int(amount_q8), int(threshold), N.ptr(out),
                                   N.stream_ptr()), "fcp_unsharp_u8")
    return out


def sharpen(crops_dev: torch.Tensor, amount: float, sigma: float = DEFAULT_SIGMA, threshold: int = 0) -> torch.Tensor:
    """crops (F,H,W,3) u8, device -> the crops sharpened by ``amount`` times their gray's difference from its Gaussian of
    ``sigma`` (``matte.blur_taps``), cored at ``threshold`` gray levels, device.  The taps are made once per sigma."""
    key = float(sigma)
    if key not in _taps:
        _taps[key] = matting.blur_taps(key)
    return unsharp(crops_dev, _taps[key], amount_q8(amount), threshold)
