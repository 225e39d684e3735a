"""Contrast-limited adaptive histogram equalisation of aligned crops (``Cropper(clahe=...)``):
the luma of every crop is equalised tile by tile on the device, ``cv2.createCLAHE(clip_limit, (grid, grid)).apply(Y)``
between ``cv2.cvtColor(crop, COLOR_RGB2YCrCb)`` and ``cvtColor(..., COLOR_YCrCb2RGB)`` restated, as two launches on the
crops that are on the device already (``fcp_clahe_u8`` / ``torch.ops.fcp.clahe``).

    Y, Cr, Cb = OpenCV's 8-bit RGB -> YCrCb in 14-bit fixed point; only Y changes
    LUT       = per tile of the grid x grid tiling (the plane reflected-101 up to a multiple of grid): histogram, clip at
                max(int(clip_limit * area / 256), 1), redistribute the excess, prefix sum, rint(s * 255 / area) in float32
    Y'        = the four LUTs around the pixel, interpolated bilinearly in float32 and rounded half to even
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from . import torch_ops as T

MAX_GRID = 16
DEFAULT_GRID = 8
MAX_SIDE = 4096


def _is_number(v) -> bool:
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def check_clahe(clahe):
    """``clahe`` of the Cropper -> None (off) or the clip limit as a float: finite and > 0."""
    if clahe is None:
        return None
    if not _is_number(clahe) or not np.isfinite(clahe) or clahe <= 0:
        raise ValueError(f"clahe must be None or a finite clip limit > 0, not {clahe!r}")
    return float(clahe)


def check_grid(grid, output_size=None) -> int:
    """``clahe_grid`` of the Cropper -> 1..16 (None: 8); with ``output_size`` (w, h), both sides must be at least
    ``2 * grid``."""
    if grid is None:
        grid = DEFAULT_GRID
    if not _is_number(grid) or not np.isfinite(grid) or int(grid) != grid or not 1 <= int(grid) <= MAX_GRID:
        raise ValueError(f"clahe_grid must be an int 1..{MAX_GRID} or None, not {grid!r}")
    grid = int(grid)
    if output_size is not None and min(output_size) < 2 * grid:
        raise ValueError(f"clahe_grid {grid} needs an output_size of at least {2 * grid} x {2 * grid}, not {tuple(output_size)}")
    return grid


def clahe(crops_dev: torch.Tensor, clip_limit: float, grid: int = DEFAULT_GRID) -> torch.Tensor:
    """crops (F,H,W,3) u8, device -> the equalised crops (F,H,W,3) u8, device.  Two launches; 2 * grid <= H, W <= 4096."""
    assert crops_dev.dtype == torch.uint8 and crops_dev.is_contiguous() and crops_dev.dim() == 4 and crops_dev.shape[3] == 3
    if T.ENABLED:
        return T.load().clahe(crops_dev, int(grid), float(clip_limit))
    f, h, w, _ = crops_dev.shape
    out = torch.empty_like(crops_dev)
    luts = torch.empty((f, max(int(grid), 0), max(int(grid), 0), 256), dtype=torch.uint8, device=crops_dev.device)
    N.check(N.lib().fcp_clahe_u8(N.ptr(crops_dev), f, h, w, int(grid), float(clip_limit), N.ptr(luts), N.ptr(out), N.stream_ptr()),
            "fcp_clahe_u8")
    return out
