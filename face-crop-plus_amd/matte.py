"""Background replacement of aligned crops (``Cropper(background=...)``): label map -> soft
alpha -> composite over a uniform fill, in integers from end to end, as one launch on the crops and the label map that
are on the device already (``fcp_matte_u8`` / ``torch.ops.fcp.matte``).

    m     = 255 where the label is one of the foreground classes, else 0
    alpha = m (feather 0), or cv2.GaussianBlur(m, (feather, feather), 0) restated: the 8.8 fixed-point taps of ksize 3,
            5 or 7, two passes, one rounding ``(sum + 32768) >> 16``, BORDER_REFLECT_101
    out   = (crop * alpha + fill * (255 - alpha) + 127) // 255

``Cropper(background_blur=sigma)`` (section 2i) keeps the background and blurs it instead: the fill of a pixel becomes

    B     = (N + D // 2) // D,  N and D the Gaussian window sums of the BACKGROUND pixels' colours and of their count
            (``fcp_matte_blur_u8`` / ``torch.ops.fcp.matte_blur``, two launches), with integer taps made here from sigma

``Cropper(refine=R)`` (section 2k) replaces the Gaussian feather by a guided filter of the hard mask, the gray of the
crop as the guide (``refine_alpha``: ``fcp_matte_refine_u8`` / ``torch.ops.fcp.matte_refine``, two launches); ``matte``
and ``matte_blur`` then composite through that plane (``alpha=``).

``Cropper(subject="largest", fill_holes=N)`` (section 2l) cleans the hard mask before any of that (``subject_mask``:
``fcp_subject_mask_u8`` / ``torch.ops.fcp.subject_mask``), every face on its own, H and W the crop's size:

    m0(y,x) = 1 where labels(y,x) < 19 and bit labels(y,x) of class_bits is set, else 0
    subject="largest": the 8-connected components of {m0 = 1}; a component's key is (its pixel count, then the SMALLER
            raster index y*W + x of its first pixel in raster order); m1 = the component with the largest count, among
            equal counts the one whose first pixel comes first; no foreground pixel: m1 = m0.  Otherwise m1 = m0.
    fill_holes=N: the 4-connected components of {m1 = 0}; a hole is one that has no pixel in row 0, row H-1, column 0
            or column W-1; m2 = m1, plus every hole of at most N pixels.  Otherwise m2 = m1.
    out(y,x) = m2(y,x), one byte, 0 or 1

The subject comes first, then the holes: an island inside a hole is background by then and counts in the hole's area.
``out`` takes the label map's place downstream, with the class bit set ``SUBJECT_BITS`` (class 1).

``Cropper(background="transparent")`` (section 2n) writes no fill at all: the crop becomes an RGBA cut-out
``(colour, alpha)``, ``(0, 0, 0, 0)`` where alpha is 0 (``feather_alpha`` + ``cutout``: ``fcp_feather_alpha_u8``,
``fcp_cutout_u8``).  ``Cropper(decontaminate=sigma)`` replaces the crop's colour in the soft edge, which is already mixed
with the old background, by an estimate of the subject's own, for the cut-out and for the composite over a uniform fill:

    sF, sB = 1 where alpha == 255 / where alpha == 0: the pixels that are certainly subject / certainly background
    F^, B^ = the mask-normalised Gaussians of the crop over sF / over sB (``blur_taps(sigma)``; the crop's colour where
             the window holds no such pixel)
    R      = 255 c - (alpha F^ + (255 - alpha) B^)
    F      = clamp((65025 F^ + alpha R + 32512) // 65025, 0, 255) where 0 < alpha < 255, else c

``Cropper(edge_shift=N)`` (section 2o) moves the boundary of the hard mask out (N > 0) or in (N < 0) by |N| pixels after
``subject`` / ``fill_holes`` and before every soft edge (``shift_mask``: ``fcp_mask_shift_u8`` /
``torch.ops.fcp.mask_shift``), every face on its own: binary morphology with a Euclidean disc, r = |N|:

    m0(y,x) = (class_bits >> labels(y,x)) & 1; only positions inside the crop exist: a pixel outside the crop is neither
            subject nor background, and it is never a source
    N > 0 (grow): out(y,x) = 1 iff some (y',x') inside the crop has m0 = 1 and (y-y')^2 + (x-x')^2 <= r^2
    N < 0 (shrink): out(y,x) = 1 iff m0(y,x) = 1 and no (y',x') inside the crop has m0 = 0 and (y-y')^2 + (x-x')^2 <= r^2
    out(y,x) is one byte, 0 or 1, and takes the label map's place downstream like ``subject_mask``'s (``SUBJECT_BITS``)

A shrink does not eat inwards from the crop's border: shoulders that touch the bottom row stay there.

``Cropper(background_image=...)`` (section 2r) puts the subject in front of a picture: the fill of a pixel becomes the
byte of the face's picture P at the pixel's own position,

    out   = (crop * alpha + P * (255 - alpha) + 127) // 255           (the subject's colour F for the crop with
            ``decontaminate``)

with the alpha the mode already has (``matte_image`` / ``cutout_image``: ``fcp_matte_image_u8``,
``fcp_matte_image_alpha_u8``, ``fcp_cutout_image_u8``, the kernels of the fill with the picture as their fill source).
The pictures are fitted to the output size once, on the host (``picture_bank``), and stay on the device as a bank
(K, H, W, 3); face i reads picture ``picks[i]``, which ``pick_pictures`` makes from the name of the face's file.
"""
from __future__ import annotations

import ctypes
import math
import os
import zlib

import numpy as np
import torch

from . import _native as N
from . import torch_ops as T

FEATHERS = (0, 3, 5, 7)
DEFAULT_FEATHER = 5
NUM_CLASSES = 19            # bise.NUM_CLASSES: the label maps are BiSeNet's
MIN_SIGMA, MAX_SIGMA = 0.5, 16.0
MIN_RADIUS, MAX_RADIUS = 3, 48
TAP_SUM = 4096
MIN_REFINE, MAX_REFINE = 1, 16
MIN_REFINE_EPS, MAX_REFINE_EPS, DEFAULT_REFINE_EPS = 1, 4096, 64
SUBJECTS = ("largest",)
MAX_FILL_HOLES = 8192 * 8192   # the largest crop the kernels take
SUBJECT_BITS = 1 << 1          # the class bit set that reads ``subject_mask``'s 0 / 1 output as a label map: class 1
TRANSPARENT = "transparent"    # ``check_background``'s answer for the RGBA cut-out: no fill, the alpha ships in the file
CUTOUT_RGBA, CUTOUT_FILL = 0, 1   # fcp_hip.h: FCP_CUTOUT_RGBA, FCP_CUTOUT_FILL
MAX_EDGE_SHIFT = 64            # the largest |edge_shift|, in output pixels: the halo a tile of fcp_mask_shift_u8 stages
FITS = ("cover", "stretch")    # ``background_fit``: a uniform scale that covers the crop, centre-cropped; or both axes on their own
DEFAULT_FIT = "cover"
MAX_PICTURES = 4096            # csrc/fcp_fill.h: kMaxPictures
MAX_BANK_BYTES = 1 << 30       # of device memory a Cropper keeps for its pictures


def _is_int(v) -> bool:
    if isinstance(v, (bool, np.bool_)):
        return False
    return isinstance(v, (int, np.integer)) or (isinstance(v, (float, np.floating)) and np.isfinite(v) and float(v) == int(v))


def check_background(background):
    """``background`` of the Cropper -> None (off), the fill (r, g, b): an int 0..255 (gray) or three of them, or
    ``TRANSPARENT`` for the string "transparent" (an RGBA cut-out in place of a fill)."""
    if background is None:
        return None
    if isinstance(background, str) and background == TRANSPARENT:
        return TRANSPARENT
    values = [background] * 3 if _is_int(background) else background
    if isinstance(values, (str, bytes)) or not hasattr(values, "__len__") or len(values) != 3 or not all(_is_int(v) for v in values):
        raise ValueError(f"background must be None, an int 0..255, three of them (R, G, B) or {TRANSPARENT!r}, not {background!r}")
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


def _check_sigma(option: str, sigma):
    if sigma is None:
        return None
    if isinstance(sigma, (bool, np.bool_)) or not isinstance(sigma, (int, float, np.integer, np.floating)) or \
            not np.isfinite(sigma) or not MIN_SIGMA <= sigma <= MAX_SIGMA:
        raise ValueError(f"{option} must be None or a finite sigma in [{MIN_SIGMA}, {MAX_SIGMA}] pixels, not {sigma!r}")
    return float(sigma)


def check_blur(sigma):
    """``background_blur`` of the Cropper -> None (off) or sigma in output pixels as a float: finite, 0.5..16."""
    return _check_sigma("background_blur", sigma)


def check_decontaminate(sigma):
    """``decontaminate`` of the Cropper -> None (off) or sigma in output pixels as a float: finite, 0.5..16, the range of
    ``background_blur`` (the taps are ``blur_taps``' too)."""
    return _check_sigma("decontaminate", sigma)


def check_refine(refine):
    """``refine`` of the Cropper -> None (off) or the window radius of the guided filter in output pixels, an int 1..16."""
    if refine is None:
        return None
    if not _is_int(refine) or not MIN_REFINE <= int(refine) <= MAX_REFINE:
        raise ValueError(f"refine must be None or an int {MIN_REFINE}..{MAX_REFINE} (a radius in pixels), not {refine!r}")
    return int(refine)


def check_refine_eps(refine_eps) -> int:
    """``refine_eps`` of the Cropper -> the regulariser of the guided filter in gray levels squared, an int 1..4096
    (None: 64, about 1e-3 of the [0, 1] range squared)."""
    if refine_eps is None:
        return DEFAULT_REFINE_EPS
    if not _is_int(refine_eps) or not MIN_REFINE_EPS <= int(refine_eps) <= MAX_REFINE_EPS:
        raise ValueError(f"refine_eps must be None or an int {MIN_REFINE_EPS}..{MAX_REFINE_EPS} (gray levels squared), "
                         f"not {refine_eps!r}")
    return int(refine_eps)


def check_subject(subject):
    """``subject`` of the Cropper -> None (off) or "largest"."""
    if subject is None:
        return None
    if not isinstance(subject, str) or subject not in SUBJECTS:
        raise ValueError(f"subject must be None or one of {SUBJECTS}, not {subject!r}")
    return subject


def check_fill_holes(fill_holes):
    """``fill_holes`` of the Cropper -> None (off) or the largest hole that is filled, in output pixels: an int
    1..67108864."""
    if fill_holes is None:
        return None
    if not _is_int(fill_holes) or not 1 <= int(fill_holes) <= MAX_FILL_HOLES:
        raise ValueError(f"fill_holes must be None or an int 1..{MAX_FILL_HOLES} (an area in pixels), not {fill_holes!r}")
    return int(fill_holes)


def check_edge_shift(edge_shift):
    """``edge_shift`` of the Cropper -> None (off) or the pixels the matte's boundary moves, a non-zero int -64..64:
    positive grows the subject, negative shrinks it."""
    if edge_shift is None:
        return None
    if not _is_int(edge_shift) or int(edge_shift) == 0 or not -MAX_EDGE_SHIFT <= int(edge_shift) <= MAX_EDGE_SHIFT:
        raise ValueError(f"edge_shift must be None or a non-zero int -{MAX_EDGE_SHIFT}..{MAX_EDGE_SHIFT} (pixels: positive grows "
                         f"the subject, negative shrinks it), not {edge_shift!r}")
    return int(edge_shift)


def check_fit(fit) -> str:
    """``background_fit`` of the Cropper -> "cover" or "stretch" (None: "cover")."""
    if fit is None:
        return DEFAULT_FIT
    if not isinstance(fit, str) or fit not in FITS:
        raise ValueError(f"background_fit must be None or one of {FITS}, not {fit!r}")
    return fit


def _picture_array(picture) -> np.ndarray:
    if picture.dtype != np.uint8 or picture.ndim != 3 or picture.shape[2] != 3 or min(picture.shape[:2]) < 1:
        raise ValueError(f"background_image arrays must be (H, W, 3) uint8 RGB with H, W >= 1, not {picture.dtype} {picture.shape}")
    return np.ascontiguousarray(picture)


def load_pictures(background_image) -> list:
    """``background_image`` of the Cropper -> its K >= 1 pictures, (H, W, 3) uint8 RGB arrays: a path to an image file, a
    path to a directory (every file in it that ``utils.read_image`` reads, in sorted name order), an array, or a list
    or tuple of those.  Files are decoded as the inputs of ``process_dir`` are."""
    from ._io_codec import read_image
    if isinstance(background_image, np.ndarray):
        return [_picture_array(background_image)]
    if isinstance(background_image, (str, os.PathLike)):
        path = os.fspath(background_image)
        if os.path.isdir(path):
            found = [read_image(os.path.join(path, name)) for name in sorted(os.listdir(path))]
            found = [p for p in found if p is not None]
            if not found:
                raise ValueError(f"background_image: the directory {path!r} holds no image that can be read")
            return found
        if not os.path.isfile(path):
            raise ValueError(f"background_image: no such file or directory: {path!r}")
        picture = read_image(path)
        if picture is None:
            raise ValueError(f"background_image: {path!r} cannot be read as an image")
        return [picture]
    if isinstance(background_image, (list, tuple)):
        if len(background_image) == 0:
            raise ValueError("background_image must name at least one picture, not an empty list")
        if any(isinstance(item, (list, tuple)) for item in background_image):
            raise ValueError("background_image: a list holds paths and (H, W, 3) uint8 arrays, not lists")
        return [picture for item in background_image for picture in load_pictures(item)]
    raise ValueError(f"background_image must be None, a path, an (H, W, 3) uint8 array or a list of those, not {background_image!r}")


def fit_picture(picture: np.ndarray, size, fit: str = DEFAULT_FIT) -> np.ndarray:
    """One picture (H, W, 3) uint8 -> (oh, ow, 3) uint8 for ``size`` = (ow, oh).  A picture of that size is taken as it
    is; otherwise Pillow's Lanczos resample of a box of it: the whole picture ("stretch"), or the centred box of the
    crop's aspect ratio, the largest the picture holds ("cover": a uniform scale, nothing of the crop left uncovered)."""
    ow, oh = size
    H, W = picture.shape[:2]
    if (W, H) == (ow, oh):
        return np.ascontiguousarray(picture)
    from PIL import Image
    box = (0, 0, W, H)
    if fit == "cover":
        s = max(ow / W, oh / H)
        bw, bh = ow / s, oh / s
        box = (max((W - bw) / 2, 0), max((H - bh) / 2, 0), min((W + bw) / 2, W), min((H + bh) / 2, H))
    return np.asarray(Image.fromarray(picture).resize((ow, oh), Image.Resampling.LANCZOS, box=box))


def picture_bank(background_image, size, fit: str = DEFAULT_FIT) -> np.ndarray:
    """``background_image`` -> the bank (K, oh, ow, 3) uint8 for ``size`` = (ow, oh), on the host: every picture of
    ``load_pictures`` through ``fit_picture``.  At most 4096 pictures and 1 GiB."""
    ow, oh = size
    pictures = load_pictures(background_image)
    nbytes = len(pictures) * oh * ow * 3
    if len(pictures) > MAX_PICTURES:
        raise ValueError(f"background_image: at most {MAX_PICTURES} pictures (got {len(pictures)})")
    if nbytes > MAX_BANK_BYTES:
        raise ValueError(f"background_image: the bank of {len(pictures)} pictures of {ow} x {oh} px needs {nbytes} bytes of "
                         f"device memory, more than {MAX_BANK_BYTES}")
    return np.stack([fit_picture(p, (ow, oh), fit) for p in pictures])


def pick_pictures(names, k: int) -> list:
    """The picture of each face of a bank of ``k``: crc32 of the stem (the base name without its extension, UTF-8) of the
    face's file, modulo k.  It depends on nothing but the name: not on the batch, its order or the other files."""
    return [zlib.crc32(os.path.splitext(os.path.basename(str(name)))[0].encode("utf-8")) % k for name in names]


def blur_taps(sigma) -> list:
    """sigma -> the integer taps t[0..r] of the background blur, in float64: r = min(48, max(3, ceil(3 sigma))),
    g_k = exp(-k^2 / (2 sigma^2)), s = g_0 + 2 sum g_k, t_k = max(1, floor(4096 g_k / s)) for k >= 1 and t_0 the rest of
    4096.  Every tap is >= 1, they do not grow with k, and the window sums to 4096: the kernel's 32-bit bounds."""
    sigma = check_blur(sigma)
    if sigma is None:
        raise ValueError("blur_taps needs a sigma")
    r = min(MAX_RADIUS, max(MIN_RADIUS, math.ceil(3 * sigma)))
    g = [math.exp(-k * k / (2 * sigma * sigma)) for k in range(r + 1)]
    s = g[0] + 2 * sum(g[1:])
    t = [0] + [max(1, math.floor(TAP_SUM * g[k] / s)) for k in range(1, r + 1)]
    t[0] = TAP_SUM - 2 * sum(t[1:])
    assert all(t[k] >= t[k + 1] for k in range(r)) and t[r] >= 1, t
    return t


def _check_crops(crops_dev, labels_dev=None):
    """crops (F,H,W,3) u8, contiguous, and with them the label maps (F,H,W) u8."""
    assert crops_dev.dtype == torch.uint8 and crops_dev.is_contiguous() and crops_dev.dim() == 4 and crops_dev.shape[3] == 3
    if labels_dev is not None:
        assert labels_dev.dtype == torch.uint8 and labels_dev.is_contiguous() and tuple(labels_dev.shape) == tuple(crops_dev.shape[:3])


def _check_alpha(alpha, crops_dev):
    assert alpha.dtype == torch.uint8 and alpha.is_contiguous() and tuple(alpha.shape) == tuple(crops_dev.shape[:3])
    assert alpha.device == crops_dev.device


def _check_taps(entry: str, taps, allow_empty: bool = False):
    """The ctypes boundary's share of the taps check (the torch ops have their own): the count and 16 bits each."""
    if allow_empty and not taps:
        return
    if not MIN_RADIUS + 1 <= len(taps) <= MAX_RADIUS + 1 or min(taps) < 0 or max(taps) > 65535:
        raise RuntimeError(f"{entry}: taps must be {'empty or ' if allow_empty else ''}t[0..radius] with radius "
                           f"{MIN_RADIUS}..{MAX_RADIUS}, each 16 bits (got {len(taps)} taps)")


def refine_alpha(crops_dev: torch.Tensor, labels_dev: torch.Tensor, class_bits: int, radius: int, eps: int) -> torch.Tensor:
    """crops (F,H,W,3) u8 and labels (F,H,W) u8, device -> alpha (F,H,W) u8, device: the hard mask of the labels filtered by
    a guided filter of window radius ``radius`` (1..16) and regulariser ``eps`` (1..4096) with the gray of the crop as the
    guide, in integers.  Two launches and a workspace of 8 bytes per pixel that lives for the
    call; H, W <= 8192."""
    _check_crops(crops_dev, labels_dev)
    if T.ENABLED:
        return T.load().matte_refine(crops_dev, labels_dev, int(class_bits), int(radius), int(eps))
    f, h, w, _ = crops_dev.shape
    alpha = torch.empty((f, h, w), dtype=torch.uint8, device=crops_dev.device)
    need = max(int(N.lib().fcp_matte_refine_workspace_bytes(f, h, w)), 0)
    work = torch.empty((need,), dtype=torch.uint8, device=crops_dev.device)
    N.check(N.lib().fcp_matte_refine_u8(N.ptr(crops_dev), N.ptr(labels_dev), f, h, w, int(class_bits), int(radius), int(eps),
                                        N.ptr(alpha), N.ptr(work), need, N.stream_ptr()), "fcp_matte_refine_u8")
    return alpha


def subject_mask(labels_dev: torch.Tensor, class_bits: int, keep_largest: bool, max_hole: int) -> torch.Tensor:
    """labels (F,H,W) u8, device -> out (F,H,W) u8 of 0 / 1, device: the hard mask of the labels, reduced to its largest
    8-connected component where ``keep_largest``, then with its holes of at most ``max_hole`` pixels (0: none) filled, in
    integers.  One launch for (False, 0), five for the subject, four for the holes, and a
    workspace of 12 bytes per pixel that lives for the call; H, W <= 8192."""
    assert labels_dev.dtype == torch.uint8 and labels_dev.is_contiguous() and labels_dev.dim() == 3
    if T.ENABLED:
        return T.load().subject_mask(labels_dev, int(class_bits), bool(keep_largest), int(max_hole))
    f, h, w = labels_dev.shape
    out = torch.empty_like(labels_dev)
    need = max(int(N.lib().fcp_subject_mask_workspace_bytes(f, h, w)), 0)
    work = torch.empty((need,), dtype=torch.uint8, device=labels_dev.device)
    N.check(N.lib().fcp_subject_mask_u8(N.ptr(labels_dev), f, h, w, int(class_bits), int(bool(keep_largest)), int(max_hole),
                                        N.ptr(out), N.ptr(work), need, N.stream_ptr()), "fcp_subject_mask_u8")
    return out


def shift_mask(labels_dev: torch.Tensor, class_bits: int, shift: int) -> torch.Tensor:
    """labels (F,H,W) u8, device -> out (F,H,W) u8 of 0 / 1, device: the hard mask of the labels grown (``shift`` > 0) or
    shrunk (``shift`` < 0) by a Euclidean disc of radius |shift| <= 64 inside the crop, in integers (INTEGRATION.md section
    2o); 0 gives the hard mask itself.  One launch, no workspace; H, W <= 8192."""
    assert labels_dev.dtype == torch.uint8 and labels_dev.is_contiguous() and labels_dev.dim() == 3
    if T.ENABLED:
        return T.load().mask_shift(labels_dev, int(class_bits), int(shift))
    f, h, w = labels_dev.shape
    out = torch.empty_like(labels_dev)
    N.check(N.lib().fcp_mask_shift_u8(N.ptr(labels_dev), f, h, w, int(class_bits), int(shift), N.ptr(out), N.stream_ptr()),
            "fcp_mask_shift_u8")
    return out


def feather_alpha(labels_dev: torch.Tensor, class_bits: int, feather: int) -> torch.Tensor:
    """labels (F,H,W) u8, device -> alpha (F,H,W) u8, device: the feathered mask ``matte`` composites through, alone.  One
    launch; H, W <= 8192."""
    assert labels_dev.dtype == torch.uint8 and labels_dev.is_contiguous() and labels_dev.dim() == 3
    if T.ENABLED:
        return T.load().feather_alpha(labels_dev, int(class_bits), int(feather))
    f, h, w = labels_dev.shape
    alpha = torch.empty_like(labels_dev)
    N.check(N.lib().fcp_feather_alpha_u8(N.ptr(labels_dev), f, h, w, int(class_bits), int(feather), N.ptr(alpha), N.stream_ptr()),
            "fcp_feather_alpha_u8")
    return alpha


def cutout(crops_dev: torch.Tensor, alpha: torch.Tensor, fill=None, taps=None) -> torch.Tensor:
    """crops (F,H,W,3) u8 and an alpha plane (F,H,W) u8 (``feather_alpha``'s or ``refine_alpha``'s), device ->
    ``fill`` None: the RGBA cut-out (F,H,W,4) u8, ``(colour, alpha)`` where alpha > 0 and zeros where it is 0;
    ``fill`` (r, g, b): the composite (F,H,W,3) u8 of the colour over that fill.  The colour is the crop's without
    ``taps`` (RGBA only: over a fill that is ``matte``), else the subject's colour estimated with the taps t[0..r] of
    ``blur_taps``: its weights are the pixels whose alpha is exactly 255 (subject) and exactly 0 (background), and where
    the window holds neither kind the crop's colour stands.  One launch without taps; two and a workspace of 32 bytes per
    pixel that lives for the call with them; H, W <= 8192."""
    _check_crops(crops_dev)
    _check_alpha(alpha, crops_dev)
    mode = CUTOUT_RGBA if fill is None else CUTOUT_FILL
    r, g, b = (0, 0, 0) if fill is None else (int(v) for v in fill)
    taps = [] if taps is None else [int(t) for t in taps]
    if T.ENABLED:
        return T.load().cutout(crops_dev, alpha, mode, r, g, b, taps)
    _check_taps("fcp_cutout_u8", taps, allow_empty=True)
    f, h, w, _ = crops_dev.shape
    out = torch.empty((f, h, w, 4 if fill is None else 3), dtype=torch.uint8, device=crops_dev.device)
    need = max(int(N.lib().fcp_cutout_workspace_bytes(f, h, w)), 0) if taps else 0
    work = torch.empty((need,), dtype=torch.uint8, device=crops_dev.device)
    t16 = (ctypes.c_uint16 * max(len(taps), 1))(*taps)
    N.check(N.lib().fcp_cutout_u8(N.ptr(crops_dev), N.ptr(alpha), f, h, w, mode, r, g, b, t16, max(len(taps) - 1, 0), N.ptr(out),
                                  N.ptr(work), need, N.stream_ptr()), "fcp_cutout_u8")
    return out


def matte_blur(crops_dev: torch.Tensor, labels_dev: torch.Tensor, class_bits: int, feather: int, taps, with_alpha: bool = False,
               alpha: torch.Tensor | None = None):
    """crops (F,H,W,3) u8 and labels (F,H,W) u8, device -> (out (F,H,W,3) u8, alpha (F,H,W) u8 or None), device: the
    crops over their own mask-normalised background blur with the taps t[0..r] of ``blur_taps``.  Two launches and a
    workspace of 16 bytes per pixel that lives for the call; H, W <= 8192.  With ``alpha`` (F,H,W) u8 (``refine_alpha``'s)
    the composite goes through that plane instead of the feathered mask: ``feather`` is not used, and the plane itself
    comes back where ``with_alpha`` asks for one."""
    _check_crops(crops_dev, labels_dev)
    taps = [int(t) for t in taps]
    if alpha is not None:
        _check_alpha(alpha, crops_dev)
        if T.ENABLED:
            out = T.load().matte_blur_alpha(crops_dev, labels_dev, alpha, int(class_bits), taps)
            return out, (alpha if with_alpha else None)
    elif T.ENABLED:
        out, alpha = T.load().matte_blur(crops_dev, labels_dev, int(class_bits), int(feather), taps, bool(with_alpha))
        return out, (alpha if with_alpha else None)
    _check_taps("fcp_matte_blur_u8", taps)
    f, h, w, _ = crops_dev.shape
    out = torch.empty_like(crops_dev)
    need = max(int(N.lib().fcp_matte_blur_workspace_bytes(f, h, w)), 0)
    work = torch.empty((need,), dtype=torch.uint8, device=crops_dev.device)
    t16 = (ctypes.c_uint16 * len(taps))(*taps)
    if alpha is not None:
        N.check(N.lib().fcp_matte_blur_alpha_u8(N.ptr(crops_dev), N.ptr(labels_dev), N.ptr(alpha), f, h, w, int(class_bits), t16,
                                                len(taps) - 1, N.ptr(out), N.ptr(work), need, N.stream_ptr()),
                "fcp_matte_blur_alpha_u8")
        return out, (alpha if with_alpha else None)
    alpha = torch.empty((f, h, w), dtype=torch.uint8, device=crops_dev.device) if with_alpha else None
    N.check(N.lib().fcp_matte_blur_u8(N.ptr(crops_dev), N.ptr(labels_dev), f, h, w, int(class_bits), int(feather), t16,
                                      len(taps) - 1, N.ptr(out), N.ptr(alpha), N.ptr(work), need, N.stream_ptr()),
            "fcp_matte_blur_u8")
    return out, alpha


def matte(crops_dev: torch.Tensor, labels_dev: torch.Tensor, class_bits: int, feather: int, fill, with_alpha: bool = False,
          alpha: torch.Tensor | None = None):
    """crops (F,H,W,3) u8 and labels (F,H,W) u8, device -> (out (F,H,W,3) u8, alpha (F,H,W) u8 or None), device.  One
    launch; H, W <= 8192.  With ``alpha`` (F,H,W) u8 (``refine_alpha``'s) the composite goes through that plane: the
    labels, ``class_bits`` and ``feather`` are not used, and the plane itself comes back where ``with_alpha`` asks for one."""
    _check_crops(crops_dev, labels_dev)
    r, g, b = (int(v) for v in fill)
    if alpha is not None:
        _check_alpha(alpha, crops_dev)
        if T.ENABLED:
            out = T.load().matte_alpha(crops_dev, alpha, r, g, b)
        else:
            f, h, w, _ = crops_dev.shape
            out = torch.empty_like(crops_dev)
            N.check(N.lib().fcp_matte_alpha_u8(N.ptr(crops_dev), N.ptr(alpha), f, h, w, r, g, b, N.ptr(out), N.stream_ptr()),
                    "fcp_matte_alpha_u8")
        return out, (alpha if with_alpha else None)
    if T.ENABLED:
        out, alpha = T.load().matte(crops_dev, labels_dev, int(class_bits), int(feather), r, g, b, bool(with_alpha))
        return out, (alpha if with_alpha else None)
    f, h, w, _ = crops_dev.shape
    out = torch.empty_like(crops_dev)
    alpha = torch.empty((f, h, w), dtype=torch.uint8, device=crops_dev.device) if with_alpha else None
    N.check(N.lib().fcp_matte_u8(N.ptr(crops_dev), N.ptr(labels_dev), f, h, w, int(class_bits), int(feather), r, g, b,
                                 N.ptr(out), N.ptr(alpha), N.stream_ptr()), "fcp_matte_u8")
    return out, alpha


def _check_bank(pictures_dev, picks, crops_dev) -> torch.Tensor:
    """The bank (K,H,W,3) u8, contiguous, on the crops' device and of the crops' H and W, and the picks, F ints 0..K-1 on
    the host -> the picks (F,) int32 on the device."""
    f, h, w, _ = crops_dev.shape
    if not isinstance(pictures_dev, torch.Tensor) or pictures_dev.dtype != torch.uint8 or not pictures_dev.is_contiguous() or \
            pictures_dev.dim() != 4 or pictures_dev.shape[0] < 1 or tuple(pictures_dev.shape[1:]) != (h, w, 3) or \
            pictures_dev.device != crops_dev.device:
        raise ValueError(f"pictures must be a contiguous (K,{h},{w},3) uint8 tensor on {crops_dev.device}, K >= 1, not "
                         f"{getattr(pictures_dev, 'dtype', type(pictures_dev))} {tuple(getattr(pictures_dev, 'shape', ()))} on "
                         f"{getattr(pictures_dev, 'device', 'the host')}")
    k = pictures_dev.shape[0]
    picks = list(picks)
    if len(picks) != f or not all(_is_int(p) and 0 <= int(p) < k for p in picks):
        raise ValueError(f"picks must be {f} ints 0..{k - 1}, one per crop, not {picks!r}")
    return torch.tensor([int(p) for p in picks], dtype=torch.int32).to(crops_dev.device)


def cutout_image(crops_dev: torch.Tensor, alpha: torch.Tensor, pictures_dev: torch.Tensor, picks, taps) -> torch.Tensor:
    """``cutout`` with a fill, over pictures: crops (F,H,W,3) u8, an alpha plane (F,H,W) u8, a bank (K,H,W,3) u8, all on one
    device, and F picks 0..K-1 on the host -> the composite (F,H,W,3) u8 of the subject's colour, estimated with the taps
    t[0..r] of ``blur_taps``, over picture ``picks[i]`` for crop i.  Without an estimate that is ``matte_image`` with the
    plane.  Two launches and a workspace of 32 bytes per pixel that lives for the call; H, W <= 8192."""
    _check_crops(crops_dev)
    _check_alpha(alpha, crops_dev)
    picks_dev = _check_bank(pictures_dev, picks, crops_dev)
    taps = [int(t) for t in taps]
    if T.ENABLED:
        return T.load().cutout_image(crops_dev, alpha, pictures_dev, picks_dev, taps)
    _check_taps("fcp_cutout_image_u8", taps)
    f, h, w, _ = crops_dev.shape
    out = torch.empty_like(crops_dev)
    need = max(int(N.lib().fcp_cutout_workspace_bytes(f, h, w)), 0)
    work = torch.empty((need,), dtype=torch.uint8, device=crops_dev.device)
    t16 = (ctypes.c_uint16 * len(taps))(*taps)
    N.check(N.lib().fcp_cutout_image_u8(N.ptr(crops_dev), N.ptr(alpha), f, h, w, N.ptr(pictures_dev), pictures_dev.shape[0],
                                        N.ptr(picks_dev), t16, len(taps) - 1, N.ptr(out), N.ptr(work), need, N.stream_ptr()),
            "fcp_cutout_image_u8")
    return out


def matte_image(crops_dev: torch.Tensor, labels_dev: torch.Tensor, class_bits: int, feather: int, pictures_dev: torch.Tensor, picks,
                with_alpha: bool = False, alpha: torch.Tensor | None = None):
    """``matte`` over pictures: crops (F,H,W,3) u8, labels (F,H,W) u8 and a bank (K,H,W,3) u8, all on one device, and F
    picks 0..K-1 on the host -> (out (F,H,W,3) u8, alpha (F,H,W) u8 or None), device: crop i over picture ``picks[i]``.
    One launch; H, W <= 8192.  With ``alpha`` (F,H,W) u8 the composite goes through that plane, as in ``matte``."""
    _check_crops(crops_dev, labels_dev)
    picks_dev = _check_bank(pictures_dev, picks, crops_dev)
    k = pictures_dev.shape[0]
    if alpha is not None:
        _check_alpha(alpha, crops_dev)
        if T.ENABLED:
            out = T.load().matte_image_alpha(crops_dev, alpha, pictures_dev, picks_dev)
        else:
            f, h, w, _ = crops_dev.shape
            out = torch.empty_like(crops_dev)
            N.check(N.lib().fcp_matte_image_alpha_u8(N.ptr(crops_dev), N.ptr(alpha), f, h, w, N.ptr(pictures_dev), k, N.ptr(picks_dev),
                                                     N.ptr(out), N.stream_ptr()), "fcp_matte_image_alpha_u8")
        return out, (alpha if with_alpha else None)
    if T.ENABLED:
        out, alpha = T.load().matte_image(crops_dev, labels_dev, int(class_bits), int(feather), pictures_dev, picks_dev,
                                          bool(with_alpha))
        return out, (alpha if with_alpha else None)
    f, h, w, _ = crops_dev.shape
    out = torch.empty_like(crops_dev)
    alpha = torch.empty((f, h, w), dtype=torch.uint8, device=crops_dev.device) if with_alpha else None
    N.check(N.lib().fcp_matte_image_u8(N.ptr(crops_dev), N.ptr(labels_dev), f, h, w, int(class_bits), int(feather),
                                       N.ptr(pictures_dev), k, N.ptr(picks_dev), N.ptr(out), N.ptr(alpha), N.stream_ptr()),
            "fcp_matte_image_u8")
    return out, alpha
