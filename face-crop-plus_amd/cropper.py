"""``Cropper`` — same constructor, attributes and ``process_dir`` / ``process_batch`` /
``crop_align`` surface as the reference (cropper.py:139-156, :441-447, :748, :852-857),
with the batch kept resident on the GPU from the upload to the final crops:
detect -> [enhance] -> estimate + warp -> [parse] run as HIP kernels; the host sees
only the uint8 crops / masks it has to write to disk.
"""
from __future__ import annotations

import itertools
import os
from collections import Counter, defaultdict
from multiprocessing.pool import ThreadPool
from threading import BoundedSemaphore, Lock, local

import numpy as np
import torch

from . import align, trace
from . import clahe as equalizing
from . import denoise as denoising
from . import matte as matting
from . import sharpen as sharpening
from . import skin as smoothing
from ._io_codec import _ENCODER_KW, JpegSettings, check_jpeg_settings, write_bytes
from .batch import batch_geometry, build_batch, upload_sources
from .utils import get_ldm_slices, parse_landmarks_file, read_image, read_images, write_image


def landmarks_target(output_size, face_factor):
    """Target 5-point set (cropper.py:423-439): float32 table scaled in place."""
    std = align.STANDARD_LANDMARKS_5.copy()
    std[:, 0] *= output_size[0] * face_factor
    std[:, 1] *= output_size[1] * face_factor
    std[:, 0] += (1 - face_factor) * output_size[0] / 2
    std[:, 1] += (1 - face_factor) * output_size[1] / 2
    return std


def _pair(v):
    """An int, a numpy integer or a sequence of one or two of them -> the (width, height) pair."""
    v = (v,) if isinstance(v, (int, np.integer)) else tuple(v)
    return v * 2 if len(v) == 1 else v


def _u8_crops(crops, channels=(3,), gray=False):
    """The checked, contiguous form of a crop array the public per-step helpers take: uint8, (F,H,W,C) with C one of
    ``channels``, or (F,H,W) where ``gray`` allows it."""
    crops = np.ascontiguousarray(crops)
    if crops.dtype != np.uint8 or not ((crops.ndim == 4 and crops.shape[3] in channels) or (gray and crops.ndim == 3)):
        shapes = [f"(F,H,W,{c})" for c in channels] + ["(F,H,W)"] * gray
        shapes = ", ".join(shapes[:-1]) + " or " * (len(shapes) > 1) + shapes[-1]         # "a, b or c"
        raise ValueError(f"crops must be {shapes} uint8, not {crops.dtype} {crops.shape}")
    return crops


class Cropper:
    # Every optional setting and every lazily created piece of state, at its "off" value: a Cropper made with __new__
    # (the CPU tests make them) or unpickled from an older build reads whatever __init__ never set on it as switched off.
    background = background_blur = background_image = background_fit = blur_taps = decontaminate = decontaminate_taps = None
    refine = refine_eps = subject = fill_holes = edge_shift = denoise = clahe = clahe_grid = None
    sharpen = sharpen_sigma = sharpen_threshold = min_sharpness = jpeg = io_ring_mb = None
    smooth_skin = smooth_sigma = smooth_amount = skin_classes = None
    _io = _io_procs = _io_procs_active = _rows_cache = _pictures_dev = None
    png_encoder = encoder = "host"
    foreground_bits = skin_bits = 0

    def __init__(
        self,
        output_size: int | tuple[int, int] | list[int] = 256,
        output_format: str | None = None,
        resize_size: int | tuple[int, int] | list[int] = 1024,
        face_factor: float = 0.65,
        strategy: str = "largest",
        padding: str = "constant",
        allow_skew: bool = False,
        landmarks: str | tuple[np.ndarray, np.ndarray] | None = None,
        attr_groups: dict[str, list[int]] | None = None,
        mask_groups: dict[str, list[int]] | None = None,
        det_threshold: float | None = 0.6,
        enh_threshold: float | None = None,
        batch_size: int = 8,
        num_processes: int = 1,
        device: str | torch.device = "cuda:0",
        weights: dict | None = None,
        precision: str | None = None,
        warp_family: str | None = None,
        crop_source: str = "batch",
        encoder: str = "host",
        png_encoder: str = "host",
        jpeg_quality: int = 95,
        jpeg_subsampling: str = "4:2:0",
        jpeg_optimize: bool = False,
        background: int | tuple[int, int, int] | list[int] | str | None = None,
        foreground: list[int] | None = None,
        feather: int | None = None,
        background_blur: float | None = None,
        background_image: str | np.ndarray | list | tuple | None = None,
        background_fit: str | None = None,
        refine: int | None = None,
        refine_eps: int | None = None,
        subject: str | None = None,
        fill_holes: int | None = None,
        smooth_skin: float | None = None,
        smooth_sigma: float | None = None,
        smooth_amount: float | None = None,
        skin_classes: list[int] | None = None,
        decontaminate: float | None = None,
        edge_shift: int | None = None,
        denoise: float | None = None,
        clahe: float | None = None,
        clahe_grid: int | None = None,
        sharpen: float | None = None,
        sharpen_sigma: float | None = None,
        sharpen_threshold: int | None = None,
        interpolation: str = "linear",
        min_sharpness: float | None = None,
    ):
        """Arguments as in the reference (cropper.py:139-156).  ``device`` must be a GPU
        (``"cuda:N"``); ``weights`` optionally maps "retinaface"/"rrdb"/"bisenet" to a
        state dict / path / "generated" (default: the real checkpoints, from ``$FCP_WEIGHTS_DIR`` or the
        torch hub cache, else downloaded like the reference does; there is no silent random-weight fallback).
        ``warp_family``: which cv2.warpAffine algorithm the crops reproduce byte for byte — "fixed" (OpenCV's classic
        fixed-point warp), "float32" (the float warp of newer OpenCV builds) or "auto" (whichever the installed cv2 runs,
        "fixed" without cv2); None = ``$FCP_WARP_FAMILY``, else "fixed" (``align.resolve_warp_family``).
        ``crop_source``: "batch" samples every crop from the resized batch image, as the reference does; "original" samples
        it from the decoded file, through a power-of-two INTER_AREA level of it when the crop minifies the file by 2 or more
        (``align.crop_align_sources``).  "original" cannot be combined with ``enh_threshold``: the enhancer works on the
        resized batch, which this mode does not sample.
        ``interpolation``: the filter of the crop warp — "linear" (cv2.INTER_LINEAR, the reference's), "cubic"
        (INTER_CUBIC) or "lanczos4" (INTER_LANCZOS4), OpenCV's fixed-point warps, on every crop path.  Cubic and Lanczos-4
        have no float32 family: combining them with an explicit ``warp_family="float32"`` (or ``$FCP_WARP_FAMILY``)
        raises ValueError.
        ``min_sharpness``: drop blurry crops — a face is kept when the variance of the Laplacian of its crop,
        ``cv2.Laplacian(cv2.cvtColor(crop, cv2.COLOR_RGB2GRAY), cv2.CV_64F).var()`` computed exactly on the device
        (``align.sharpness_sums`` / ``sharpness_score``), is at least this value; dropped faces are neither parsed nor
        written.  None (the default) scores nothing.  It needs aligned crops, so it cannot be combined with "no alignment"
        (``det_threshold=None`` and ``landmarks=None``); useful values depend on ``output_size`` and the content:
        calibrate with ``Cropper.sharpness``.
        ``encoder``: "host" (the default) compresses every output file with Pillow on the I/O pool; "device" compresses
        the JPEG files (.jpg / .jpeg / .jpe) of aligned crops and parse masks on the GPU (``jpegenc.encode_jpeg``) — the
        same files byte for byte — so that the lengths and the compressed streams come back instead of the pixels and the
        I/O pool only writes.  Every other file (other formats, the images of "no alignment", a crop whose stream
        outgrows its slot) is encoded on the host as before.
        ``png_encoder``: the same choice for the PNG files (.png) of aligned crops and parse masks, independent of
        ``encoder``: "device" filters and deflates them on the GPU (``pngenc.encode_png``), so
        that the lengths and the zlib streams come back instead of the pixels.  The files decode to exactly the pixels
        the host's files decode to, but they are NOT the host's bytes (a deflate stream has many valid encodings; this one
        is mostly smaller than zlib's level 1, which the host writes).  The images of "no alignment", a face whose
        stream outgrows its slot and faces larger than the kernels take keep the host encoder.  "host" (the default)
        changes nothing.  ``Cropper.encode_png`` applies it to crops one already has.
        ``background``: replace what is behind the subject — an int 0..255 (gray) or three of them (R, G, B) fills every
        pixel the face parser does not label as one of the ``foreground`` classes (BiSeNet indices; None: every class but
        0), through a soft edge of ``feather`` pixels (0, 3, 5 or 7; None: 5): the Gaussian of that size over the hard
        mask, OpenCV's fixed-point ``cv2.GaussianBlur(mask, (feather, feather), 0)`` restated, then
        ``(crop * alpha + fill * (255 - alpha) + 127) // 255`` (``matte.matte``).  It runs on
        the device after ``min_sharpness`` and the parse, which both see the original crop, and before anything is
        encoded; the mask files of ``mask_groups`` are unchanged.  A face without a foreground pixel becomes a uniformly
        filled image and is still written (``attr_groups`` is the way to drop such faces).  It creates the parser even
        without ``attr_groups`` / ``mask_groups``, needs aligned crops like ``min_sharpness``, and ``foreground`` /
        ``feather`` without ``background`` raise ValueError.  None (the default) launches nothing.
        ``Cropper.matte`` applies it to crops and label maps one already has.
        ``background_blur``: keep what is behind the subject and blur it — the sigma, in output pixels (0.5..16), of a
        Gaussian over the background pixels alone, divided by the Gaussian weight of the background pixels it saw, so
        that the subject's colours never leak into the background (a plain blur of the crop would show them as a halo
        through the soft edge); the subject, ``foreground`` and ``feather`` are those of ``background`` and the
        composite is the same, with the blurred background as the fill of every pixel (``matte.matte_blur``,
        INTEGRATION.md section 2i).  It sits where ``background`` sits, cannot be combined with it (ValueError), creates
        the parser and needs aligned crops like it; a face without a background pixel is written unchanged.  None (the
        default) launches nothing.
        ``background_image``: put the subject in front of a picture — a path to an image file, a path to a directory
        (every file in it that the input decoder reads, in sorted name order), an (H, W, 3) uint8 RGB array, or a list or
        tuple of paths and arrays: K >= 1 pictures.  The fill of every pixel is the byte of the face's picture at the
        pixel's own position; the subject, ``foreground``, ``feather`` and the composite are those of ``background``
        (``matte.matte_image``), so a picture of one colour gives exactly the files of that
        ``background``, and ``refine``, ``subject``, ``fill_holes``, ``edge_shift`` and ``decontaminate`` apply as they
        do with a fill.  The pictures are fitted to ``output_size`` once, at construction, on the host with Pillow's
        Lanczos filter — ``background_fit="cover"`` (None: that) scales uniformly until the picture covers the crop and
        crops its centre, ``"stretch"`` scales both axes on their own, and a picture that has the output size already
        is taken byte for byte — and stay on the device as one bank (at most 4096 pictures and 1 GiB).  With K > 1 a
        face gets picture ``crc32(stem) % K`` of the name its file has in the output directory
        (``matte.pick_pictures``): the same picture whatever the batch size, the workers or the other files, which makes
        background randomisation over a bank repeatable.  It sits where ``background`` sits, cannot be combined with it
        or with ``background_blur`` (ValueError), creates the parser and needs aligned crops like them;
        ``background_fit`` without it raises ValueError.  None (the default) launches nothing.  ``Cropper.matte(crops,
        labels, picks)`` applies it to crops one already has.
        ``refine``: follow the image's edges with the matte — the window radius, in output pixels (an int 1..16), of a
        guided filter (He, Sun, Tang) of the parser's hard mask with the gray of the crop as the guide: the alpha stays
        the parser's over flat regions and snaps to the crop's own edges along hair, ears and shoulders, where the label
        map is a few pixels off and staircase-shaped.  ``refine_eps`` (an int 1..4096, in gray levels squared; None: 64)
        is the filter's regulariser: below it a variation of the guide counts as flat.  It is stated in integers and held
        byte for byte to a numpy reference (``matte.refine_alpha``).  It needs ``background``
        or ``background_blur`` and replaces the Gaussian feather as their soft edge: an explicit ``feather`` beside it
        raises ValueError and ``Cropper.feather`` is 0; ``refine_eps`` without ``refine`` raises ValueError.  Everything
        else about the two modes is unchanged: the guide is the crop the composite uses (after ``clahe``), the blurred
        background still comes from the hard mask, mask files are untouched.  None (the default) launches nothing.
        ``subject`` / ``fill_holes``: keep one connected subject, whole — two repairs of the parser's hard mask before
        either background mode (and ``refine``) sees it.  ``subject="largest"`` keeps the largest 8-connected component
        of the foreground (among equal areas the one whose first pixel comes first in raster order), so that the
        neighbours' heads and shoulders and the parser's specks become background; ``fill_holes=N`` (an int
        1..67108864, in output pixels) then turns every 4-connected background region of at most N pixels that does not
        touch the crop's border into foreground, so that the fill or the blur no longer shows through highlights on
        glasses or between strands of hair.  The subject comes first: an island inside a hole counts in its area.  Both
        are connected-component labelling on the device, in integers, held byte for byte to a numpy reference
        (``matte.subject_mask``); the cleaned 0 / 1 map takes the label map's place for the
        feather, the guided filter, the composite and the blur's background sums.  They need ``background`` or
        ``background_blur`` (ValueError); mask files are untouched and a face without a foreground pixel behaves as
        before.  None (the default) launches nothing.
        ``edge_shift``: grow or shrink the matte — the pixels (a non-zero int -64..64) by which the boundary of the hard
        mask moves before any soft edge is made: negative shrinks the subject, positive grows it.  The parser's label
        map is computed at its own resolution and resampled, so along hair, ears and shoulders it sits a pixel or two
        outside the subject; that ring of old background has alpha 255, ``feather``, ``refine`` and ``decontaminate``
        all keep it, and it shows as a thin halo on every new background: ``edge_shift=-2`` removes it.  A positive
        value hands ``refine`` a mask that is a few pixels generous, for wisps of hair and the rims of glasses the
        parser cuts off, and lets the image's own edges pull it back.  It is binary morphology with a Euclidean disc
        of that radius, on the device, in integers, held byte for byte to a numpy reference (``matte.shift_mask``,
        INTEGRATION.md section 2o), and it runs after ``subject`` / ``fill_holes`` and before ``refine``, the feather,
        the composite and the blur's background sums.  Only positions inside the crop count: a shrink does not eat
        inwards from the crop's border, so shoulders that touch the bottom row stay there.  It needs ``background`` or
        ``background_blur`` (ValueError); mask files are untouched, and a face whose subject a shrink erases behaves as
        a face without a foreground pixel does.  None (the default) launches nothing.
        ``background="transparent"``: write RGBA cut-outs — no fill at all: every crop becomes ``(colour, alpha)`` with the
        matte as its alpha channel and ``(0, 0, 0, 0)`` wherever the alpha is 0, so that nothing of the old background ships
        in the file (``matte.cutout``).  It is a background mode like the fill: it creates the
        parser, needs aligned crops, ``foreground`` / ``feather`` / ``refine`` / ``subject`` / ``fill_holes`` apply, it
        excludes ``background_blur`` and mask files are unchanged.  Only PNG keeps an alpha channel among the formats
        written here, so it requires ``output_format="png"`` (any letter case; ValueError otherwise, at construction);
        the files are colour type 6, through either ``png_encoder``.
        ``decontaminate``: give the soft edge the subject's own colour — the sigma, in output pixels (0.5..16), of the
        "blur fusion" estimate.  In the soft edge the crop's colour is already ``alpha F + (1 - alpha) B_old``: shipping it
        beside the alpha, or compositing it over a new fill, carries the old background along as a halo.  The estimate is
        two mask-normalised Gaussians of that sigma, one over the pixels whose alpha is exactly 255 (certainly subject)
        and one over those whose alpha is exactly 0 (certainly background), and one integer correction that makes
        ``alpha F + (1 - alpha) B`` meet the crop again; where the window holds no pixel of a kind the crop's colour
        stands in for it.  Pixels with alpha 255 keep the crop's colour.  A useful sigma is about the width of the soft
        edge or more: below it the windows do not reach the certain pixels on both sides.  It works with
        ``background="transparent"`` and with a fill ``background=(R, G, B)`` (``matte.cutout``); with
        ``background_blur`` or without a background it raises ValueError.  None (the default) launches nothing new: a
        fill composites the crop's colour, byte for byte as before.
        ``denoise``: remove sensor noise from every crop — the filter strength H, in gray levels (a finite number 1..32; 8
        suits the grain of a small face enlarged from a high-ISO photo), of a non-local-means filter: every pixel becomes
        the weighted mean of the 21 x 21 pixels around it, each weighted by ``exp(-d / (49 H^2))`` of the squared
        difference d of the 7 x 7 gray patches around the two (the window sizes are the defaults of
        ``cv2.fastNlMeansDenoising``), stated in integers and held byte for byte to a numpy reference
        (``denoise.denoise``).  The weights come from the gray alone and the three channels
        are averaged with them: pure chroma noise is reduced less than luma noise.  It runs after ``min_sharpness`` and
        the parse, which both see the original crop (calibrated thresholds, label maps, attribute groups and mask files
        are the same with and without it), and immediately before ``clahe``, so that everything after it (``clahe``, the
        guide of ``refine``, both background modes, both encoders) sees the denoised crop.  It needs aligned crops like
        ``min_sharpness`` and an ``output_size`` of at least 14 x 14.  None (the default) launches nothing.
        ``Cropper.remove_noise`` applies it to crops one already has.
        ``clahe``: equalise the contrast of every crop — the clip limit (finite, > 0; 2.0 is the usual value) of a
        contrast-limited adaptive histogram equalisation of the luma on a ``clahe_grid`` x ``clahe_grid`` tiling (1..16;
        None: 8), ``cv2.createCLAHE(clahe, (grid, grid)).apply(Y)`` between ``cv2.cvtColor(crop, COLOR_RGB2YCrCb)`` and
        ``COLOR_YCrCb2RGB`` restated on the device (``clahe.clahe``).  It runs after
        ``min_sharpness`` and the parse, which both see the original crop, and before ``background`` (the fill colour
        stays exact) and the encoder; the histograms are over the whole crop and mask files are unchanged.  It needs
        aligned crops like ``min_sharpness`` and an ``output_size`` of at least ``2 * clahe_grid`` on both sides;
        ``clahe_grid`` without ``clahe`` raises ValueError.  None (the default) launches nothing.
        ``Cropper.equalize`` applies it to crops one already has.
        ``sharpen``: sharpen every crop — the amount A (a finite number 0.05..4; 1.0 adds the whole difference) of an
        unsharp mask of the gray: the gray's difference from its own Gaussian blur of ``sharpen_sigma`` output pixels
        (0.5..16, the range and the taps of ``background_blur``; None: 1.5), less ``sharpen_threshold`` gray levels
        (an int 0..255, a soft threshold that leaves noise and flat skin alone; None: 0), times A, is added to all three
        channels alike, so there are no colour fringes; coordinates outside the crop are clamped to its edge.  It is stated
        in integers and held byte for byte to a numpy reference (``sharpen.sharpen``).  It runs
        after ``min_sharpness`` and the parse, which both see the original crop (calibrated thresholds, label maps,
        attribute groups and mask files are the same with and without it), after ``denoise`` and ``clahe`` and before the
        matte, so that the guide of ``refine``, both background modes and both encoders see the sharpened crop and a fill
        colour stays exact.  It needs aligned crops like ``min_sharpness``; any ``output_size`` will do.
        ``sharpen_sigma`` or ``sharpen_threshold`` without ``sharpen`` raises ValueError.  None (the default) launches
        nothing.  ``Cropper.unsharp`` applies it to crops one already has.
        ``smooth_skin``: smooth the skin and nothing else — the range strength S, in gray levels (a finite number 1..64;
        10 suits a portrait), of a bilateral filter that the face parser guides: only pixels labelled as one of
        ``skin_classes`` (BiSeNet indices; None: (1, 7, 8, 10, 14): skin, both ears, nose, neck) change, only such pixels
        are averaged, and every other pixel of the crop stays byte-identical, so eyes, brows, lips and hair keep their
        detail and their colour does not bleed into the cheek.  Gray differences well below S are averaged away,
        differences well above S survive.  ``smooth_sigma`` (0.5..8 output pixels; None: 3.0) is the spatial sigma of the
        window (the taps of ``background_blur``, radius 3..24), ``smooth_amount`` (0.05..1; None: 1.0) how much of the
        smoothed skin replaces the crop's: below 1 some texture stays.  The effect ramps in over about three pixels from
        the edge of the skin region (the shared feather of 7), so the jagged label boundary does not show as a seam.  It is
        stated in integers and held byte for byte to a numpy reference (``skin.smooth``).  It
        runs after ``min_sharpness`` and the parse, which both see the original crop (calibrated thresholds, label maps,
        attribute groups and mask files are the same with and without it), after ``denoise``, so that grain is not
        mistaken for texture worth keeping, and before ``clahe``, ``sharpen`` and the matte, which see the smoothed crop as
        the guide of ``refine``, the background modes and both encoders do.  It creates the parser even without
        ``attr_groups`` / ``mask_groups`` or a background mode (one parse per batch serves both), needs aligned crops
        like ``min_sharpness``; any ``output_size`` will do.  ``smooth_sigma``, ``smooth_amount`` or ``skin_classes``
        without ``smooth_skin`` raises ValueError.  None (the default) launches nothing.  ``Cropper.retouch`` applies it
        to crops and label maps one already has.
        ``jpeg_quality`` (an int, 1..100; 95), ``jpeg_subsampling`` ("4:4:4", "4:2:2" or "4:2:0"; "4:2:0") and
        ``jpeg_optimize`` (per-file Huffman tables, Pillow's ``optimize=True``: smaller files, the same pixels; False):
        the settings of every JPEG file (.jpg / .jpeg / .jpe) this Cropper writes — aligned crops, the mask files of
        ``mask_groups``, the images of "no alignment" — through either encoder, which still write the same bytes
        (INTEGRATION.md section 2j); other formats are untouched.  A gray mask file has no chroma: the subsampling only
        changes the sampling byte of its frame header, as it does in Pillow.  The defaults are ``cv2.imwrite``'s, i.e. the
        reference's, and change nothing.  ``Cropper.encode_jpeg`` uses them too."""
        # the size checks of clahe and denoise quote the size in their messages as it was given: one number stays one
        size_given = (output_size,) if isinstance(output_size, (int, np.integer)) else tuple(output_size)
        self.output_size, self.resize_size = output_size, resize_size = _pair(size_given), _pair(resize_size)
        aligned = det_threshold is not None or landmarks is not None

        def needs_aligned(subject, plural=False):
            if not aligned:
                raise ValueError(f"{subject} {'need' if plural else 'needs'} aligned crops: {'they' if plural else 'it'} "
                                 f"cannot be combined with det_threshold=None and landmarks=None (no alignment), where the "
                                 f"faces are the images themselves")
        if encoder not in ("host", "device"):
            raise ValueError(f"unknown encoder {encoder!r}: choose 'host' or 'device'")
        self.encoder = encoder
        if png_encoder not in ("host", "device"):
            raise ValueError(f"unknown png_encoder {png_encoder!r}: choose 'host' or 'device'")
        self.png_encoder = png_encoder
        self.jpeg = check_jpeg_settings(jpeg_quality, jpeg_subsampling, jpeg_optimize)
        self.jpeg_quality, self.jpeg_subsampling, self.jpeg_optimize = self.jpeg
        explicit_family = warp_family if warp_family is not None else (os.environ.get("FCP_WARP_FAMILY") or None)
        align.check_interpolation(interpolation, explicit_family)
        if crop_source not in ("batch", "original"):
            raise ValueError(f"unknown crop_source {crop_source!r}: choose 'batch' or 'original'")
        if crop_source == "original" and enh_threshold is not None:
            raise ValueError("crop_source='original' cannot be combined with enh_threshold: the enhancer works on the "
                             "resized batch, which this mode does not sample")
        if min_sharpness is not None:
            if isinstance(min_sharpness, bool) or not isinstance(min_sharpness, (int, float, np.integer, np.floating)):
                raise ValueError(f"min_sharpness must be a number or None, not {min_sharpness!r}")
            if not np.isfinite(min_sharpness) or min_sharpness < 0:
                raise ValueError(f"min_sharpness must be finite and >= 0 (a variance), not {min_sharpness!r}")
            needs_aligned("min_sharpness")
            min_sharpness = float(min_sharpness)
        self.min_sharpness = min_sharpness
        self.background = matting.check_background(background)
        self.background_blur = matting.check_blur(background_blur)
        if self.background is not None and self.background_blur is not None:
            raise ValueError("background and background_blur exclude each other: the background is filled or blurred")
        self.blur_taps = None if self.background_blur is None else matting.blur_taps(self.background_blur)
        if background_image is None:
            if background_fit is not None:
                raise ValueError("background_fit needs background_image: without it it would do nothing")
        else:
            if self.background is not None or self.background_blur is not None:
                raise ValueError("background_image excludes background and background_blur: the background is filled, "
                                 "blurred or replaced by a picture")
            needs_aligned("background_image")
            self.background_fit = matting.check_fit(background_fit)
            # the pictures fitted to the output size, (K, oh, ow, 3) uint8 on the host; _init_models uploads them once
            self.background_image = matting.picture_bank(background_image, output_size, self.background_fit)
        if self.background == matting.TRANSPARENT and (not isinstance(output_format, str) or output_format.lower() != "png"):
            raise ValueError(f"background='transparent' needs output_format='png', the one format written here that keeps an "
                             f"alpha channel, not {output_format!r}")
        self.decontaminate = matting.check_decontaminate(decontaminate)
        if self.decontaminate is not None and self.background_blur is not None:
            raise ValueError("decontaminate and background_blur exclude each other: the blurred background keeps the crop's colours")
        if self.decontaminate is not None and self.background is None and self.background_image is None:
            raise ValueError("decontaminate needs background (a fill or 'transparent'): without one it would do nothing")
        self.decontaminate_taps = None if self.decontaminate is None else matting.blur_taps(self.decontaminate)
        self.refine = matting.check_refine(refine)
        if self.refine is None:
            if refine_eps is not None:
                raise ValueError("refine_eps needs refine: without it it would do nothing")
        else:
            self.refine_eps = matting.check_refine_eps(refine_eps)
            if feather is not None:
                raise ValueError("refine and feather exclude each other: the soft edge is the guided filter's or the Gaussian's")
        self.subject = matting.check_subject(subject)
        self.fill_holes = matting.check_fill_holes(fill_holes)
        self.edge_shift = matting.check_edge_shift(edge_shift)
        if not self._has_background():
            if foreground is not None or feather is not None:
                raise ValueError("foreground / feather need background or background_blur: without one they would do nothing")
            if self.refine is not None:
                raise ValueError("refine needs background or background_blur: without one it would do nothing")
            if self.subject is not None or self.fill_holes is not None:
                raise ValueError("subject / fill_holes need background or background_blur: without one they would do nothing")
            if self.edge_shift is not None:
                raise ValueError("edge_shift needs background or background_blur: without one it would do nothing")
            self.foreground, self.foreground_bits, self.feather = None, 0, None
        else:
            needs_aligned("background / background_blur", plural=True)
            self.foreground_bits = matting.check_foreground(foreground)
            self.foreground = tuple(c for c in range(matting.NUM_CLASSES) if self.foreground_bits >> c & 1)
            self.feather = 0 if self.refine is not None else matting.check_feather(feather)
        self.clahe = equalizing.check_clahe(clahe)
        if self.clahe is None:
            if clahe_grid is not None:
                raise ValueError("clahe_grid needs clahe: without it it would do nothing")
        else:
            needs_aligned("clahe")
            self.clahe_grid = equalizing.check_grid(clahe_grid, size_given)
        self.denoise = denoising.check_denoise(denoise)
        if self.denoise is not None:
            needs_aligned("denoise")
            denoising.check_size(size_given)
        self.sharpen = sharpening.check_sharpen(sharpen)
        if self.sharpen is None:
            for name, value in (("sharpen_sigma", sharpen_sigma), ("sharpen_threshold", sharpen_threshold)):
                if value is not None:
                    raise ValueError(f"{name} needs sharpen: without it it would do nothing")
        else:
            needs_aligned("sharpen")
            self.sharpen_sigma = sharpening.check_sigma(sharpen_sigma)
            self.sharpen_threshold = sharpening.check_threshold(sharpen_threshold)
        self.smooth_skin = smoothing.check_smooth_skin(smooth_skin)
        if self.smooth_skin is None:
            for name, value in (("smooth_sigma", smooth_sigma), ("smooth_amount", smooth_amount), ("skin_classes", skin_classes)):
                if value is not None:
                    raise ValueError(f"{name} needs smooth_skin: without it it would do nothing")
        else:
            needs_aligned("smooth_skin")
            self.smooth_sigma = smoothing.check_sigma(smooth_sigma)
            self.smooth_amount = smoothing.check_amount(smooth_amount)
            self.skin_bits = smoothing.check_classes(skin_classes)
            self.skin_classes = tuple(c for c in range(matting.NUM_CLASSES) if self.skin_bits >> c & 1)
        self.crop_source, self.interpolation, self.output_format = crop_source, interpolation, output_format
        self.face_factor, self.strategy, self.padding, self.allow_skew = face_factor, strategy, padding, allow_skew
        self.attr_groups, self.mask_groups = attr_groups, mask_groups
        self.det_threshold, self.enh_threshold = det_threshold, enh_threshold
        self.batch_size, self.num_processes = batch_size, num_processes
        self.device = device
        if isinstance(device, str):
            self.device = torch.device("cuda:0" if device in ("cuda", "hip") else device.replace("hip", "cuda"))
        self.landmarks = parse_landmarks_file(landmarks) if isinstance(landmarks, str) else landmarks
        self.weights = weights or {}
        self.precision = precision   # "f16x3" (default) | "f32": arithmetic of the conv engine
        self.num_std_landmarks = 5
        # GPU worker threads of process_dir (each runs whole batches: upload, detect, align, read-back).  The reference's
        # `num_processes` is the size of its ThreadPool (cropper.py:900-902, default 1); here one worker leaves the device idle
        # while it is in its host phases — 2365-2438 images/s end to end against 3148-3209 with two (profiles/r06_probes.md
        # section 2) — so at least two batches (three for batch_size <= 8) are in flight unless told otherwise (gpu_workers = 1, or FCP_GPU_WORKERS=1).
        # The output set does not depend on it (tests/test_cropper_gpu.py::test_process_dir_pipeline_is_deterministic).
        self.gpu_workers = int(os.environ["FCP_GPU_WORKERS"]) if os.environ.get("FCP_GPU_WORKERS") else None
        # host I/O threads of process_dir (decode prefetch + asynchronous encode/write around the GPU workers)
        self.io_threads = max(2, min(16, (os.cpu_count() or 4) // 2))
        # ... and, by default, one decode / encode worker PROCESS behind every I/O thread (_io_pool.py): the
        # Pillow work leaves the parent's interpreter lock.  (readers, writers); None = sized from the host's cores;
        # FCP_IO_PROCESSES=0 (or io_processes = (0, 0)) keeps decode / encode on the threads
        self.io_processes = (0, 0) if os.environ.get("FCP_IO_PROCESSES", "1") == "0" else None
        self.io_ring_mb = None       # shared-memory ring of a decode worker in MiB (None: FCP_IO_RING_MB, default 128)
        self._io_procs = None
        # set by process_dir as ONE tuple (executor the encoded files are written on, futures of the writes still in
        # flight, semaphore bounding them), so that a task of a failed run can never see a half-reset state
        self._io = None
        self._write_lock = Lock()

        self._init_models()
        self._init_landmarks_target()
        if interpolation == "linear":
            self.warp_family = align.resolve_warp_family(warp_family, self.padding, self.device)
        else:
            # cubic and Lanczos-4 exist in the fixed-point family only (whose coordinates they share): "auto" has nothing
            # to pick, an unknown name still raises
            self.warp_family = ("fixed" if explicit_family in (None, "auto")
                                else align.resolve_warp_family(explicit_family, self.padding, self.device))

    # ------------------------------------------------------------------ init
    def _init_models(self):
        """cropper.py:346-390.  One immutable model set per Cropper (the reference
        re-creates them in every pool thread on the shared ``self``)."""
        self.det_model = None
        self.enh_model = None
        self.par_model = None
        if self.device.type != "cuda":
            raise RuntimeError("face_crop_plus_amd: device must be an AMD GPU ('cuda:N'); no CPU fallback")
        if self.device.index is not None:
            torch.cuda.set_device(self.device.index)
        if self.det_threshold is not None and self.landmarks is None:
            from .retinaface import RetinaFace
            self.det_model = RetinaFace(self.strategy, self.det_threshold)
            self.det_model.load(self.device, self.weights.get("retinaface"), self.precision)
        if self.enh_threshold is not None:
            from .rrdb import RRDBNet
            self.enh_model = RRDBNet(self.enh_threshold)
            self.enh_model.load(self.device, self.weights.get("rrdb"), self.precision)
        if self.attr_groups is not None or self.mask_groups is not None or self._needs_labels():
            from .bise import BiSeNet
            self.par_model = BiSeNet(self.attr_groups, self.mask_groups, self.batch_size)
            self.par_model.load(self.device, self.weights.get("bisenet"), self.precision)
            self.par_model.masks_on_device = self._encodes_on_device()
        image = self.background_image
        self._pictures_dev = None if image is None else torch.from_numpy(image).to(self.device)

    def _has_background(self) -> bool:
        """Whether a background mode is on: a fill or a cut-out, a blur, or pictures."""
        return self.background is not None or self.background_blur is not None or self.background_image is not None

    def _needs_labels(self) -> bool:
        """Whether a finishing step reads the parser's label map: a background mode, or ``smooth_skin``."""
        return self._has_background() or self.smooth_skin is not None

    def _init_landmarks_target(self):
        if self.num_std_landmarks != 5:
            raise ValueError(f"Unsupported number of standard landmarks for estimating alignment transform "
                             f"matrix: {self.num_std_landmarks}.")
        self.landmarks_target = landmarks_target(self.output_size, self.face_factor)

    # ------------------------------------------------------------ crop_align
    def _crop_align_device(self, images_dev, paddings, indices, landmarks_dev):
        """Device tensors in, (crops (F,oh,ow,3) u8 device, ok (F,) i32 device) out."""
        pads = None if paddings is None else torch.as_tensor(np.asarray(paddings), dtype=torch.int32)
        idx = indices if isinstance(indices, torch.Tensor) else torch.as_tensor(np.asarray(indices), dtype=torch.int32)
        crops, ok, _ = align.crop_align(images_dev, idx, landmarks_dev, self.landmarks_target, self.output_size,
                                        align.border_code(self.padding), self.allow_skew, pads, family=self.warp_family,
                                        interpolation=self.interpolation)
        return crops, ok

    def _source_landmarks(self, images, paddings, indices, lm_batch):
        """Detector landmarks in the batch (before un-padding) -> the same points in each face's decoded image."""
        geo = [batch_geometry(im.shape[0], im.shape[1], self.resize_size) for im in images]
        idx = np.asarray(indices, np.int64)
        w = np.array([images[i].shape[1] for i in idx]); h = np.array([images[i].shape[0] for i in idx])
        ww = np.array([geo[i][0] for i in idx]); hh = np.array([geo[i][1] for i in idx])
        return align.source_landmarks(lm_batch, w, h, ww, hh, paddings[idx, 2], paddings[idx, 0])

    def crop_align(self, images, padding, indices, landmarks_source) -> np.ndarray:
        """Reference signature (cropper.py:441-552): numpy in, numpy out.  ``images`` is an
        (N,H,W,3) uint8 array or a list of differently-sized arrays."""
        if len(indices) == 0:
            return np.array([])
        lms = torch.from_numpy(np.ascontiguousarray(landmarks_source, dtype=np.float32))
        outs = []
        if isinstance(images, np.ndarray) and images.ndim == 4:
            dev_imgs = torch.from_numpy(np.ascontiguousarray(images)).to(self.device)
            crops, ok = self._crop_align_device(dev_imgs, padding, list(indices), lms.to(self.device))
            crops, ok = crops.cpu().numpy(), ok.cpu().numpy()
            outs = [c for c, o in zip(crops, ok) if o]
        else:
            # ragged list: one upload + one launch per source image, face order preserved
            order = defaultdict(list)
            for li, ii in enumerate(indices):
                order[int(ii)].append(li)
            res = {}
            for ii, lis in order.items():
                dev_img = torch.from_numpy(np.ascontiguousarray(images[ii])).to(self.device)[None]
                pad = None if padding is None else np.asarray(padding)[ii:ii + 1]
                crops, ok = self._crop_align_device(dev_img, pad, [0] * len(lis), lms[lis].to(self.device))
                for li, c, o in zip(lis, crops.cpu().numpy(), ok.cpu().numpy()):
                    if o:
                        res[li] = c
            outs = [res[li] for li in sorted(res)]
        return np.stack(outs) if len(outs) > 0 else np.array(outs)

    def sharpness(self, crops: np.ndarray) -> np.ndarray:
        """The score ``min_sharpness`` is compared with, for crops one already has: (F,H,W,3) uint8 RGB -> (F,) float64
        variance of the Laplacian (``align.sharpness_score``)."""
        crops = _u8_crops(crops)
        if crops.shape[0] == 0:
            return np.zeros(0, np.float64)
        with torch.cuda.device(self.device):
            sums = align.sharpness_sums(torch.from_numpy(crops).to(self.device))
            return align.sharpness_score(sums, crops.shape[1] * crops.shape[2])

    def matte(self, crops: np.ndarray, labels: np.ndarray, picks=None):
        """What ``background`` does, for crops and label maps one already has: (F,H,W,3) uint8 RGB crops and (F,H,W)
        uint8 labels -> (the composited crops (F,H,W,3) uint8, the alpha (F,H,W) uint8), with this Cropper's
        ``background`` / ``foreground`` / ``feather`` (``matte.matte``), or with its ``background_blur``
        (``matte.matte_blur``); with ``refine`` the alpha is the guided filter's (``matte.refine_alpha``) and the
        composite goes through it; with ``subject`` / ``fill_holes`` the mask is cleaned first (``matte.subject_mask``),
        and with ``edge_shift`` its boundary is then moved (``matte.shift_mask``).
        With ``background="transparent"`` the first array is the RGBA cut-out (F,H,W,4) itself; with ``decontaminate`` its
        colours, or those composited over the fill, are the estimated subject colours (``matte.cutout``).
        With ``background_image`` the crops must have this Cropper's ``output_size`` and crop i goes over picture
        ``picks[i]`` of the K (F ints 0..K-1; None: ``i % K``), through ``matte.matte_image`` / ``matte.cutout_image``;
        without it ``picks`` must be None."""
        if not self._has_background():
            raise ValueError("Cropper.matte needs a Cropper with background=..., background_blur=... or background_image=...")
        crops, labels = _u8_crops(crops), np.ascontiguousarray(labels)
        if labels.dtype != np.uint8 or labels.shape != crops.shape[:3]:
            raise ValueError(f"labels must be {crops.shape[:3]} uint8, not {labels.dtype} {labels.shape}")
        image = self.background_image
        if image is None:
            if picks is not None:
                raise ValueError("picks need a Cropper with background_image=...: a fill or a blur has no pictures to pick from")
        else:
            if crops.shape[1:3] != image.shape[1:3]:
                raise ValueError(f"crops must have the output size of the pictures, (F,{image.shape[1]},{image.shape[2]},3), "
                                 f"not {crops.shape}")
            if picks is not None:
                picks = list(picks)
                if len(picks) != len(crops) or not all(matting._is_int(p) and 0 <= int(p) < len(image) for p in picks):
                    raise ValueError(f"picks must be {len(crops)} ints 0..{len(image) - 1}, one per crop, not {picks!r}")
        if crops.size == 0:
            return np.zeros(crops.shape, np.uint8), np.zeros(labels.shape, np.uint8)
        with torch.cuda.device(self.device):
            crops_dev, labels_dev = torch.from_numpy(crops).to(self.device), torch.from_numpy(labels).to(self.device)
            more = {} if image is None else {"picks": picks}
            out, alpha = self._matte_device(crops_dev, labels_dev, with_alpha=True, **more)
            return out.cpu().numpy(), alpha.cpu().numpy()

    def _matte_device(self, crops_dev, labels_dev, with_alpha=False, picks=None):
        """The matte step on device tensors: the cleaned mask first when ``subject`` / ``fill_holes`` are set (it takes
        the label map's place, as class 1), its boundary moved when ``edge_shift`` is set (likewise), the refined alpha when
        ``refine`` is set, then the composite.  ``picks``: with ``background_image``, the picture of each crop (None:
        crop i over picture ``i % K``)."""
        bits = self.foreground_bits
        if self.subject is not None or self.fill_holes is not None:
            labels_dev = matting.subject_mask(labels_dev, bits, self.subject is not None, self.fill_holes or 0)
            bits = matting.SUBJECT_BITS
        if self.edge_shift is not None:
            labels_dev = matting.shift_mask(labels_dev, bits, self.edge_shift)
            bits = matting.SUBJECT_BITS
        refined = {}
        if self.refine is not None:
            refined["alpha"] = matting.refine_alpha(crops_dev, labels_dev, bits, self.refine, self.refine_eps)
        if self.background_blur is not None:
            return matting.matte_blur(crops_dev, labels_dev, bits, self.feather, self.blur_taps, with_alpha=with_alpha, **refined)
        taps = self.decontaminate_taps
        if self.background_image is not None:
            # the colour branch below, over the bank: the decontaminated composite reads an alpha plane, the plain one not
            bank = self._pictures_dev
            if picks is None:
                picks = [i % bank.shape[0] for i in range(crops_dev.shape[0])]
            if taps is None:
                return matting.matte_image(crops_dev, labels_dev, bits, self.feather, bank, picks, with_alpha=with_alpha, **refined)
            alpha = refined["alpha"] if refined else matting.feather_alpha(labels_dev, bits, self.feather)
            return matting.cutout_image(crops_dev, alpha, bank, picks, taps), (alpha if with_alpha else None)
        transparent = self.background == matting.TRANSPARENT
        if transparent or taps is not None:
            # the cut-out and the decontaminated composite read an alpha plane: the refined one, or the feathered mask
            alpha = refined["alpha"] if refined else matting.feather_alpha(labels_dev, bits, self.feather)
            out = matting.cutout(crops_dev, alpha, None if transparent else self.background, taps)
            return out, (alpha if with_alpha else None)
        return matting.matte(crops_dev, labels_dev, bits, self.feather, self.background, with_alpha=with_alpha, **refined)

    def _filter_crops(self, crops, step) -> np.ndarray:
        """One device step over crops one already has: (F,H,W,3) uint8 on the host -> what ``step`` makes of them on the
        device, back on the host."""
        crops = _u8_crops(crops)
        if crops.shape[0] == 0:
            return np.zeros(crops.shape, np.uint8)
        with torch.cuda.device(self.device):
            return step(torch.from_numpy(crops).to(self.device)).cpu().numpy()

    def equalize(self, crops: np.ndarray) -> np.ndarray:
        """What ``clahe`` does, for crops one already has: (F,H,W,3) uint8 RGB -> the equalised crops (F,H,W,3) uint8,
        with this Cropper's ``clahe`` / ``clahe_grid`` (``clahe.clahe``)."""
        if self.clahe is None:
            raise ValueError("Cropper.equalize needs a Cropper with clahe=...")
        return self._filter_crops(crops, lambda dev: equalizing.clahe(dev, self.clahe, self.clahe_grid))

    def remove_noise(self, crops: np.ndarray) -> np.ndarray:
        """What ``denoise`` does, for crops one already has: (F,H,W,3) uint8 RGB -> the denoised crops (F,H,W,3) uint8,
        at this Cropper's filter strength (``denoise.denoise``)."""
        if self.denoise is None:
            raise ValueError("Cropper.remove_noise needs a Cropper with denoise=...")
        return self._filter_crops(crops, lambda dev: denoising.denoise(dev, self.denoise))

    def unsharp(self, crops: np.ndarray) -> np.ndarray:
        """What ``sharpen`` does, for crops one already has: (F,H,W,3) uint8 RGB -> the sharpened crops (F,H,W,3) uint8,
        at this Cropper's amount, sigma and threshold (``sharpen.sharpen``)."""
        if self.sharpen is None:
            raise ValueError("Cropper.unsharp needs a Cropper with sharpen=...")
        return self._filter_crops(crops, lambda dev: sharpening.sharpen(dev, self.sharpen, self.sharpen_sigma, self.sharpen_threshold))

    def retouch(self, crops: np.ndarray, labels: np.ndarray) -> np.ndarray:
        """What ``smooth_skin`` does, for crops and label maps one already has: (F,H,W,3) uint8 RGB crops and (F,H,W)
        uint8 labels -> the crops with the skin smoothed (F,H,W,3) uint8, at this Cropper's strength, sigma, amount and
        skin classes (``skin.smooth``)."""
        if self.smooth_skin is None:
            raise ValueError("Cropper.retouch needs a Cropper with smooth_skin=...")
        crops, labels = _u8_crops(crops), np.ascontiguousarray(labels)
        if labels.dtype != np.uint8 or labels.shape != crops.shape[:3]:
            raise ValueError(f"labels must be {crops.shape[:3]} uint8, not {labels.dtype} {labels.shape}")
        if crops.size == 0:
            return np.zeros(crops.shape, np.uint8)
        with torch.cuda.device(self.device):
            labels_dev = torch.from_numpy(labels).to(self.device)
            return self._smooth_device(torch.from_numpy(crops).to(self.device), labels_dev).cpu().numpy()

    def _smooth_device(self, crops_dev, labels_dev):
        """The skin step on device tensors."""
        return smoothing.smooth(crops_dev, labels_dev, self.smooth_skin, self.smooth_sigma, self.smooth_amount, self.skin_bits)

    def encode_jpeg(self, crops: np.ndarray) -> list:
        """What ``encoder="device"`` writes, for crops one already has: (F,H,W,3) or (F,H,W) uint8 -> F JPEG files as
        bytes, each equal to the file the host encoder writes for those pixels (``jpegenc.encode_jpeg``)."""
        from . import jpegenc
        crops = _u8_crops(crops, gray=True)
        if crops.shape[0] == 0:
            return []
        with torch.cuda.device(self.device):
            return jpegenc.encode_jpeg(torch.from_numpy(crops).to(self.device), **self._jpeg_kw())

    def encode_png(self, crops: np.ndarray) -> list:
        """What ``png_encoder="device"`` writes, for crops one already has: (F,H,W,3), (F,H,W,4) (RGBA cut-outs) or
        (F,H,W) uint8 -> F PNG files as bytes, each of which decodes to those pixels (``pngenc.encode_png``); not the host
        encoder's bytes."""
        from . import pngenc
        crops = _u8_crops(crops, channels=(3, 4), gray=True)
        if crops.shape[0] == 0:
            return []
        with torch.cuda.device(self.device):
            return pngenc.encode_png(torch.from_numpy(crops).to(self.device))

    def _encodes_on_device(self) -> bool:
        """Whether some format is compressed on the GPU: then crops and masks stay there until they are saved."""
        return self.encoder == "device" or self.png_encoder == "device"

    def _jpeg_kw(self) -> dict:
        """Keywords of ``jpegenc.encode_jpeg`` for this Cropper's settings; none at all for the defaults."""
        jpeg = self.jpeg
        if jpeg is None or jpeg == JpegSettings():
            return {}
        return dict(quality=jpeg.quality, subsampling=jpeg.subsampling, optimize=jpeg.optimize)

    # ----------------------------------------------------------------- saving
    MAX_PENDING_WRITES = 256     # encode / write tasks in flight before a GPU worker waits (process_dir)

    def _target_paths(self, file_names, output_dir: str):
        """Where each face of one group goes, in face order.  Naming rules of the reference's writer
        (cropper.py:588-603): the source file's stem; with strategy "all" a running "_<k>" per source file,
        counted inside this group, starting at 0; the source extension unless ``output_format`` overrides it."""
        nth = Counter()
        paths = []
        for source in map(str, file_names):
            stem, ext = os.path.splitext(source)
            if self.output_format is not None:
                ext = "." + self.output_format
            if self.strategy == "all":
                stem = f"{stem}_{nth[source]}"
                nth[source] += 1
            paths.append(os.path.join(output_dir, stem + ext))
        return paths

    def _emit(self, path: str, pixels):
        """Write one file — pixels to encode, or the bytes of a file the GPU has encoded — inline, or — inside
        process_dir — as a task on the I/O pool.  At most
        MAX_PENDING_WRITES tasks are in flight: a slow disk stalls the GPU worker here instead of piling uint8
        crops up in host memory, and a failed write surfaces at the next batch, not at the end of the run."""
        # Locals: process_dir resets the attributes when it unwinds, while tasks of a failed run may still be in flight.
        writer, writes, slots = self._io or (None, None, None)      # ONE read: never a torn triple
        encoded = isinstance(pixels, bytes)
        jpeg = self.jpeg
        # the defaults are the encoder table's own entry: the writers are called as they always were
        jpeg = {} if jpeg is None or jpeg == JpegSettings() else {"jpeg": jpeg}
        if writer is None:
            write_bytes(path, pixels) if encoded else write_image(path, pixels, **jpeg)
            return
        slots.acquire()
        procs = self._io_procs_active        # encode in the thread's worker process, or on the thread

        def task():
            try:
                if procs is not None:
                    procs.write_bytes(path, pixels) if encoded else procs.write(path, pixels, **jpeg)
                else:
                    write_bytes(path, pixels) if encoded else write_image(path, pixels, **jpeg)
            finally:
                slots.release()
        with self._write_lock:
            done = [w for w in writes if w.done()]
            writes[:] = [w for w in writes if not w.done()]
            try:
                writes.append(writer.submit(task))
            except BaseException:
                slots.release()          # the task will never run: give its slot back
                raise
        for w in done:
            w.result()               # re-raise an encode / write error of an earlier file now

    def save_group(self, faces, file_names, output_dir: str):
        """One directory of faces (or masks) — reference ``save_group``, cropper.py:554-609, with Pillow as the
        encoder (arrays are RGB already, so there is no colour swap)."""
        if len(faces) == 0:
            return
        os.makedirs(output_dir, exist_ok=True)
        for path, pixels in zip(self._target_paths(file_names, output_dir), faces):
            self._emit(path, pixels if isinstance(pixels, bytes) else np.asarray(pixels))

    def save_groups(self, faces, file_names, output_dir, attr_groups, mask_groups):
        """Directory tree ``output_dir/<attr group>/<mask group>[_mask]`` — reference ``save_groups``,
        cropper.py:611-746.  A face lands in every (attr, mask) cell both groups list it in; the masks of a
        cell go to the sibling ``<mask group>_mask`` directory under the same file names."""
        everyone = list(range(len(faces)))
        attrs = {"": everyone} if attr_groups is None else attr_groups
        masks = {"": (everyone, None)} if mask_groups is None else mask_groups
        for (attr_name, in_attr), (mask_name, (in_mask, mask_rows)) in itertools.product(attrs.items(), masks.items()):
            # Order matters (it decides which face of a file gets which "_<k>"): the reference iterates the
            # CPython set `set(a) & set(b)`, so the very same expression is evaluated here.
            cell = list(set(in_attr) & set(in_mask))
            cell_dir = os.path.join(output_dir, attr_name, mask_name)
            sources = file_names[cell]
            self.save_group([faces[i] for i in cell], sources, cell_dir)
            if mask_rows is not None:
                row_of = {}
                for row, face in enumerate(in_mask):
                    row_of.setdefault(face, row)
                self.save_group([mask_rows[row_of[i]] for i in cell], sources, cell_dir + "_mask")

    def _is_target(self, file_names, fmt):
        """Per source file name: whether the face cut from it is written in the format ``fmt`` of the encoder table, as
        ``jpegenc.JPEG_EXTENSIONS`` / ``pngenc.PNG_EXTENSIONS`` list it (``_target_paths``' extension rule)."""
        hit = lambda ext: _ENCODER_KW.get(ext.lower(), {}).get("format") == fmt
        if self.output_format is not None:
            return np.full(len(file_names), hit("." + self.output_format))
        return np.array([hit(os.path.splitext(str(n))[1]) for n in file_names], bool)

    def _is_jpeg_target(self, file_names):
        return self._is_target(file_names, "JPEG")

    def _is_png_target(self, file_names):
        return self._is_target(file_names, "PNG")

    def _encode_on_device(self, pixels_dev, pixels, names):
        """``encoder="device"`` / ``png_encoder="device"``: (F,H,W[,3 or 4]) u8 device pixels (and their host copy, if one
        exists already) of the faces or masks cut from ``names`` -> a list with the encoded file (bytes) of every face
        whose format is compressed on the GPU — JPEG targets by ``encoder``, PNG targets by ``png_encoder`` — and the
        host pixels of every other.  The pixels are read back only when some target needs the host."""
        from . import jpegenc, pngenc
        none = np.zeros(len(names), bool)
        jpeg = self._is_jpeg_target(names) if self.encoder == "device" else none
        png = self._is_png_target(names) if self.png_encoder == "device" else none
        out = [None] * len(names)
        for which, label, encode in ((jpeg, "fcp:jpeg", lambda rows: jpegenc.encode_jpeg(rows, **self._jpeg_kw())),
                                     (png, "fcp:png", pngenc.encode_png)):
            if which.any():
                with trace.range(label):
                    rows = pixels_dev if which.all() else pixels_dev[torch.from_numpy(which).to(pixels_dev.device)].contiguous()
                    for i, data in zip(np.nonzero(which)[0], encode(rows)):
                        out[i] = data
        on_host = ~(jpeg | png)
        if on_host.any():
            host = pixels if pixels is not None else pixels_dev.cpu().numpy()
            for i in np.nonzero(on_host)[0]:
                out[i] = host[i]
        return out

    # ------------------------------------------------------------- processing
    def _landmark_rows(self, table_names):
        """file name -> rows of the user's landmark table, built once per table (not per batch)."""
        cached = self._rows_cache
        if cached is None or cached[0] is not table_names:
            rows_of = defaultdict(list)
            for row, name in enumerate(table_names):
                rows_of[str(name)].append(row)
            cached = self._rows_cache = (table_names, rows_of)
        return cached[1]

    @torch.no_grad()
    def process_batch(self, file_names, input_dir: str, output_dir: str):
        """cropper.py:748-850."""
        images, file_names = read_images(file_names, input_dir)
        self._process_images(images, file_names, output_dir)

    def _locate(self, images, file_names, pinned):
        """Where the faces are.  Decoded images (host) and their names in -> (indices, landmarks, images_dev, paddings,
        sources): the image of every face (a list), its five landmarks there ((F,5,2) on the host; None without alignment:
        every image is one "face"), and what the detector path leaves: the resized batch on the device, its paddings on the
        host and, with ``crop_source="original"``, the (blob, (N,3) table) of the decoded images on the device."""
        landmarks = images_dev = paddings = sources = None
        if self.landmarks is None and self.det_model is None:
            indices = list(range(len(file_names)))              # one "face" per image, no alignment
        elif self.landmarks is not None:
            # user-supplied landmark sets (cropper.py:796-813): rows of the landmark table whose file name is in
            # this batch, grouped by image in batch order; images without a row are dropped
            table, table_names = self.landmarks
            rows_of = self._landmark_rows(table_names)
            pairs = [(i, row) for i, name in enumerate(file_names) for row in rows_of.get(str(name), ())]
            indices = [i for i, _ in pairs]
            landmarks = table[[row for _, row in pairs]]
        else:
            original = self.crop_source == "original"
            with trace.range("fcp:build_batch"):
                images_dev, _, paddings, *kept = build_batch(images, self.resize_size, "constant", self.device, pinned,
                                                             keep_sources=original)
            with trace.range("fcp:detect"):
                landmarks, indices = self.det_model.predict(images_dev)
            if original:
                sources = kept[0]
                if len(indices):
                    landmarks = self._source_landmarks(images, paddings, indices, landmarks)
            elif len(indices):
                landmarks = landmarks - paddings[indices][:, None, [2, 0]].astype(np.float32)
        if landmarks is not None and len(landmarks) > 0 and landmarks.shape[1] != self.num_std_landmarks:
            slices = get_ldm_slices(self.num_std_landmarks, landmarks.shape[1])
            landmarks = np.stack([landmarks[:, s].mean(1) for s in slices], 1)
        return indices, landmarks, images_dev, paddings, sources

    def _enhance(self, images, images_dev, landmarks, indices):
        """The enhancer over the images whose faces pass its gate: the device batch in -> the enhanced batch out; without
        one (given landmarks: a ragged list on the host) the enhanced images replace their entries of ``images``."""
        with trace.range("fcp:enhance"):
            if images_dev is not None:
                return self.enh_model.predict(images_dev, landmarks, indices)
            # ragged list (no detector): the reference hands the whole list to RRDBNet.predict (cropper.py:833-836), whose
            # gate measures every image's faces against the area of images[0] (rrdb.py:124-140) and skips images that have no landmark set
            todo = self.enh_model.gate(len(images), images[0].shape[0], images[0].shape[1], landmarks, indices)
            for i in todo:
                images[i] = self.enh_model.predict(torch.from_numpy(images[i]).to(self.device)[None], None, None)[0].cpu().numpy()
        return None

    def _align(self, images, images_dev, paddings, sources, indices, landmarks, pinned):
        """Estimate + warp.  What ``_locate`` returned in -> (faces, faces_dev, indices): the crops on the host (None when
        a device encoder will read them where they are), the same crops (F,oh,ow,3) u8 on the device, and the image of
        every face that is left.  Without alignment the faces are the decoded images, on the host alone."""
        if landmarks is None:
            # no alignment: the decoded images themselves are the "faces".  Inside process_dir they may be views of a
            # decode worker's shared-memory ring, which is recycled as soon as this call returns, while the encode
            # tasks run later: they get their own copies
            return ([np.array(im) for im in images] if pinned is not None else images), None, indices
        original = self.crop_source == "original"
        if not original and images_dev is None:          # given landmarks: a ragged list of images on the host
            with trace.range("fcp:align"):
                faces = self.crop_align(images, paddings, indices, landmarks)
            return faces, (torch.from_numpy(faces).to(self.device) if len(faces) else None), indices
        with trace.range("fcp:align"):
            landmarks = np.ascontiguousarray(landmarks, dtype=np.float32)
            if original:
                if sources is None:          # given landmarks: the originals have not been uploaded yet
                    sources = upload_sources(images, self.device, pinned)
                crops_dev, ok, _, _ = align.crop_align_sources(
                    *sources, indices, landmarks, self.landmarks_target, self.output_size, align.border_code(self.padding),
                    self.allow_skew, self.warp_family, self.interpolation)
            else:
                crops_dev, ok = self._crop_align_device(images_dev, paddings, list(indices), torch.from_numpy(landmarks).to(self.device))
        _, crops_dev, indices = self._keep(ok.cpu().numpy() != 0, None, crops_dev, indices)
        return self._host_copy(crops_dev), crops_dev, indices

    @staticmethod
    def _keep(keep, faces, faces_dev, indices):
        """Drop faces.  ``keep``: (F,) bool on the host -> the kept rows of ``faces`` (host, or None), of ``faces_dev``
        (device) and of ``indices`` (a list), in their order."""
        faces = None if faces is None else faces[keep]
        return faces, faces_dev[torch.from_numpy(keep).to(faces_dev.device)], [i for i, k in zip(indices, keep) if k]

    def _drop_blurry(self, faces, faces_dev, indices):
        """``min_sharpness``: the crops (host and / or device) in -> ``_keep`` of those whose score reaches it."""
        with trace.range("fcp:sharpness"):
            if faces_dev is None:
                faces_dev = torch.from_numpy(np.ascontiguousarray(faces)).to(self.device)
            score = align.sharpness_score(align.sharpness_sums(faces_dev), faces_dev.shape[1] * faces_dev.shape[2])
        return self._keep(score >= self.min_sharpness, faces, faces_dev, indices)

    def _parse(self, faces, faces_dev):
        """The face parser over the crops (device; host crops are uploaded one by one) -> (groups, labels): the
        (attr_groups, mask_groups) pair ``save_groups`` takes and, when a background mode or ``smooth_skin`` will use it,
        the label map (F,oh,ow) u8 on the device behind them, else None."""
        if faces_dev is None:
            faces_dev = [torch.from_numpy(np.ascontiguousarray(f)).to(self.device) for f in faces]
        with trace.range("fcp:parse"):
            if self._needs_labels() and isinstance(faces_dev, torch.Tensor):
                # one parse per batch: the label map behind the groups is the one the skin step and the matte use
                *groups, labels = self.par_model.predict(faces_dev, return_labels=True)
                return tuple(groups), labels
            return self.par_model.predict(faces_dev), None

    def _finish_crops(self, faces_dev, labels, names, output_dir, skin_labels=None):
        """What changes the pixels of a crop, after the parse, which saw the original crop: first the noise, then the
        skin, then the contrast, then the edges, over the whole crop, then the fill.  Crops (F,oh,ow,3) u8, the label map
        of the matte (or None: no matte) and that of the skin step (or None: no skin step), all on the device, and the
        source file name of every face in -> the finished crops on the device: the very object that came in when no step
        is switched on.  Nothing is read back here."""
        if self.denoise is not None:
            with trace.range("fcp:denoise"):
                faces_dev = denoising.denoise(faces_dev, self.denoise)
        if self.smooth_skin is not None and skin_labels is not None:
            with trace.range("fcp:skin"):
                faces_dev = self._smooth_device(faces_dev, skin_labels)
        if self.clahe is not None:
            with trace.range("fcp:clahe"):
                faces_dev = equalizing.clahe(faces_dev, self.clahe, self.clahe_grid)
        if self.sharpen is not None:
            with trace.range("fcp:sharpen"):
                faces_dev = sharpening.sharpen(faces_dev, self.sharpen, self.sharpen_sigma, self.sharpen_threshold)
        if labels is not None:
            with trace.range("fcp:matte"):
                more = {}
                if self.background_image is not None:    # a face's picture comes from the name of its file in the output directory
                    more["picks"] = matting.pick_pictures(self._target_paths(names, output_dir), len(self.background_image))
                faces_dev, _ = self._matte_device(faces_dev, labels, **more)
        return faces_dev

    def _host_copy(self, pixels_dev):
        """Device pixels -> their copy on the host, or None with a device encoder: the pixels stay where they are, and
        what is read back is decided when they are saved."""
        return None if self._encodes_on_device() else pixels_dev.cpu().numpy()

    @torch.no_grad()
    def _process_images(self, images, file_names, output_dir: str, pinned=None):
        """Everything of ``process_batch`` after the files have been decoded.  ``pinned``: per-image flags of arrays that
        live in page-locked memory (``build_batch`` uploads those without a staging copy)."""
        if len(images) == 0:
            return
        with torch.cuda.device(self.device):
            indices, landmarks, images_dev, paddings, sources = self._locate(images, file_names, pinned)
            if landmarks is not None and len(landmarks) == 0:
                return
            if self.enh_model is not None:
                images_dev = self._enhance(images, images_dev, landmarks, indices)
            faces, faces_dev, indices = self._align(images, images_dev, paddings, sources, indices, landmarks, pinned)
            if self.min_sharpness is not None and landmarks is not None and len(indices) > 0:
                faces, faces_dev, indices = self._drop_blurry(faces, faces_dev, indices)
            groups, labels = (None, None), None
            if self.par_model is not None and len(indices) > 0:
                groups, labels = self._parse(faces, faces_dev)
            if len(indices) > 0 and isinstance(faces_dev, torch.Tensor):
                finished = self._finish_crops(faces_dev, labels if self._has_background() else None, file_names[indices], output_dir,
                                              skin_labels=labels)
                if finished is not faces_dev:       # the host encoder's copy is the finished crop as well
                    faces_dev, faces = finished, self._host_copy(finished)
            if self._encodes_on_device() and isinstance(faces_dev, torch.Tensor):
                # aligned crops (and their masks): same size, on the device.  Faces and mask rows become lists that hold
                # the encoded file of every target a device encoder takes, in the order save_groups indexes them
                names = file_names[indices]
                faces = self._encode_on_device(faces_dev, faces, names) if len(indices) > 0 else []
                if groups[1] is not None:
                    groups = (groups[0], {k: (rows_of, self._encode_on_device(m, None, names[rows_of]))
                                          for k, (rows_of, m) in groups[1].items()})
            elif groups[1] is not None:          # no aligned crops to encode here: the masks go to the host encoder as well
                groups = (groups[0], {k: (rows_of, m.cpu().numpy() if isinstance(m, torch.Tensor) else m)
                                      for k, (rows_of, m) in groups[1].items()})
        with trace.range("fcp:save"):
            self.save_groups(faces, file_names[indices], output_dir, *groups)

    def process_dir(self, input_dir: str, output_dir: str | None = None, desc: str | None = "Processing"):
        """cropper.py:852-909: batches of file names over a thread pool sharing the models."""
        if output_dir is None:
            output_dir = input_dir + "_faces"
        files, bs = os.listdir(input_dir), self.batch_size
        files = sorted(files)          # deterministic batches, so ranks agree on the partition
        file_batches = [files[i:i + bs] for i in range(0, len(files), bs)]
        from .dist import shard
        file_batches = shard(file_batches)   # rank r of R takes batches r, r+R, ... (no-op single-process)
        if len(file_batches) == 0:
            return
        # Overlapped host I/O: decode is prefetched `depth` batches ahead on an I/O pool, the
        # `num_processes` GPU workers of the reference's ThreadPool only run the device pipeline, and the
        # encoded crops / masks are written asynchronously on the same I/O pool.  File naming, warn-and-skip
        # and the output directory layout are exactly those of the synchronous `process_batch`.
        from concurrent.futures import ThreadPoolExecutor
        # small batches (the reference's default batch_size = 8) leave the device idle even with two in flight: 1264-1282 images/s
        # end to end with three workers against 1086-1258 with two (batch 8 @1024^2), while batch 32 prefers two (1357-1368 against 1261-1289)
        workers = max(1, self.gpu_workers) if self.gpu_workers else max(3 if self.batch_size <= 8 else 2, self.num_processes)
        depth = max(2, 2 * workers)
        procs = self._io_processes()
        if procs is not None:
            # one I/O thread per worker process (a thread only relays: request, blocking reply); decode and encode have
            # their own executors so that a burst of reads can never starve the writes a batch needs to finish
            procs.begin()
            io = ThreadPoolExecutor(max_workers=procs.readers, thread_name_prefix="fcp-read")
            wio = ThreadPoolExecutor(max_workers=procs.writers, thread_name_prefix="fcp-write")
            read_one = None
        else:
            io = wio = ThreadPoolExecutor(max_workers=self.io_threads, thread_name_prefix="fcp-io")
            read_one = lambda path: (read_image(path), None)
        self._io_procs_active = procs
        writes = []
        self._io = (wio, writes, BoundedSemaphore(self.MAX_PENDING_WRITES))
        # Threads: every file is its own decode task (a batch decoded by one thread would cap the pipeline at `depth`
        # decoders).  Worker processes: a batch is dealt round-robin into one request per decoder — the parent's relay
        # threads wake up once per request, not once per image (their wake-ups contend for the interpreter lock).
        def submit_read(i):
            paths = [os.path.join(input_dir, f) for f in file_batches[i]]
            if procs is None:
                return [io.submit(read_one, p_) for p_ in paths]
            k = min(procs.readers, len(paths))
            return [(paths[j::k], io.submit(procs.read_many, paths[j::k])) for j in range(k)]

        def collect_read(i, futs):
            """-> images, surviving names, release tokens of the shared-memory regions the images live in."""
            if procs is None:
                decoded = [f.result() for f in futs]
            else:                                    # undo the round-robin deal: image m of the batch is item m // k of chunk m % k
                chunks = [f.result() for _, f in futs]
                decoded = [chunks[m % len(chunks)][m // len(chunks)] for m in range(len(file_batches[i]))]
            ok = [k for k, (im, _) in enumerate(decoded) if im is not None]
            return [decoded[k][0] for k in ok], np.array(file_batches[i])[ok], [decoded[k][1] for k in ok]

        reads = {i: submit_read(i) for i in range(min(depth, len(file_batches)))}
        lock = Lock()

        tls = local()

        def worker(i):
            futs = reads.pop(i, None)
            with lock:
                nxt = i + depth
                if nxt < len(file_batches) and nxt not in reads:
                    reads[nxt] = submit_read(nxt)
            images, names, tokens = collect_read(i, futs) if futs is not None else (*read_images(file_batches[i], input_dir), [])
            pinned = procs.pinned_flags(tokens) if procs is not None and tokens else None   # images in page-locked rings
            try:
                if workers == 1:
                    return self._process_images(images, names, output_dir, pinned)
                # one HIP stream per GPU worker: the batches of different workers overlap on the device (the tail of
                # one kernel with the head of another; measured +4 % at two streams) instead of queueing on stream 0
                if not hasattr(tls, "stream"):
                    from . import engine as E
                    with torch.cuda.device(self.device):
                        tls.stream = E.thread_main_stream(self.device)           # the same streams again in every run
                        tls.stream.wait_stream(torch.cuda.default_stream())      # filters were uploaded there
                with torch.cuda.device(self.device), torch.cuda.stream(tls.stream):
                    self._process_images(images, names, output_dir, pinned)
                    tls.stream.synchronize()
            finally:
                # every use of the decoded images is over — the uploads out of the rings were enqueued before kernels whose
                # results _process_images has read back (a stream synchronisation), the no-alignment path copied what it
                # hands to the asynchronous writers — so their ring regions go back to the decode workers
                del images
                if procs is not None:
                    procs.release(tokens)

        failed = True
        try:
            with ThreadPool(workers) as pool:
                imap = pool.imap(worker, range(len(file_batches)))
                if desc is not None:
                    try:
                        import tqdm
                        imap = tqdm.tqdm(imap, total=len(file_batches), desc=desc)
                    except ImportError:
                        pass
                list(imap)
            for w in writes:
                w.result()                       # surface encode / write errors
            failed = False
        finally:
            io.shutdown(wait=True)       # in-flight tasks still hold the semaphore / list: reset only afterwards
            if wio is not io:
                wio.shutdown(wait=True)
            self._io = None
            self._io_procs_active = None
            # A run that failed may have left a dead worker, a request cut off in the middle (its ring space handed out but
            # never reported) or prefetched batches nobody collected: that pool is not reused — the next run starts fresh
            # workers instead of inheriting the damage.
            if procs is not None and (failed or not procs.healthy()):
                procs.close()
                if self._io_procs is procs:
                    self._io_procs = None

    @staticmethod
    def _pin_ring(ring, nbytes) -> bool:
        """Page-lock (nbytes > 0) / unlock (0) a decode ring for HIP, so that ``build_batch`` uploads images straight from
        the ring instead of through a host copy into its staging blob (14 of 40 ms per batch of 64 at 640^2)."""
        addr = np.frombuffer(ring, dtype=np.uint8).ctypes.data
        rt = torch.cuda.cudart()
        try:
            if nbytes:
                err = rt.cudaHostRegister(addr, nbytes, 0)
                ok = int(err) == 0
                return ok and torch.from_numpy(np.frombuffer(ring, dtype=np.uint8, count=64)).is_pinned()
            rt.cudaHostUnregister(addr)
        except Exception:                            # noqa: BLE001 - a runtime without host registration: staging still works
            pass
        return False

    @staticmethod
    def default_io_processes(cores: int, local_world: int = 1):
        """(decode, encode) worker processes of one ``Cropper`` on a host with ``cores`` usable cores shared by
        ``local_world`` ranks (one process per GPU: the ranks of a node share the host).  Measured on a 2 x 64-core EPYC
        9575F box (2048 JPEGs of 640^2, one decode request per decoder and batch; 2 / 3 GPU workers): (8, 3) 2320 / 2650,
        (12, 3) 2360 / 2750, (12, 4) 2300 / 2540, (16, 4) 2270 / 2600, (24, 4) 2110 / 2650 images/s — flat beyond a dozen
        decoders (one decodes ~600 images/s).  8 ranks on that box: 16 cores each -> (5, 2), i.e. 40 + 16 I/O processes,
        8 x (1 + num_processes) Python threads that enqueue, and 3000 decodes/s per rank against ~3500 faces/s of device
        rate."""
        cores = max(1, cores // max(1, local_world))
        return (max(2, min(12, cores // 3)), max(1, min(3, cores // 8)))

    def _io_processes(self):
        """The decode / encode worker processes of this Cropper (started on first use, reused by later runs), or None
        when they are switched off or cannot be had on this platform."""
        want = self.io_processes
        if want is None:
            cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 4)
            want = self.default_io_processes(cores, int(os.environ.get("LOCAL_WORLD_SIZE", "1")))
        if min(want) <= 0:
            return None
        have = self._io_procs
        if have is not None and have.healthy() and (have.readers, have.writers) == tuple(want):
            return have
        if have is not None:
            have.close()
        try:
            from ._io_pool import IOProcesses
            kw = {} if self.io_ring_mb is None else {"ring_mb": int(self.io_ring_mb)}
            self._io_procs = IOProcesses(*want, register=self._pin_ring if os.environ.get("FCP_IO_PIN", "1") != "0" else None, **kw)
        except (ValueError, OSError) as e:           # no memfd / no processes left on this host: threads still work
            import warnings
            warnings.warn(f"decode / encode worker processes unavailable ({e}): using I/O threads")
            self.io_processes, self._io_procs = (0, 0), None
        return self._io_procs
