"""File decode / encode of the host pipeline (Pillow), free of torch imports: the worker processes of ``_io_pool.py``
import only this module.  ``utils.py`` re-exports ``read_image`` / ``write_image`` (reference ``utils.py:228-271``,
``cropper.py:605-609``)."""
from __future__ import annotations

import os
import threading
import warnings
from typing import NamedTuple

import numpy as np


def read_image(path: str):
    """One file -> RGB uint8 HWC array, or None (with the reference's warning) when it cannot be read.
    Like ``cv2.imread`` (utils.py:262), the EXIF orientation tag is applied: phone photos arrive upright, and
    user-supplied landmark files — which live in that oriented frame — point at the right pixels."""
    from PIL import Image, ImageOps
    try:
        with Image.open(path) as im:
            im = ImageOps.exif_transpose(im)
            return np.asarray(im.convert("RGB"), dtype=np.uint8)
    except Exception:
        warnings.warn(f"Could not read the image {path}")
        return None


# Encoder settings of ``cv2.imwrite`` with no parameters (cropper.py:605-609), so that files written here have the
# fidelity and roughly the size of the reference's: JPEG quality 95 with 4:2:0 chroma subsampling (Pillow's own
# default, quality 75, is visibly lossier), PNG at zlib level 1 (lossless either way: only size / speed differ),
# WebP lossless (OpenCV's default quality setting means lossless).
_ENCODER_KW = {
    ".jpg": dict(format="JPEG", quality=95, subsampling="4:2:0"),
    ".jpeg": dict(format="JPEG", quality=95, subsampling="4:2:0"),
    ".jpe": dict(format="JPEG", quality=95, subsampling="4:2:0"),
    ".png": dict(format="PNG", compress_level=1),
    ".webp": dict(format="WEBP", lossless=True),
    ".bmp": dict(format="BMP"),
    ".tif": dict(format="TIFF"),
    ".tiff": dict(format="TIFF"),
}


_NOT_CV2_FORMATS = {"GIF", "PDF", "ICO", "ICNS", "PALM", "MPO", "XBM", "IM", "MSP", "PCX", "DDS", "TGA", "SGI", "EPS", "SPIDER",
                    "BLP", "BUFR", "GRIB", "HDF5", "DIB", "APNG"}   # Pillow writes them, cv2.imwrite refuses: skipped like there


JPEG_SUBSAMPLINGS = ("4:4:4", "4:2:2", "4:2:0")     # index = the `subsampling` argument of the device encoder


class JpegSettings(NamedTuple):
    """``Cropper(jpeg_quality=, jpeg_subsampling=, jpeg_optimize=)`` as it travels to the writers (picklable)."""
    quality: int = 95
    subsampling: str = "4:2:0"
    optimize: bool = False


def check_jpeg_settings(quality, subsampling, optimize) -> JpegSettings:
    """The three settings, validated: an int 1..100 (no bool, no float), one of the three strings, a bool."""
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not (1 <= int(quality) <= 100):
        raise ValueError(f"jpeg_quality must be an int in 1..100, not {quality!r}")
    if not isinstance(subsampling, str) or subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError(f"unknown jpeg_subsampling {subsampling!r}: choose '4:4:4', '4:2:2' or '4:2:0'")
    if not isinstance(optimize, (bool, np.bool_)):
        raise ValueError(f"jpeg_optimize must be True or False, not {optimize!r}")
    return JpegSettings(int(quality), subsampling, bool(optimize))


_MAXBLOCK_LOCK = threading.Lock()


def jpeg_worst_case_bytes(h: int, w: int) -> int:
    """No JPEG file of an h x w image written here is longer: a block costs at most 27 + 63 * 26 = 1665 bits, 417 bytes
    after FF -> FF 00 stuffing; there are at most 12 blocks per 16 x 16 pixels (4:4:4, or 4:2:0's MCUs with their dummy
    blocks, rounded up to whole MCUs); the header with four full Huffman tables stays below 2048 bytes."""
    return 2048 + 417 * 12 * ((h + 15) // 16) * ((w + 15) // 16)


def save_jpeg(image: np.ndarray, target, kw: dict):
    """``Image.fromarray(image).save(target, **kw)`` for a JPEG.  With ``optimize`` libjpeg writes the whole file into
    ONE buffer, which Pillow sizes at w * h bytes (2 w h from quality 95) or ``ImageFile.MAXBLOCK``, whichever is larger;
    a file longer than that (noise at 4:4:4 is) fails with "broken data stream" (libjpeg: "Suspension not allowed
    here").  So MAXBLOCK is raised to the worst case of this image for the duration of the save, and restored."""
    from PIL import Image, ImageFile
    im = Image.fromarray(image)
    if not kw.get("optimize"):
        im.save(target, **kw)
        return
    with _MAXBLOCK_LOCK:                             # the I/O threads of the inline path share the module attribute
        old = ImageFile.MAXBLOCK
        ImageFile.MAXBLOCK = max(old, jpeg_worst_case_bytes(image.shape[0], image.shape[1]))
        try:
            im.save(target, **kw)
        finally:
            ImageFile.MAXBLOCK = old


def jpeg_kw(jpeg: JpegSettings | None = None, ext: str = ".jpg") -> dict:
    """Pillow's keywords of a JPEG file: the table entry, overridden by ``jpeg``."""
    kw = _ENCODER_KW[ext]
    if jpeg is None:
        return kw
    quality, subsampling, optimize = jpeg
    return dict(kw, quality=int(quality), subsampling=subsampling, optimize=bool(optimize))


def write_image(path: str, image: np.ndarray, jpeg: JpegSettings | None = None) -> bool:
    """RGB (or single-channel mask) uint8 array -> file; format from the extension, ``cv2.imwrite`` defaults for the
    formats listed above, Pillow's own choice of encoder for every other extension it knows (.ppm / .pgm / .pnm /
    .jp2 / ... — ``cv2.imwrite`` writes these too).  Only an extension NO encoder exists for warns and returns False
    (the file is skipped) instead of raising.  ``jpeg`` (quality, subsampling, optimize) overrides the table entry of
    the three JPEG extensions and touches no other format."""
    from PIL import Image
    ext = os.path.splitext(path)[1].lower()
    kw = _ENCODER_KW.get(ext)
    if kw is not None:
        if jpeg is not None and kw.get("format") == "JPEG":
            save_jpeg(image, path, jpeg_kw(jpeg, ext))
        else:
            Image.fromarray(image).save(path, **kw)
        return True
    ext = os.path.splitext(path)[1].lower()
    Image.init()                                    # fill Pillow's extension -> encoder registry
    fmt = Image.registered_extensions().get(ext)
    if fmt is None or fmt.upper() not in Image.SAVE or fmt.upper() in _NOT_CV2_FORMATS:
        # no encoder for this extension (here or in cv2.imwrite): the reference's writer returns False and goes on
        warnings.warn(f"Could not write the image {path}: no encoder for the extension {ext!r}")
        return False
    # real I/O errors (disk full, permissions, a missing directory) propagate, like everywhere else in the writer; the
    # file goes to a temporary name first so that a failed write never leaves a truncated image behind
    tmp = f"{path}.part{os.getpid()}"
    try:
        Image.fromarray(image).save(tmp, format=fmt)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return True


def read_slots(out, lengths, fitted, overflowed) -> list:
    """The way back from the device encoders: out (F, capacity) u8 device slots and lengths (F,) int32 device, as
    ``encode_scans`` / ``encode_streams`` left them -> one entry per face, ``fitted(i, stream bytes)`` where the stream fits
    its slot and ``overflowed(i)`` where it does not.  What comes to the host is the lengths and, in one read, the part of
    the slots that is used."""
    lengths = lengths.cpu().numpy()
    fits = lengths <= out.shape[1]
    used = int(lengths[fits].max()) if fits.any() else 0
    slots = out[:, :used].cpu().numpy() if used else None
    return [fitted(i, slots[i, :lengths[i]].tobytes()) if fits[i] else overflowed(i) for i in range(len(lengths))]


def write_bytes(path: str, data) -> bool:
    """An already encoded file (``Cropper(encoder="device")``: header + the stream the GPU wrote) -> disk, through a
    temporary name so that a failed write never leaves a truncated image behind."""
    tmp = f"{path}.part{os.getpid()}"
    try:
        with open(tmp, "wb") as fh:
            fh.write(data)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return True
