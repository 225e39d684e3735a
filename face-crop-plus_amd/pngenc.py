"""PNG files of device-resident faces (``Cropper(png_encoder="device")``): the kernels of
``csrc/fcp_png.hip`` filter every face and write its zlib stream, the host puts the PNG chunks around it.  The files
decode to exactly the pixels the host's PNG files decode to; they are NOT the host's bytes (a deflate stream has many valid
encodings, and this one is not zlib's).  A face whose stream does not fit its slot, or whose size the kernels refuse, is
encoded on the host with ``write_image``'s PNG settings instead."""
from __future__ import annotations

import io
import struct
import zlib

import numpy as np
import torch

from . import _native as N
from . import torch_ops as T
from ._io_codec import _ENCODER_KW, read_slots

PNG_EXTENSIONS = tuple(ext for ext, kw in _ENCODER_KW.items() if kw.get("format") == "PNG")     # .png
SYMBOLS = 286                    # literal/length symbols of deflate
MAX_SIDE = 8192
MAX_SYMBOLS = 9227464            # h * (w * c + 1) + 1 stays below it: no Huffman tree deeper than 32 (fcp_hip.h)


def supported(h: int, w: int, c: int) -> bool:
    """Whether the device encoder takes faces of this size (``fcp_png_encode_u8`` refuses the others with a message)."""
    return 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and c in (1, 3) and h * (w * c + 1) + 1 < MAX_SYMBOLS


def supported_rgba(h: int, w: int) -> bool:
    """``supported`` for RGBA faces (F,H,W,4): the same limits at c = 4, h * (4 w + 1) + 1 < 9227464, so 1500 x 1500 fits
    and 1520 x 1520 does not.  (``supported`` keeps answering for gray and RGB alone.)"""
    return 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and h * (w * 4 + 1) + 1 < MAX_SYMBOLS


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def _file(h: int, w: int, colour_type: int, stream: bytes) -> bytes:
    if not (1 <= h < 2 ** 31 and 1 <= w < 2 ** 31):
        raise ValueError(f"a PNG image is 1..2^31-1 px on each side, not {h} x {w}")
    ihdr = struct.pack(">IIBBBBB", w, h, 8, colour_type, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", bytes(stream)) + _chunk(b"IEND", b"")


def png_file(h: int, w: int, c: int, stream: bytes) -> bytes:
    """The file around one zlib stream of filtered scanlines: signature, IHDR (8 bit; colour type 0 for c = 1, 2 for
    c = 3; no interlace), one IDAT, IEND.  The chunk CRC-32 is zlib's, on the host, over bytes that are already here."""
    if c not in (1, 3):
        raise ValueError(f"channels must be 1 or 3, not {c!r}")
    return _file(h, w, 0 if c == 1 else 2, stream)


def png_file_rgba(h: int, w: int, stream: bytes) -> bytes:
    """``png_file`` around the zlib stream of RGBA scanlines: IHDR colour type 6 (8 bit, no interlace)."""
    return _file(h, w, 6, stream)


def encode_streams(pixels_dev: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """pixels (F,H,W,3), (F,H,W,4) or (F,H,W) u8 device, out (F, capacity) u8 device (rows may be a view of a wider buffer) ->
    lengths (F,) int32 device.  Row i receives face i's zlib stream, at most ``capacity`` bytes of it; the length is the
    true one even then.  One memset and six launches."""
    return N.encode_slots("png_encode", "fcp_png_encode_u8", pixels_dev, out,
                          (lambda: T.load().png_encode(pixels_dev, out)) if T.ENABLED else None,
                          lambda *size: N.lib().fcp_png_workspace_bytes(*size),
                          lambda size, slots, work: N.lib().fcp_png_encode_u8(N.ptr(pixels_dev), *size, *slots, *work))


def huffman_lengths(freq: torch.Tensor, with_codes: bool = False):
    """freq (N,286) uint32-valued int32 device rows of literal/length counts (each row's sum below 2^32) -> the
    code lengths (N,286) u8 device the encoder gives them (at most 15 bits); with ``with_codes`` also (N,286) int32
    ``bit-reversed code | length << 16`` by symbol.  A row with fewer than two non-zero counts gives zeros.  One launch."""
    assert freq.dtype == torch.int32 and freq.is_contiguous() and freq.dim() == 2 and freq.shape[1] == SYMBOLS
    if T.ENABLED:
        lengths, codes = T.load().png_huffman_lengths(freq, bool(with_codes))
        return (lengths, codes) if with_codes else lengths
    n = freq.shape[0]
    lengths = torch.empty((n, SYMBOLS), dtype=torch.uint8, device=freq.device)
    codes = torch.empty((n, SYMBOLS), dtype=torch.int32, device=freq.device) if with_codes else None
    N.check(N.lib().fcp_png_huffman_lengths(N.ptr(freq), n, N.ptr(lengths), N.ptr(codes), N.stream_ptr()),
            "fcp_png_huffman_lengths")
    return (lengths, codes) if with_codes else lengths


def _host_png(pixels: np.ndarray) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, **_ENCODER_KW[".png"])
    return buf.getvalue()


def encode_png(pixels_dev: torch.Tensor, capacity: int | None = None) -> list:
    """pixels (F,H,W,3), (F,H,W,4) (RGBA: colour type 6) or (F,H,W) u8 device -> F complete PNG files (bytes) that decode
    to those pixels.
    ``capacity``: bytes of a face's slot on the device (default: H * (W * C + 1) + 1024, which no stream whose codes
    average 9 bits or less outgrows); what comes back to the host is the lengths and the used part of the slots — not
    the pixels.  A face whose stream is longer than its slot is read back alone and encoded on the host with
    ``write_image``'s PNG settings, and so is every face of a size the kernels refuse."""
    f, h, w = pixels_dev.shape[:3]
    c = pixels_dev.shape[3] if pixels_dev.dim() == 4 else 1
    if f == 0:
        return []

    def on_host(i):
        px = pixels_dev[i].cpu().numpy()
        return _host_png(px[..., 0] if px.ndim == 3 and c == 1 else px)
    if not (supported_rgba(h, w) if c == 4 else supported(h, w, c)):
        return [on_host(i) for i in range(f)]
    capacity = h * (w * c + 1) + 1024 if capacity is None else int(capacity)
    out = torch.empty((f, capacity), dtype=torch.uint8, device=pixels_dev.device)
    wrap = (lambda i, data: png_file_rgba(h, w, data)) if c == 4 else (lambda i, data: png_file(h, w, c, data))
    return read_slots(out, encode_streams(pixels_dev, out), wrap, on_host)
