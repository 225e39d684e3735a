"""JPEG files of device-resident crops (``Cropper(encoder="device")``): the kernels of
``csrc/fcp_jpeg.hip`` write every face's entropy-coded segment, the host puts the header in front.  The result is byte for
byte the file ``_io_codec.write_image`` (Pillow over libjpeg-turbo) writes for the same pixels, so a face whose stream does
not fit its slot is simply encoded there instead.  Quality, chroma subsampling and per-file ("optimised") Huffman tables
are the caller's (section 2j); the defaults are the encoder table's and take the entry point they always took."""
from __future__ import annotations

import io

import numpy as np
import torch

from . import _native as N
from . import torch_ops as T
from ._io_codec import _ENCODER_KW, JPEG_SUBSAMPLINGS, JpegSettings, jpeg_kw, read_slots, save_jpeg

JPEG_EXTENSIONS = tuple(ext for ext, kw in _ENCODER_KW.items() if kw.get("format") == "JPEG")     # .jpg / .jpeg / .jpe
_KW = _ENCODER_KW[".jpg"]
QUALITY = _KW["quality"]
SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}[_KW["subsampling"]]

_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
           62, 63)
# ITU-T T.81 Annex K.1 (quantisation, natural order) and K.3 (Huffman: codes per length 1..16, symbols in code order)
_QUANT = ((16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
           80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
           95, 98, 112, 100, 103, 99),
          (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
           99, 99) + (99,) * 32)
_DC = (((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
       ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))))
_AC = (((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
        (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209,
         240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69,
         70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119,
         120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164,
         165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201,
         202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243,
         244, 245, 246, 247, 248, 249, 250)),
       ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
        (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82,
         240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68,
         69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119,
         120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
         164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200,
         201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244,
         245, 246, 247, 248, 249, 250)))


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + payload


TABLE_BYTES = 272                # one Huffman table of the device encoder: 16 counts + up to 256 symbols, zero padded


def subsampling_index(subsampling) -> int:
    """"4:4:4" / "4:2:2" / "4:2:0" (or 0 / 1 / 2 already) -> the `subsampling` argument of the C entry points."""
    if isinstance(subsampling, str):
        if subsampling not in JPEG_SUBSAMPLINGS:
            raise ValueError(f"unknown subsampling {subsampling!r}: choose '4:4:4', '4:2:2' or '4:2:0'")
        return JPEG_SUBSAMPLINGS.index(subsampling)
    if isinstance(subsampling, bool) or int(subsampling) not in (0, 1, 2):
        raise ValueError(f"subsampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), not {subsampling!r}")
    return int(subsampling)


def _dht_payloads(tables, sets: int):
    """`tables`: None (the standard tables) or one face's four 272-byte records -> [(DC payload, AC payload)] per set."""
    if tables is None:
        return [(bytes(_DC[k][0]) + bytes(_DC[k][1]), bytes(_AC[k][0]) + bytes(_AC[k][1])) for k in range(sets)]
    rec = np.frombuffer(bytes(tables), np.uint8) if isinstance(tables, (bytes, bytearray)) else np.asarray(tables, np.uint8)
    rec = rec.reshape(4, TABLE_BYTES)
    out = []
    for k in range(sets):
        pair = []
        for r in rec[2 * k:2 * k + 2]:
            n = int(r[:16].sum())
            if n > 256:
                raise ValueError("a Huffman table record lists more than 256 symbols")
            pair.append(r[:16 + n].tobytes())
        out.append(tuple(pair))
    return out


def jpeg_header(h: int, w: int, channels: int, quality: int = QUALITY, *, subsampling=SUBSAMPLING, tables=None) -> bytes:
    """Everything of the file in front of the entropy-coded segment, as Pillow / libjpeg write it at these settings: SOI,
    the JFIF 1.01 APP0 segment (no density unit, 1:1), one DQT per table (IJG quality scale, baseline range), SOF0 (8 bit;
    luma sampled 1x1, 2x1 or 2x2 for 4:4:4, 4:2:2, 4:2:0 — written for gray too, where it changes nothing but that
    byte), the Huffman tables, SOS.  ``tables``: None for the standard tables, or the face's four 272-byte records as
    the device encoder wrote them (Y DC, Y AC, chroma DC, chroma AC): optimised tables sit where the standard ones do."""
    if channels not in (1, 3):
        raise ValueError(f"channels must be 1 or 3, not {channels!r}")
    if not (1 <= int(quality) <= 100):
        raise ValueError(f"quality must be in 1..100, not {quality!r}")
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"a JPEG frame is 1..65535 px on each side, not {h} x {w}")
    ss = subsampling_index(subsampling)
    sets = 1 if channels == 1 else 2
    scale = 5000 // int(quality) if quality < 50 else 200 - 2 * int(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for k in range(sets):
        table = [min(max((_QUANT[k][i] * scale + 50) // 100, 1), 255) for i in _ZIGZAG]
        out += _segment(0xDB, bytes([k]) + bytes(table))
    comps = [(1, (0x11, 0x21, 0x22)[ss], 0), (2, 0x11, 1), (3, 0x11, 1)][:channels]
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([channels]) +
                    b"".join(bytes(c) for c in comps))
    for k, (dc, ac) in enumerate(_dht_payloads(tables, sets)):
        out += _segment(0xC4, bytes([k]) + dc)
        out += _segment(0xC4, bytes([0x10 | k]) + ac)
    return out + _segment(0xDA, bytes([channels]) + b"".join(bytes([c[0], 0x11 * c[2]]) for c in comps) + b"\x00\x3f\x00")


def encode_scans(crops_dev: torch.Tensor, out: torch.Tensor, quality: int = QUALITY, *, subsampling=SUBSAMPLING,
                 tables: torch.Tensor | None = None) -> torch.Tensor:
    """crops (F,H,W,3) or (F,H,W) u8 device, out (F, capacity) u8 device (rows may be a view of a wider buffer) -> lengths
    (F,) int32 device.  Row i receives face i's entropy-coded segment and EOI, at most ``capacity`` bytes of it; the length
    is the true one even then.  One memset and four launches.
    ``tables`` (F,4,272) u8 device, contiguous: code every face with Huffman tables made for it (libjpeg's
    ``optimize_coding``); the four records of face i are written to tables[i] (a histogram and a table launch more).
    With 4:2:0 and no ``tables`` this is the call it always was; anything else takes ``fcp_jpeg_encode_ex_u8``."""
    ss = subsampling_index(subsampling)
    if tables is not None:
        assert tables.dtype == torch.uint8 and tables.is_contiguous() and tables.device == crops_dev.device
        assert tuple(tables.shape) == (crops_dev.shape[0], 4, TABLE_BYTES)
    q, opt = int(quality), 0 if tables is None else 1
    if ss != SUBSAMPLING or opt:
        return N.encode_slots(
            "jpeg_encode", "fcp_jpeg_encode_ex_u8", crops_dev, out,
            (lambda: T.load().jpeg_encode_ex(crops_dev, q, ss, out, tables)) if T.ENABLED else None,
            lambda *size: N.lib().fcp_jpeg_workspace_bytes_ex(*size, ss, opt),
            lambda size, slots, work: N.lib().fcp_jpeg_encode_ex_u8(N.ptr(crops_dev), *size, q, ss, opt, *slots, N.ptr(tables),
                                                                    *work))
    return N.encode_slots(
        "jpeg_encode", "fcp_jpeg_encode_u8", crops_dev, out,
        (lambda: T.load().jpeg_encode(crops_dev, q, SUBSAMPLING, out)) if T.ENABLED else None,
        lambda *size: N.lib().fcp_jpeg_workspace_bytes(*size),
        lambda size, slots, work: N.lib().fcp_jpeg_encode_u8(N.ptr(crops_dev), *size, q, SUBSAMPLING, *slots, *work))


def huffman_tables(freq: torch.Tensor, with_codes: bool = False):
    """freq (N,256) uint32-valued int32 device rows of symbol counts (each row's sum below 9 227 464) -> the optimal
    tables libjpeg's ``jpeg_gen_optimal_table`` makes of them, as records (N,272) u8 device; with ``with_codes`` also
    (N,256) int32 ``code | length << 16`` by symbol.  An all-zero row gives an all-zero record.  One launch."""
    assert freq.dtype == torch.int32 and freq.is_contiguous() and freq.dim() == 2 and freq.shape[1] == 256
    if T.ENABLED:
        tables, codes = T.load().jpeg_huffman_tables(freq, bool(with_codes))
        return (tables, codes) if with_codes else tables
    n = freq.shape[0]
    tables = torch.empty((n, TABLE_BYTES), dtype=torch.uint8, device=freq.device)
    codes = torch.empty((n, 256), dtype=torch.int32, device=freq.device) if with_codes else None
    N.check(N.lib().fcp_jpeg_huffman_tables(N.ptr(freq), n, N.ptr(tables), N.ptr(codes), N.stream_ptr()),
            "fcp_jpeg_huffman_tables")
    return (tables, codes) if with_codes else tables


def _host_jpeg(pixels: np.ndarray, quality: int, subsampling=SUBSAMPLING, optimize: bool = False) -> bytes:
    buf = io.BytesIO()
    save_jpeg(pixels, buf, jpeg_kw(JpegSettings(int(quality), JPEG_SUBSAMPLINGS[subsampling_index(subsampling)], bool(optimize))))
    return buf.getvalue()


def encode_jpeg(crops_dev: torch.Tensor, quality: int = QUALITY, capacity: int | None = None, *, subsampling=SUBSAMPLING,
                optimize: bool = False) -> list:
    """crops (F,H,W,3) or (F,H,W) u8 device -> F complete JPEG files (bytes), each equal to what ``write_image`` writes for
    those pixels at these settings.  ``capacity``: bytes of a face's slot on the device (default: the raw size of a face,
    H*W*C); what comes back to the host is the lengths, the used part of the slots and, with ``optimize``, the faces'
    Huffman tables (1088 bytes each) — not the pixels.  A face whose stream is longer than its slot (noise can be: a
    block costs up to 417 bytes) is read back alone and encoded on the host: same bytes."""
    f, h, w = crops_dev.shape[:3]
    c = crops_dev.shape[3] if crops_dev.dim() == 4 else 1
    if f == 0:
        return []
    ss = subsampling_index(subsampling)
    capacity = h * w * c if capacity is None else int(capacity)
    out = torch.empty((f, capacity), dtype=torch.uint8, device=crops_dev.device)
    tables = torch.empty((f, 4, TABLE_BYTES), dtype=torch.uint8, device=crops_dev.device) if optimize else None
    lengths = encode_scans(crops_dev, out, quality, subsampling=ss, tables=tables)
    records = tables.cpu().numpy() if optimize else None
    head = None if optimize else jpeg_header(h, w, c, quality, subsampling=ss)

    def on_host(i):
        px = crops_dev[i].cpu().numpy()
        return _host_jpeg(px[..., 0] if px.ndim == 3 and c == 1 else px, quality, ss, optimize)
    return read_slots(out, lengths, lambda i, scan: (jpeg_header(h, w, c, quality, subsampling=ss, tables=records[i])
                                                    if optimize else head) + scan, on_host)
