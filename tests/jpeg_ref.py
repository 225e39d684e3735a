"""Baseline JPEG encoder restated in numpy / Python integers: the reference of tests/test_jpeg_cpu.py and test_jpeg_gpu.py.

Written from ITU-T T.81 (frame / scan syntax, Annex K tables, Annex F Huffman procedures) and the documented arithmetic of
the IJG library's default compressor, which libjpeg-turbo keeps bit for bit: 16-bit scaled RGB -> YCbCr, edge
replication, 2x2 chroma averaging with the alternating 1, 2 bias, the 13-bit "islow" forward DCT whose output is scaled
by 8, and division by 8*Q rounding half away from zero.  Two stages are exposed: ``coefficients`` (quantised blocks per
component, natural order) and ``encode`` / ``encode_scan`` (the bytes).  ``Image.fromarray(a).save(buf, "JPEG",
quality=q, subsampling="4:2:0")`` is what it has to equal, byte for byte (test_jpeg_cpu.py)."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])

# T.81 Annex K.1: luminance and chrominance quantisation tables (natural order), the ones quality 50 stands for
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

# T.81 Annex K.3: the typical Huffman tables, as (codes per length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82,
            209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67,
            68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117,
            118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162,
            163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199,
            200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241,
            242, 243, 244, 245, 246, 247, 248, 249, 250])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35,
              51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56,
              57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106,
              115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150,
              151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186,
              194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229,
              230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])


def quant_tables(quality: int):
    """The IJG quality scale: 5000 / q below 50, 200 - 2 q from 50 on, entries clamped to 1..255 (baseline)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [np.clip((t * scale + 50) // 100, 1, 255) for t in (Q_LUMA, Q_CHROMA)]


def huffman_codes(table):
    """T.81 Annex C: symbol -> (code, length)."""
    counts, symbols = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(h: int, w: int, channels: int, quality: int) -> bytes:
    """SOI, JFIF 1.01 APP0 (no units, 1:1), one DQT and two DHT segments per table set, SOF0, SOS."""
    assert channels in (1, 3)
    qt = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for k in range(1 if channels == 1 else 2):
        out += _segment(0xDB, bytes([k]) + bytes(int(v) for v in qt[k][ZIGZAG]))
    # the 2x2 sampling factors are written for a lone gray component too (they change nothing there: its scan is not
    # interleaved, so its MCU is one block)
    comps = [(1, 0x22, 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if channels == 3 else [])
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([channels]) +
                    b"".join(bytes(c) for c in comps))
    for k, (dc, ac) in enumerate([(DC_LUMA, AC_LUMA), (DC_CHROMA, AC_CHROMA)][:1 if channels == 1 else 2]):
        out += _segment(0xC4, bytes([k]) + bytes(dc[0]) + bytes(dc[1]))
        out += _segment(0xC4, bytes([0x10 | k]) + bytes(ac[0]) + bytes(ac[1]))
    out += _segment(0xDA, bytes([channels]) + b"".join(bytes([c[0], 0x11 * c[2]]) for c in comps) + b"\x00\x3f\x00")
    return out


# ---------------------------------------------------------------- samples
def _cdiv(a, b):
    return -(-a // b)


def component_planes(img: np.ndarray):
    """uint8 (h,w) or (h,w,3) -> component sample planes, each padded to whole 8x8 blocks of ITS OWN block grid
    (ceil(samples / 8) blocks): Y (or gray) by repeating the last column and row; Cb / Cr from the full-resolution plane
    whose right edge is repeated, averaged 2x2 with bias 1 in even and 2 in odd output columns, a missing odd last row
    being the row above it again, and the averaged rows then repeated downwards."""
    img = np.asarray(img)
    h, w = img.shape[:2]
    if img.ndim == 2:
        full = [img.astype(np.int64)]
    else:
        r, g, b = (img[..., k].astype(np.int64) for k in range(3))
        full = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16]
    bw, bh = _cdiv(w, 8), _cdiv(h, 8)
    ys, xs = np.minimum(np.arange(8 * bh), h - 1), np.minimum(np.arange(8 * bw), w - 1)
    planes = [full[0][ys][:, xs]]
    if img.ndim == 3:
        cw, ch = _cdiv(_cdiv(w, 2), 8), _cdiv(_cdiv(h, 2), 8)
        rows = np.minimum(np.arange(8 * ch), _cdiv(h, 2) - 1)
        y0, y1 = 2 * rows, np.minimum(2 * rows + 1, h - 1)
        x0, x1 = np.minimum(2 * np.arange(8 * cw), w - 1), np.minimum(2 * np.arange(8 * cw) + 1, w - 1)
        bias = 1 + (np.arange(8 * cw) & 1)
        for p in full[1:]:
            planes.append((p[y0][:, x0] + p[y0][:, x1] + p[y1][:, x0] + p[y1][:, x1] + bias) >> 2)
    return planes


# ---------------------------------------------------------------- DCT + quantisation
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_pass(d, first: bool):
    """One pass of the islow DCT over the LAST axis of d (..., 8), int64.  The first pass leaves its output scaled up by
    4, the second removes that again; both keep the DCT's own factor of sqrt(8) per pass."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = _descale(z1 + t13 * 6270, n)
    out[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, -1)


def coefficients(img: np.ndarray, quality: int = 95):
    """-> per component an int array (block rows, block columns, 64) of quantised coefficients in natural order, for the
    blocks that hold samples (the dummy blocks an odd block grid adds to its last MCUs are not among them)."""
    qt = quant_tables(quality)
    out = []
    for k, plane in enumerate(component_planes(img)):
        bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
        blocks = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128            # (bh, bw, row, column)
        rows = _dct_pass(blocks, True)
        both = _dct_pass(rows.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)
        div = (8 * qt[min(k, 1)]).reshape(8, 8)
        mag = (np.abs(both) + div // 2) // div
        out.append((np.sign(both) * mag).reshape(bh, bw, 64))
    return out


# ---------------------------------------------------------------- entropy coding
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code: int, length: int):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def finish(self) -> bytes:
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out)


def scan_blocks(coefs):
    """MCU order: [(component, quantised block (64,) natural order, or None for a dummy block)].  One component: its
    blocks row by row.  Three: MCUs of 2x2 Y blocks, Cb, Cr; a Y position past the block grid is a dummy block."""
    if len(coefs) == 1:
        return [(0, b) for row in coefs[0] for b in row]
    ybh, ybw = coefs[0].shape[:2]
    out = []
    for my in range(coefs[1].shape[0]):
        for mx in range(coefs[1].shape[1]):
            for dy in range(2):
                for dx in range(2):
                    y, x = 2 * my + dy, 2 * mx + dx
                    out.append((0, coefs[0][y, x] if y < ybh and x < ybw else None))
            out.append((1, coefs[1][my, mx]))
            out.append((2, coefs[2][my, mx]))
    return out


def encode_scan(img: np.ndarray, quality: int = 95, stats: dict | None = None) -> bytes:
    """Entropy-coded segment + EOI.  ``stats`` (optional) counts the ZRL and EOB symbols and the stuffed bytes."""
    coefs = coefficients(img, quality)
    dc_codes = [huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA)]
    ac_codes = [huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA)]
    bits, pred = _Bits(), [0, 0, 0]
    zrl = eob = 0
    for comp, block in scan_blocks(coefs):
        dc, ac = dc_codes[min(comp, 1)], ac_codes[min(comp, 1)]
        if block is None:                       # dummy: all AC zero, DC that of the block before it, i.e. difference 0
            bits.put(*dc[0])
            bits.put(*ac[0])
            eob += 1
            continue
        zz = [int(v) for v in block[ZIGZAG]]
        diff, pred[comp] = zz[0] - pred[comp], zz[0]
        size = abs(diff).bit_length()
        bits.put(*dc[size])
        if size:
            bits.put((diff if diff >= 0 else diff - 1) & ((1 << size) - 1), size)
        run = 0
        for v in zz[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                bits.put(*ac[0xF0])
                zrl += 1
                run -= 16
            size = abs(v).bit_length()
            bits.put(*ac[(run << 4) | size])
            bits.put((v if v >= 0 else v - 1) & ((1 << size) - 1), size)
            run = 0
        if run:
            bits.put(*ac[0])
            eob += 1
    data = bits.finish()
    if stats is not None:
        stats.update(zrl=zrl, eob=eob, stuffed=data.count(b"\xff\x00"))
    return data + b"\xff\xd9"


def encode(img: np.ndarray, quality: int = 95) -> bytes:
    img = np.asarray(img)
    return header(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, quality) + encode_scan(img, quality)


# ---------------------------------------------------------------- the case list shared by the CPU and GPU tests
SIZES = [(1, 1), (8, 8), (16, 16), (17, 9), (9, 17), (24, 40), (37, 53), (96, 80), (112, 112), (256, 256)]
CONTENTS = ["constant", "ramp", "noise", "checker", "impulses"]


def content(kind: str, h: int, w: int, channels: int, seed: int = 0) -> np.ndarray:
    """One test image, uint8 (h,w) or (h,w,3)."""
    rng = np.random.default_rng([seed, h, w, channels, CONTENTS.index(kind)])
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "constant":
        img = np.broadcast_to(rng.integers(0, 256, 3), (h, w, 3)).copy()
    elif kind == "ramp":
        img = np.stack([(2 * xx + yy) // 3 + 20, 200 - (xx + 3 * yy) // 4, (xx * yy) // max(1, (h + w) // 4) + 10], -1)
    elif kind == "noise":
        img = rng.integers(0, 256, (h, w, 3))
    elif kind == "checker":                     # 8-px blocks alternating black / white: the largest DC differences
        img = np.repeat(((((yy >> 3) + (xx >> 3)) & 1) * 255)[..., None], 3, -1)
    elif kind == "impulses":
        # a ramp that is constant inside every block (DC only) plus, in some blocks, a faint copy of the highest DCT basis
        # function: it quantises to one isolated +-1 at zig-zag position 63 (or 28: the highest horizontal frequency
        # alone), i.e. runs of 62 and 27 zeros, three ZRLs and one
        base = 100.0 + 3 * ((yy >> 3) + (xx >> 3))
        c7y, c7x = np.cos((2 * (yy & 7) + 1) * 7 * np.pi / 16), np.cos((2 * (xx & 7) + 1) * 7 * np.pi / 16)
        sel = ((yy >> 3) + 2 * (xx >> 3)) % 3
        sign = np.where(((yy >> 3) ^ (xx >> 3)) & 2, -1.0, 1.0)
        bump = np.where(sel == 0, 3.0 * c7y * c7x, np.where(sel == 1, 2.2 * c7x, 0.0)) * sign
        img = np.repeat(np.rint(base + bump)[..., None], 3, -1)
    else:
        raise ValueError(kind)
    img = np.clip(img, 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img[..., 1] if channels == 1 else img)


def cases():
    """Every (kind, h, w, channels) of the list: all contents at every size except 256^2, which gets noise only."""
    out = []
    for h, w in SIZES:
        for ch in (3, 1):
            for kind in (CONTENTS if (h, w) != (256, 256) else ["noise"]):
                out.append((kind, h, w, ch))
    return out
