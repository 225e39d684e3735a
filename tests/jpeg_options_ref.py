"""tests/jpeg_ref.py extended by the three settings of ``Cropper(jpeg_quality=, jpeg_subsampling=, jpeg_optimize=)``: the
reference of tests/test_jpeg_options_cpu.py and test_jpeg_options_gpu.py.

On top of jpeg_ref's colour conversion, DCT, quantisation and entropy coder it adds the sample planes of 4:4:4 and 4:2:2
(libjpeg's ``fullsize_downsample`` and ``h2v1_downsample``: edge replication of the full-resolution plane, then for 4:2:2
the pair average with bias 0 in even and 1 in odd output columns), MCUs of ``hs * vs`` Y blocks followed by Cb and Cr, and
the statistics pass and ``jpeg_gen_optimal_table`` of libjpeg's ``optimize_coding``.  ``Image.fromarray(a).save(buf,
"JPEG", quality=q, subsampling=s, optimize=o)`` is what ``encode`` has to equal, byte for byte."""
import importlib.util
import os

import numpy as np


def _load_base():
    spec = importlib.util.spec_from_file_location("_jpeg_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load_base()

SUBSAMPLINGS = ("4:4:4", "4:2:2", "4:2:0")          # index = the `subsampling` argument of the C entry points
LUMA_FACTORS = ((1, 1), (2, 1), (2, 2))             # (hs, vs) of the Y component
FIB35 = 9227465
MAX_CLEN = 32


def sub_index(subsampling) -> int:
    return SUBSAMPLINGS.index(subsampling) if isinstance(subsampling, str) else int(subsampling)


# ---------------------------------------------------------------- samples
def component_planes(img: np.ndarray, subsampling=2):
    """uint8 (h,w) or (h,w,3) -> component planes, each padded to whole blocks of its own block grid."""
    img = np.asarray(img)
    ss = sub_index(subsampling)
    if img.ndim == 2 or ss == 2:
        return R.component_planes(img)
    h, w = img.shape[:2]
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    full = [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
            (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
            (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16]
    bw, bh = -(-w // 8), -(-h // 8)
    ys, xs = np.minimum(np.arange(8 * bh), h - 1), np.minimum(np.arange(8 * bw), w - 1)
    planes = [full[0][ys][:, xs]]
    for p in full[1:]:
        if ss == 0:
            planes.append(p[ys][:, xs])
        else:
            cw = -(-(-(-w // 2)) // 8)
            xo = np.arange(8 * cw)
            x0, x1 = np.minimum(2 * xo, w - 1), np.minimum(2 * xo + 1, w - 1)
            rows = p[ys]
            planes.append((rows[:, x0] + rows[:, x1] + (xo & 1)) >> 1)
    return planes


def coefficients(img: np.ndarray, quality: int = 95, subsampling=2):
    """jpeg_ref.coefficients for the planes above."""
    qt = R.quant_tables(quality)
    out = []
    for k, plane in enumerate(component_planes(img, subsampling)):
        bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
        blocks = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3) - 128
        rows = R._dct_pass(blocks, True)
        both = R._dct_pass(rows.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)
        div = (8 * qt[min(k, 1)]).reshape(8, 8)
        mag = (np.abs(both) + div // 2) // div
        out.append((np.sign(both) * mag).reshape(bh, bw, 64))
    return out


def scan_blocks(coefs, subsampling=2):
    """MCU order: [(component, block (64,) natural order or None for a dummy)]; an MCU is hs * vs Y blocks row by row, Cb, Cr."""
    if len(coefs) == 1:
        return [(0, b) for row in coefs[0] for b in row]
    hs, vs = LUMA_FACTORS[sub_index(subsampling)]
    ybh, ybw = coefs[0].shape[:2]
    out = []
    for my in range(coefs[1].shape[0]):
        for mx in range(coefs[1].shape[1]):
            for dy in range(vs):
                for dx in range(hs):
                    y, x = vs * my + dy, hs * mx + dx
                    out.append((0, coefs[0][y, x] if y < ybh and x < ybw else None))
            out.append((1, coefs[1][my, mx]))
            out.append((2, coefs[2][my, mx]))
    return out


# ---------------------------------------------------------------- symbols
def block_symbols(blocks):
    """-> [(table set 0 / 1, 'dc' / 'ac', symbol, value bits, size)] of the whole scan, dummies included (DC 0 and EOB)."""
    out, pred = [], [0, 0, 0]
    for comp, block in blocks:
        t = min(comp, 1)
        if block is None:
            out.append((t, "dc", 0, 0, 0))
            out.append((t, "ac", 0, 0, 0))
            continue
        zz = [int(v) for v in block[R.ZIGZAG]]
        diff, pred[comp] = zz[0] - pred[comp], zz[0]
        size = abs(diff).bit_length()
        out.append((t, "dc", size, (diff if diff >= 0 else diff - 1) & ((1 << size) - 1), size))
        run = 0
        for v in zz[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                out.append((t, "ac", 0xF0, 0, 0))
                run -= 16
            size = abs(v).bit_length()
            out.append((t, "ac", (run << 4) | size, (v if v >= 0 else v - 1) & ((1 << size) - 1), size))
            run = 0
        if run:
            out.append((t, "ac", 0, 0, 0))
    return out


def histograms(symbols):
    """-> (4, 256) int64 in record order: Y DC, Y AC, chroma DC, chroma AC."""
    freq = np.zeros((4, 256), np.int64)
    for t, kind, sym, _, _ in symbols:
        freq[2 * t + (kind == "ac"), sym] += 1
    return freq


# ---------------------------------------------------------------- libjpeg's jpeg_gen_optimal_table
def gen_optimal_table(freq, info: dict | None = None):
    """256 frequencies -> (codes per length 1..16, symbols in code order).  ``info['depth']`` gets the deepest code before
    the lengths are limited to 16.  An all-zero row gives an empty table."""
    freq = [int(v) for v in freq] + [1]
    assert len(freq) == 257
    if not any(freq[:256]):
        if info is not None:
            info["depth"] = 0
        return [0] * 16, []
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    if info is not None:
        info["depth"] = max(codesize)
    assert max(codesize) <= MAX_CLEN, "libjpeg: Huffman code size table overflow"
    bits = [0] * (MAX_CLEN + 1)
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(MAX_CLEN, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    symbols = [j for n in range(1, MAX_CLEN + 1) for j in range(256) if codesize[j] == n]
    return bits[1:17], symbols


def table_record(table) -> bytes:
    """(counts, symbols) -> the 272-byte record of the `tables` buffer: 16 counts, the symbols in code order, zero padded."""
    counts, symbols = table
    return bytes(counts) + bytes(symbols) + bytes(256 - len(symbols))


def code_words(table) -> np.ndarray:
    """(counts, symbols) -> 256 x uint32 ``code | length << 16`` by symbol (0 where the symbol has no code)."""
    out = np.zeros(256, np.uint32)
    for sym, (code, length) in R.huffman_codes(table).items():
        out[sym] = code | (length << 16)
    return out


STANDARD = ((R.DC_LUMA, R.AC_LUMA), (R.DC_CHROMA, R.AC_CHROMA))


def tables_of(img, quality=95, subsampling=2, optimize=False):
    """-> [Y DC, Y AC, chroma DC, chroma AC] as (counts, symbols); gray images have empty chroma tables when optimised."""
    if not optimize:
        return [STANDARD[0][0], STANDARD[0][1], STANDARD[1][0], STANDARD[1][1]]
    blocks = scan_blocks(coefficients(img, quality, subsampling), subsampling)
    return [gen_optimal_table(row) for row in histograms(block_symbols(blocks))]


# ---------------------------------------------------------------- the bytes
def header(h, w, channels, quality, subsampling=2, tables=None) -> bytes:
    """jpeg_ref.header with the sampling byte of the first component following the subsampling (gray too) and, when
    ``tables`` (four (counts, symbols)) is given, those Huffman tables in the DHT segments."""
    assert channels in (1, 3)
    ss = sub_index(subsampling)
    qt = R.quant_tables(quality)
    tables = tables_of(None) if tables is None else tables
    out = b"\xff\xd8" + R._segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    sets = 1 if channels == 1 else 2
    for k in range(sets):
        out += R._segment(0xDB, bytes([k]) + bytes(int(v) for v in qt[k][R.ZIGZAG]))
    comps = [(1, (0x11, 0x21, 0x22)[ss], 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if channels == 3 else [])
    out += R._segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([channels]) +
                      b"".join(bytes(c) for c in comps))
    for k in range(sets):
        dc, ac = tables[2 * k], tables[2 * k + 1]
        out += R._segment(0xC4, bytes([k]) + bytes(dc[0]) + bytes(dc[1]))
        out += R._segment(0xC4, bytes([0x10 | k]) + bytes(ac[0]) + bytes(ac[1]))
    return out + R._segment(0xDA, bytes([channels]) + b"".join(bytes([c[0], 0x11 * c[2]]) for c in comps) + b"\x00\x3f\x00")


def encode_scan(img, quality=95, subsampling=2, optimize=False, tables=None) -> bytes:
    """Entropy-coded segment + EOI."""
    blocks = scan_blocks(coefficients(img, quality, subsampling), subsampling)
    symbols = block_symbols(blocks)
    if tables is None:
        tables = [gen_optimal_table(row) for row in histograms(symbols)] if optimize else tables_of(None)
    codes = [R.huffman_codes(t) for t in tables]
    bits = R._Bits()
    for t, kind, sym, value, size in symbols:
        bits.put(*codes[2 * t + (kind == "ac")][sym])
        if size:
            bits.put(value, size)
    return bits.finish() + b"\xff\xd9"


def encode(img, quality=95, subsampling=2, optimize=False) -> bytes:
    img = np.asarray(img)
    tables = tables_of(img, quality, subsampling, optimize)
    return (header(img.shape[0], img.shape[1], 1 if img.ndim == 2 else 3, quality, subsampling, tables) +
            encode_scan(img, quality, subsampling, optimize, tables))


def pillow(img, quality=95, subsampling="4:2:0", optimize=False) -> bytes:
    """Pillow's file at these settings, whatever the image's size (``optimize`` needs the whole file in one buffer)."""
    import io
    from PIL import Image, ImageFile
    buf = io.BytesIO()
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = max(old, 4096 + 4 * np.asarray(img).size)
    try:
        Image.fromarray(img).save(buf, format="JPEG", quality=quality, subsampling=SUBSAMPLINGS[sub_index(subsampling)],
                                  optimize=bool(optimize))
    finally:
        ImageFile.MAXBLOCK = old
    return buf.getvalue()


# ---------------------------------------------------------------- the case list shared by the CPU and GPU tests
SIZES = [(1, 1), (8, 8), (16, 16), (17, 9), (9, 17), (24, 40), (37, 53), (96, 80), (112, 112)]
GPU_SIZES = SIZES[:7]
EXTRA_QUALITY_SIZES = [(17, 9), (37, 53)]
MODES = [(3, "4:4:4"), (3, "4:2:2"), (3, "4:2:0"), (1, "4:2:0")]      # (channels, subsampling): RGB at three, plus gray


def cases(sizes=None, extra_qualities=(1, 50, 100)):
    """[(kind, h, w, channels, subsampling, optimize, quality)]"""
    out = []
    for h, w in (SIZES if sizes is None else sizes):
        qualities = (95,) + (tuple(extra_qualities) if (h, w) in EXTRA_QUALITY_SIZES else ())
        for ch, ss in MODES:
            for opt in (False, True):
                for q in qualities:
                    for kind in R.CONTENTS:
                        out.append((kind, h, w, ch, ss, opt, q))
    return out


def case_key(case) -> str:
    kind, h, w, ch, ss, opt, q = case
    return f"{kind}_{h}x{w}x{ch}_{ss.replace(':', '')}_{'opt' if opt else 'std'}_q{q}"


def fibonacci_image(shift: int = 0, nsym: int = 19):
    """The length-limit pins: gray 840 x 840, 105 x 105 blocks; symbol i of ``nsym`` (zig-zag position 1 + i % 10, value
    (1, 2, 4)[i // 10], i.e. run i % 10 and size i // 10 + 1) is the one non-zero AC coefficient of Fibonacci(i + 1 + shift)
    blocks, the remaining blocks are flat 128; at quality 50 the divisors are the Annex K table itself.
    (0, 19) is the image the feature's issue describes: 10 945 one-coefficient blocks and 80 flat ones.  Its tree is only 12
    deep: libjpeg breaks ties towards the largest index, i.e. towards single symbols and away from merged nodes, so the
    two leading 1s (the pseudo-symbol and Fibonacci(1)) start two interleaved chains.  (1, 18) — counts 1, 2, 3, 5, ... —
    has no such tie: one chain, 19 deep before the limit.  -> (image, {symbol: count})."""
    fib = [1, 1]
    while len(fib) < nsym + shift:
        fib.append(fib[-1] + fib[-2])
    fib = fib[shift:]
    q = R.quant_tables(50)[0]
    yy, xx = np.mgrid[0:8, 0:8]
    blocks, want = [], {}
    for i in range(nsym):
        pos, value = 1 + i % 10, (1, 2, 4)[i // 10]
        nat = int(R.ZIGZAG[pos])
        u, v = nat // 8, nat % 8                                   # vertical, horizontal frequency
        cu, cv = (np.sqrt(0.5) if u == 0 else 1.0), (np.sqrt(0.5) if v == 0 else 1.0)
        basis = 0.25 * cu * cv * np.cos((2 * yy + 1) * u * np.pi / 16) * np.cos((2 * xx + 1) * v * np.pi / 16)
        block = np.clip(np.rint(128 + value * int(q[nat]) * basis), 0, 255).astype(np.uint8)
        blocks += [block] * fib[i]
        want[((pos - 1) << 4) | value.bit_length()] = fib[i]
    assert len(blocks) <= 105 * 105
    blocks += [np.full((8, 8), 128, np.uint8)] * (105 * 105 - len(blocks))
    img = np.stack(blocks).reshape(105, 105, 8, 8).transpose(0, 2, 1, 3).reshape(840, 840)
    want[0] = 105 * 105
    return np.ascontiguousarray(img), want


def fibonacci_row(nsym: int, shift: int = 0) -> np.ndarray:
    """256 frequencies: symbol i < nsym occurs Fibonacci(i + 1 + shift) times."""
    fib = [1, 1]
    while len(fib) < nsym + shift:
        fib.append(fib[-1] + fib[-2])
    row = np.zeros(256, np.int64)
    row[:nsym] = fib[shift:shift + nsym]
    return row
