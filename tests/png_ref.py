"""The PNG stream of ``Cropper(png_encoder="device")``, stated once in plain Python / numpy.
The kernels of ``csrc/fcp_png.hip`` are held to ``encode_stream`` byte for byte; nothing here is meant to be fast.

A face (h, w, c), c in {1, 3}, 8 bits per channel, becomes one zlib stream:

  filter   every scanline takes the PNG filter 0..4 whose filtered bytes have the smallest sum of min(v, 256 - v); ties
           go to the lowest type.  The filters read raw neighbours, so rows are independent.
  tokens   per filtered row (type byte included, never across rows): a maximal run of n equal bytes is n literals when
           n < 4, else one literal and matches at distance 1 over the other n - 1 bytes (``match_lengths``).
  codes    one dynamic Huffman block per face.  The literal/length lengths are libjpeg's jpeg_gen_optimal_table without its
           pseudo-symbol, limited to 15 bits; one distance code (code 0, length 1); a fixed code-length code.
  wrapper  78 01, the block, Adler-32 of the filtered bytes.
"""
import struct
import zlib

import numpy as np

MAX_BITS = 15
MAX_SIDE = 8192
MAX_SYMBOLS = 9227464                  # h * (w * c + 1) + 1 stays below it: no code is longer than 32 bits before the limit
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# the fixed code-length code: 14 codes of 4 bits and 4 of 5 bits (Kraft: 14/16 + 4/32 = 1); symbol 16 is never sent
CLEN_LENGTHS = tuple(5 if s in (1, 2, 3, 14) else (0 if s == 16 else 4) for s in range(19))


# ---------------------------------------------------------------------------------------------------------- filter
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img):
    """(h,w) or (h,w,c) u8 -> (h, w*c + 1) u8: every row's filter type and its filtered bytes."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = img[..., None]
    h, w, c = img.shape
    raw = img.reshape(h, w * c).astype(np.int64)
    out = np.empty((h, w * c + 1), np.uint8)
    zeros = np.zeros(w * c, np.int64)
    for y in range(h):
        x = raw[y]
        b = raw[y - 1] if y else zeros
        a = np.concatenate([zeros[:c], x[:-c]]) if w > 1 else zeros[:w * c]
        cc = np.concatenate([zeros[:c], b[:-c]]) if w > 1 else zeros[:w * c]
        cands = [(x - p) & 255 for p in (zeros, a, b, (a + b) >> 1, _paeth(a, b, cc))]
        costs = [int(np.where(v < 128, v, 256 - v).sum()) for v in cands]
        t = costs.index(min(costs))                     # the first of equals: the lowest type
        out[y, 0] = t
        out[y, 1:] = cands[t]
    return out


# ---------------------------------------------------------------------------------------------------------- tokens
def match_lengths(rem):
    """The matches (distance 1) that cover ``rem`` >= 3 bytes: 258 as long as at least 3 bytes stay behind."""
    out = []
    while rem > 258:
        m = 258 if rem - 258 >= 3 else rem - 3
        out.append(m)
        rem -= m
    out.append(rem)
    return out


def tokens(row):
    """One filtered row -> [("L", byte) | ("M", length)]."""
    row = [int(v) for v in row]
    out, i = [], 0
    while i < len(row):
        j = i
        while j < len(row) and row[j] == row[i]:
            j += 1
        n = j - i
        if n < 4:
            out += [("L", row[i])] * n
        else:
            out.append(("L", row[i]))
            out += [("M", m) for m in match_lengths(n - 1)]
        i = j
    return out


def length_symbol(m):
    """Match length 3..258 -> (symbol 257..285, number of extra bits, their value)."""
    k = max(i for i, base in enumerate(LENGTH_BASE) if base <= m)
    return 257 + k, LENGTH_EXTRA[k], m - LENGTH_BASE[k]


# ---------------------------------------------------------------------------------------------------------- Huffman
def huffman_lengths(freq, limit=MAX_BITS):
    """libjpeg's jpeg_gen_optimal_table without the pseudo-symbol: merge the two smallest non-zero frequencies (among
    equals the larger index first), limit the lengths with its bits[] loop, hand the limited lengths to the symbols in
    order of (length before the limit, symbol).  Fewer than two non-zero frequencies make no tree: all lengths are 0."""
    freq = [int(v) for v in freq]
    n = len(freq)
    size, others = [0] * n, [-1] * n
    while True:
        c1, v = -1, None
        for i in range(n):
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        c2, v = -1, None
        for i in range(n):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        size[c1] += 1                                    # one bit more for every symbol under c1 ..
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2                                  # .. the two chains become one ..
        size[c2] += 1                                    # .. and one bit more for every symbol under c2
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    bits = [0] * (max(size + [limit]) + 2)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(len(bits) - 1, limit, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    order = sorted((s, i) for i, s in enumerate(size) if s)
    out, k = [0] * n, 0
    for length in range(1, limit + 1):
        for _ in range(bits[length]):
            out[order[k][1]] = length
            k += 1
    assert k == len(order)
    return out


def canonical_codes(lengths):
    """RFC 1951 section 3.2.2: lengths -> codes (most significant bit first, as numbers)."""
    count = [0] * (max(lengths) + 2)
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * len(count), 0
    for b in range(1, len(count)):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for n in lengths:
        out.append(nxt[n] if n else 0)
        if n:
            nxt[n] += 1
    return out


def reverse_bits(v, n):
    return int(format(v, f"0{n}b")[::-1], 2) if n else 0


class BitWriter:
    """Least significant bit first, as deflate packs them."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, nbits):
        self.put(reverse_bits(code, nbits), nbits)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def code_length_sequence(lengths):
    """The literal/length lengths and the one distance length -> [(code-length symbol, extra bits, value)]."""
    out, i = [], 0
    while i < len(lengths):
        if lengths[i]:
            out.append((lengths[i], 0, 0))
            i += 1
            continue
        j = i
        while j < len(lengths) and lengths[j] == 0:
            j += 1
        n = j - i
        while n >= 11:
            k = min(n, 138)
            out.append((18, 7, k - 11))
            n -= k
        if n >= 3:
            out.append((17, 3, n - 3))
        else:
            out += [(0, 0, 0)] * n
        i = j
    return out


def adler32(data):
    """The two sums as the kernels fold them: A = (1 + sum d) mod 65521, B = (N + sum (N - i) d_i) mod 65521."""
    d = np.frombuffer(bytes(data), np.uint8).astype(object)
    n = len(d)
    a = (1 + int(d.sum())) % 65521
    b = (n + sum((n - i) * int(v) for i, v in enumerate(d))) % 65521
    return (b << 16) | a


def symbol_frequencies(filtered):
    """Counts of the 286 literal/length symbols over every row's tokens; the end-of-block symbol once."""
    freq = [0] * 286
    for row in filtered:
        for kind, v in tokens(row):
            freq[v if kind == "L" else length_symbol(v)[0]] += 1
    freq[256] = 1
    return freq


def encode_stream(img):
    """(h,w) or (h,w,c) u8 -> the zlib stream of the definition."""
    filtered = filter_rows(img)
    rows = [tokens(row) for row in filtered]
    lengths = huffman_lengths(symbol_frequencies(filtered), MAX_BITS)
    codes = canonical_codes(lengths)
    hlit = max(257, max(i for i, n in enumerate(lengths) if n) + 1) - 257
    w = BitWriter()
    w.put(1, 1)                                          # BFINAL
    w.put(2, 2)                                          # BTYPE: dynamic Huffman codes
    w.put(hlit, 5)
    w.put(0, 5)                                          # HDIST: one distance code
    w.put(15, 4)                                         # HCLEN: all 19 code-length code lengths
    for s in CLEN_ORDER:
        w.put(CLEN_LENGTHS[s], 3)
    clen_codes = canonical_codes(list(CLEN_LENGTHS))
    for sym, nbits, value in code_length_sequence(lengths[:hlit + 257] + [1]):
        w.huff(clen_codes[sym], CLEN_LENGTHS[sym])
        w.put(value, nbits)
    for row in rows:
        for kind, v in row:
            if kind == "L":
                w.huff(codes[v], lengths[v])
            else:
                sym, nbits, value = length_symbol(v)
                w.huff(codes[sym], lengths[sym])
                w.put(value, nbits)
                w.put(0, 1)                              # distance code 0: distance 1
    w.huff(codes[256], lengths[256])
    return b"\x78\x01" + w.done() + struct.pack(">I", adler32(filtered.tobytes()))


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def png_file(h, w, c, stream):
    """Signature, IHDR (8 bit, gray or RGB, no interlace), one IDAT, IEND."""
    ihdr = struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2}[c], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", bytes(stream)) + _chunk(b"IEND", b"")


# ---------------------------------------------------------------------------------------------------------- cases
SHAPES = ((1, 1, 1), (17, 9, 3), (37, 53, 3), (96, 80, 1), (96, 80, 3))
KINDS = ("noise", "smooth", "zeros", "checker", "impulses", "disc")


def smooth(h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([127.5 + 100 * np.sin(xx / 30.0 + 0.4 * c) * np.cos(yy / 20.0 - 0.3 * c) for c in range(3)],
                    -1).round().astype(np.uint8)


def smooth_bands(h, w):
    """Smooth content in four bands of rows, so that Sub, Up, Average and Paeth each win somewhere: fine vertical stripes,
    waves along y, the surface of ``smooth``, and that surface under a few gray levels of noise."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    q = h // 4
    noise = np.random.default_rng(5).integers(-10, 11, (h, w, 3)).astype(np.float64)
    planes = []
    for c in range(3):
        v = 127.5 + 60 * np.sin(xx / 3.0 + 0.4 * c) * (yy < q) + 60 * np.sin(yy / 2.0 + xx / 40 + c) * ((yy >= q) & (yy < 2 * q))
        v = v + 90 * np.sin(xx / 30.0 + 0.4 * c) * np.cos(yy / 20.0 - 0.3 * c) * (yy >= 2 * q) + noise[..., c] * (yy >= 3 * q)
        planes.append(v)
    return np.stack(planes, -1).round().clip(0, 255).astype(np.uint8)


def disc(h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return (((yy - h / 2.0) ** 2 / max(h * 0.35, 1) ** 2 + (xx - w / 2.0) ** 2 / max(w * 0.3, 1) ** 2 <= 1.0) * 255).astype(np.uint8)


def content(kind, h, w, c, seed=0):
    """(h,w,c) u8; the gray version of a colour content is its first channel, of "disc" every channel is the mask."""
    rng = np.random.default_rng(1000 * h + 10 * w + c + seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "smooth":
        return np.ascontiguousarray(smooth(h, w)[..., :c])
    if kind == "zeros":
        return np.zeros((h, w, c), np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat(((((yy // 3) + (xx // 5)) & 1) * 200 + 20).astype(np.uint8)[..., None], c, 2)
    if kind == "impulses":
        img = np.full((h, w, c), 17, np.uint8)
        img[rng.integers(0, h, max(h * w // 20, 1)), rng.integers(0, w, max(h * w // 20, 1))] = 250
        return img
    if kind == "disc":
        return np.repeat(disc(h, w)[..., None], c, 2)
    raise ValueError(kind)


def cases():
    """[(name, image (h,w,c) u8)]: every content at every shape, then the shapes that aim at one mechanism."""
    out = [(f"{kind}_{h}x{w}x{c}", content(kind, h, w, c)) for h, w, c in SHAPES for kind in KINDS]
    out.append(("zeros_3x259x1", np.zeros((3, 259, 1), np.uint8)))          # a row is a run of 260: rem 259
    out.append(("zeros_3x260x1", np.zeros((3, 260, 1), np.uint8)))          # rem 260
    out.append(("flat255_2x700x1", np.full((2, 700, 1), 255, np.uint8)))    # three matches per run
    out.append(("smooth_64x300x3", smooth_bands(64, 300)))                  # a row longer than a workgroup, every filter
    return out


def huffman_rows():
    """Rows of 286 counts for the Huffman tests, on the CPU and on the GPU: Fibonacci counts over 40 symbols (a tree 39
    deep, far past the limit) and over 33, degenerate rows, equal counts, a skewed row.  Then the rows that aim at the
    table builder the kernels share with the JPEG encoder: Fibonacci counts over 45 symbols, the deepest tree (44) a row
    that sums to less than 2^32 can make (over 46 symbols they sum to 4 807 526 975), so the lengths before the limit come
    as close to the arrays' bound of 48 as the precondition lets them; a row whose non-zero counts all sit in lane 5 of
    the wave (index % 64), so that both halves of every merge come from one lane's registers; a row whose two smallest
    counts are equal and sit in lanes 0 and 63, the two ends of the butterfly."""
    fib = [1, 1]
    while len(fib) < 45:
        fib.append(fib[-1] + fib[-2])
    one_lane, tie = [0] * 286, [0] * 286
    for i, n in ((5, 3), (69, 1), (133, 4), (197, 1), (261, 5)):
        one_lane[i] = n
    tie[0], tie[63], tie[130] = 1, 1, 7
    two = [0] * 286
    two[7], two[256] = 5, 1
    single = [0] * 286
    single[65], single[256] = 3, 1                              # one literal and the end-of-block symbol
    lone = [0] * 286
    lone[256] = 1
    skew = [(i * 7919) % 97 + (1000 if i < 3 else 0) for i in range(286)]
    return {"fib40": fib[:40] + [0] * 246, "fib33": fib[:33] + [0] * 253, "two": two, "single_literal": single, "lone": lone,
            "zeros": [0] * 286, "equal": [1] * 286, "skew": skew, "fib45": fib + [0] * 241, "one_lane": one_lane,
            "butterfly_tie": tie}
