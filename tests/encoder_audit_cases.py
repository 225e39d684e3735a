"""The case lists of the encoder audit (tests/test_encoder_audit_cpu.py asserts, from the references alone, that every case
exercises the mechanism it is here for; tests/test_encoder_audit_gpu.py holds the kernels of csrc/fcp_png.hip and
csrc/fcp_jpeg.hip to the references on them, byte for byte).  Everything is built on tests/png_ref.py, tests/jpeg_ref.py
and tests/jpeg_options_ref.py; nothing here reads the code under test.

PNG: faces at and above the default output size, so that a face's filtered bytes pass 65 521 (the Adler-32 fold
``((total - y * len) % 65521) * sum`` runs with total >= 65521) and the bit-offset scan carries over more than 256 and more
than 1024 rows; rows whose runs start, end or pass the 256-byte rounds of the filter kernel; single-row faces that pin the
alphabet of the block header (runs of unused symbols around the 3 / 11 / 138 switches of the code-length writer, the
highest used symbol).

JPEG: the default output size and above at every mode with standard and optimised tables, on contents whose stream fits
the default slot (so the device path is the one compared); 1024 x 1024; faces 1, 3 px wide or high and 8192 the other
way, whose odd block grids put dummy blocks into every MCU of a row or column."""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location("_audit_" + name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _load("png_ref")
O = _load("jpeg_options_ref")
J = O.R
ADLER = 65521
ROUND = 256                                  # bytes of a filtered row one round of png_filter_kernel takes


# ---------------------------------------------------------------------------------------------------------- PNG
def png_content(kind, h, w, c):
    """(h,w,c) u8.  ``smooth_bands`` is RGB: gray is its first channel, RGBA adds the disc as the alpha."""
    if kind != "smooth_bands":
        return P.content(kind, h, w, c)
    rgb = P.smooth_bands(h, w)
    if c == 4:
        return np.ascontiguousarray(np.concatenate([rgb, P.disc(h, w)[..., None]], -1))
    return np.ascontiguousarray(rgb[..., :c])


def png_fullsize_cases():
    """[(name, image)]: 256 x 256 at c = 1, 3, 4; h * (w * c + 1) > 65521 for every one of them."""
    return [(f"{kind}_256x256x{c}", png_content(kind, 256, 256, c)) for c in (1, 3, 4)
            for kind in ("smooth_bands", "noise", "disc")]


def png_big_case():
    return "smooth_bands_512x512x3", png_content("smooth_bands", 512, 512, 3)


TALL = ((257, 3, 1), (263, 7, 1), (1030, 5, 3))          # h % 4 = 1, 3, 2; more than 256 and more than 1024 rows


def png_tall_cases():
    return [(f"noise_{h}x{w}x{c}", P.content("noise", h, w, c)) for h, w, c in TALL]


def _sub_rows(wanted, w, seed):
    """Gray face whose odd rows filter (Sub, type 1) to the rows of ``wanted`` (each w bytes): row 2k + 1 is the running
    sum of wanted[k], rows 2k are noise, which keeps Up, Average and Paeth expensive on the rows that count."""
    rng = np.random.default_rng(seed)
    rows = []
    for d in wanted:
        assert len(d) == w
        rows.append(rng.integers(0, 256, w, dtype=np.uint8))
        rows.append((np.cumsum(np.asarray(d, np.int64)) & 255).astype(np.uint8))
    return np.stack(rows)[..., None]


def _filler(n, phase=0):
    """n bytes without a run longer than one: 2, 3, 2, 3 .. (never 1, the Sub type byte, nor a run value below)."""
    return [2 + ((i + phase) & 1) for i in range(n)]


def _row_with_runs(w, runs):
    """The w filtered bytes behind the type byte (positions 1..w of the row) with ``runs`` [(start position in the row,
    length, value)] laid over the filler; the filler next to a run differs from it (values >= 5)."""
    d = _filler(w)
    for start, n, v in runs:
        assert 1 <= start and start + n <= w + 1 and v >= 5
        d[start - 1:start - 1 + n] = [v] * n
    return d


def png_run_boundary_cases():
    """[(name, image, [(row of the image, start, length)])]: gray faces with w = 255, 256, 257 whose Sub-filtered rows
    hold a run of 3 that ends and a run of 4 that starts at byte p of the row (and 4 / 3), for every p in 255, 256, 257 the
    row has; where the row ends before the second run is complete it is cut there.  Two wider faces hold a run of 259
    over one and over two round boundaries."""
    out = []
    for w in (255, 256, 257):
        wanted, marks = [], []
        for p in (255, 256, 257):
            if p > w:
                continue
            for first, second in ((3, 4), (4, 3)):
                second = min(second, w + 1 - p)
                wanted.append(_row_with_runs(w, [(p - first, first, 5), (p, second, 7)]))
                marks.append((2 * len(wanted) - 1, p - first, first))
                marks.append((2 * len(wanted) - 1, p, second))
        out.append((f"runs_{2 * len(wanted)}x{w}x1", _sub_rows(wanted, w, w), marks))
    for w, start in ((300, 10), (520, 255)):                               # bytes 10..268 and 255..513
        wanted, marks = [_row_with_runs(w, [(start, 259, 5)])], [(1, start, 259)]
        if w == 300:                                                       # wide enough for whole runs of 4 and 3 from every p
            for p in (255, 256, 257):
                for first, second in ((3, 4), (4, 3)):
                    wanted.append(_row_with_runs(w, [(p - first, first, 5), (p, second, 7)]))
                    marks += [(2 * len(wanted) - 1, p - first, first), (2 * len(wanted) - 1, p, second)]
        out.append((f"run259_{2 * len(wanted)}x{w}x1", _sub_rows(wanted, w, w), marks))
    return out


GAPS = (1, 2, 3, 10, 11, 12, 138, 139, 140, 141, 148, 149, 150)
# what the code-length writer has to send for a run of n zero lengths: (symbol, extra bits, value)
GAP_CODES = {1: [(0, 0, 0)], 2: [(0, 0, 0)] * 2, 3: [(17, 3, 0)], 10: [(17, 3, 7)], 11: [(18, 7, 0)], 12: [(18, 7, 1)],
             138: [(18, 7, 127)], 139: [(18, 7, 127), (0, 0, 0)], 140: [(18, 7, 127), (0, 0, 0), (0, 0, 0)],
             141: [(18, 7, 127), (17, 3, 0)], 148: [(18, 7, 127), (17, 3, 7)], 149: [(18, 7, 127), (18, 7, 0)],
             150: [(18, 7, 127), (18, 7, 1)]}
HIGHEST = {256: 0, 257: 3, 284: 240, 285: 258}           # highest used symbol -> the match length that makes it (0: none)


def png_header_cases():
    """[(name, image (1,w,1), ("gap", n) | ("highest", symbol))]: one scanline that filter 0 wins, so the literals of the
    block are the type byte 0 and the pixels' own values.  Gap n: the pixels alternate between n + 1 and a larger value,
    the first (searched from 255 down) with which filter 0 wins; the symbols 1..n are unused.  Highest symbol s: a run of
    zeros behind the type byte as long as the match needs, then 200, 60, 200."""
    out = []
    for n in GAPS:
        for other in range(255, n + 1, -1):
            img = np.array([n + 1, other] * 3, np.uint8).reshape(1, 6, 1)
            if P.filter_rows(img)[0, 0] == 0:
                break
        else:
            raise AssertionError(f"no face for a gap of {n}")
        out.append((f"gap{n}_1x6x1", img, ("gap", n)))
    for sym, m in HIGHEST.items():
        px = [0] * m + [200, 60, 200]                    # the type byte and m zeros: one literal and a match of m
        out.append((f"highest{sym}_1x{len(px)}x1", np.array(px, np.uint8).reshape(1, len(px), 1), ("highest", sym)))
    return out


def png_small_cases():
    """Every PNG case but 512 x 512 (whose reference takes seconds): [(name, image)]."""
    return (png_fullsize_cases() + png_tall_cases() + [(n, im) for n, im, _ in png_run_boundary_cases()] +
            [(n, im) for n, im, _ in png_header_cases()])


# ---------------------------------------------------------------------------------------------------------- JPEG
QUALITY = 90
CONTENTS = ("ramp", "checker", "lownoise")
FULL_SIZES = ((256, 256), (512, 512))
BIG_MODES = ((3, "4:2:0", False), (3, "4:4:4", True))                    # 1024 x 1024: Pillow and the fixture only
ASPECTS = ((3, 8192, 3), (8192, 3, 3), (1, 8192, 1), (8192, 1, 3))       # (h, w, channels)
ASPECT_SUBSAMPLINGS = ("4:2:2", "4:2:0")


def jpeg_content(kind, h, w, ch):
    """jpeg_ref's ramp and checker; ``lownoise``: 128 +- 8 of noise, which codes to well under a byte per sample."""
    if kind != "lownoise":
        return J.content(kind, h, w, ch)
    rng = np.random.default_rng([7, h, w, ch])
    img = (128 + rng.integers(-8, 9, (h, w, 3))).astype(np.uint8)
    return np.ascontiguousarray(img[..., 1] if ch == 1 else img)


def jpeg_groups():
    """[(group name, h, w, channels, subsampling, optimize, restate)]: one device call each, over the faces of
    ``jpeg_faces``; ``restate``: whether the restatement is part of the comparison (it is too slow at 1024 x 1024)."""
    out = []
    for h, w in FULL_SIZES:
        for ch, ss in O.MODES:
            for opt in (False, True):
                out.append((h, w, ch, ss, opt, True))
    for ch, ss, opt in BIG_MODES:
        out.append((1024, 1024, ch, ss, opt, False))
    for h, w, ch in ASPECTS:
        for ss in ASPECT_SUBSAMPLINGS:
            for opt in (False, True):
                out.append((h, w, ch, ss, opt, True))
    return [(group_key(g), *g) for g in out]


def group_key(group) -> str:
    h, w, ch, ss, opt = group[:5]
    return f"{h}x{w}x{ch}_{ss.replace(':', '')}_{'opt' if opt else 'std'}"


def jpeg_faces(h, w, ch):
    """The faces of one call: (kinds, batch (3,h,w[,3]) u8), differing content, so each has its own tables and offsets."""
    return list(CONTENTS), np.stack([jpeg_content(k, h, w, ch) for k in CONTENTS])


def fixture_key(name, kind) -> str:
    return f"sum_{kind}_{name}_q{QUALITY}"


def block_grid(h, w, ch, ss):
    """-> (Y blocks high, Y blocks wide, blocks of the scan, dummy blocks of the scan)."""
    bh, bw = -(-h // 8), -(-w // 8)
    if ch == 1:
        return bh, bw, bh * bw, 0
    hs, vs = O.LUMA_FACTORS[O.sub_index(ss)]
    mh, mw = -(-bh // vs), -(-bw // hs)
    return bh, bw, mh * mw * (hs * vs + 2), mh * mw * hs * vs - bh * bw


def restate(img, quality, subsampling):
    """The restatement's scans and table records with standard and with optimised tables, the coefficients and symbols
    computed once: {optimize: (scan bytes, table records (4 * 272 bytes) or None)}."""
    symbols = O.block_symbols(O.scan_blocks(O.coefficients(img, quality, subsampling), subsampling))
    out = {}
    for opt in (False, True):
        tables = [O.gen_optimal_table(row) for row in O.histograms(symbols)] if opt else O.tables_of(None)
        codes = [J.huffman_codes(t) for t in tables]
        bits = J._Bits()
        for t, kind, sym, value, size in symbols:
            bits.put(*codes[2 * t + (kind == "ac")][sym])
            if size:
                bits.put(value, size)
        out[opt] = (bits.finish() + b"\xff\xd9", b"".join(O.table_record(t) for t in tables) if opt else None)
    return out
