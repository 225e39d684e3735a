"""The encoder audit's case list (tests/encoder_audit_cases.py), held to what it claims from the references alone: a case
that stopped exercising its mechanism fails here, on the CPU, not silently on the GPU.

PNG: the faces whose filtered bytes pass 65 521; the tall faces; the rows whose runs start, end or pass a 256-byte round,
literal / match switch included; the single-row faces whose block header holds a run of unused symbols of each length
around the code-length writer's switches, and whose highest used symbol is 256, 257, 284, 285; the reference stream of
every small case inflated by zlib.  JPEG: every face's file fits the default slot of h * w * c bytes (so the device path is
the one compared), every call has more than one workgroup of blocks where it says so, the extreme aspect ratios have dummy
blocks in every MCU of a row or column, the restatement equals Pillow where it is cheap, and the fixture is Pillow's."""
import importlib.util
import os
import zlib

import numpy as np
import pytest


def _load():
    spec = importlib.util.spec_from_file_location("_encoder_audit_cases", os.path.join(os.path.dirname(__file__), "encoder_audit_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


C = _load()
P, O = C.P, C.O
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


def _runs(row):
    """One filtered row -> [(start, length, byte)] of its maximal runs."""
    row = [int(v) for v in row]
    out, i = [], 0
    while i < len(row):
        j = i
        while j < len(row) and row[j] == row[i]:
            j += 1
        out.append((i, j - i, row[i]))
        i = j
    return out


# ---------------------------------------------------------------------------------------------------------- PNG
def test_png_fullsize_faces_pass_the_adler_modulus_with_data_in_folded_rows():
    cases = C.png_fullsize_cases() + [C.png_big_case()]
    assert [img.shape for _, img in cases] == [(256, 256, c) for c in (1, 3, 4) for _ in range(3)] + [(512, 512, 3)]
    for name, img in cases:
        h, w, c = img.shape
        filtered = P.filter_rows(img)
        assert filtered.shape == (h, w * c + 1) and h * (w * c + 1) > C.ADLER, name
        assert h * (w * c + 1) + 1 < P.MAX_SYMBOLS, name
        total, length = h * (w * c + 1), w * c + 1
        folded = [y for y in range(h) if total - y * length >= C.ADLER and filtered[y].any()]
        # rows with data whose factor total - y * len is reduced by the modulus; the gray disc has none (its first two rows
        # are empty), it is here for its long runs
        assert folded or name == "disc_256x256x1", name
        if "noise" in name:
            assert filtered[:, 1:].any(axis=1).all(), name     # every row's sum is non-zero: every row's fold counts
        if "smooth" in name:                                   # (its band of vertical stripes filters to empty rows: Up)
            assert filtered[:, 1:].any(axis=1).sum() > h // 2, name
    types = set(P.filter_rows(C.png_big_case()[1])[:, 0].tolist())
    assert types >= {1, 2, 3, 4}, types                        # Sub, Up, Average and Paeth each win somewhere
    types = set(P.filter_rows(C.png_content("smooth_bands", 256, 256, 4))[:, 0].tolist())
    assert len(types) >= 3, types


def test_png_tall_faces():
    assert [(h % 4, h > 256, h > 1024) for h, _, _ in C.TALL] == [(1, True, False), (3, True, False), (2, True, True)]
    for (name, img), shape in zip(C.png_tall_cases(), C.TALL):
        assert img.shape == shape and len(set(img.ravel().tolist())) > 100, name


def test_png_run_boundary_rows():
    cases = C.png_run_boundary_cases()
    assert [img.shape[1] for _, img, _ in cases] == [255, 256, 257, 300, 520]
    seen = set()
    for name, img, marks in cases:
        filtered = P.filter_rows(img)
        for y, start, n in marks:
            assert filtered[y, 0] == 1, (name, y, "Sub was to win this row")
            runs = {(s, k) for s, k, _ in _runs(filtered[y])}
            assert (start, n) in runs, (name, y, start, n)
            seen.add((img.shape[1], start, n))
            toks = P.tokens(filtered[y])
            if n >= 4:                                         # a literal and matches over the other n - 1 bytes
                assert ("M", n - 1) in toks or n - 1 > 258, (name, y)
    for w in (255, 256, 257):
        for p in (255, 256, 257):
            if p > w:
                continue
            # a run of 3 and a run of 4 end at p (the literal / match switch), and a run starts there
            assert (w, p - 3, 3) in seen and (w, p - 4, 4) in seen, (w, p)
            assert any(s == p for ww, s, _ in seen if ww == w), (w, p)
    assert (257, 255, 3) in seen                                               # the widest of the three still holds a run of 3 there
    for p in (255, 256, 257):                                                  # the wider face holds both, whole, at every p
        assert {(300, p - 3, 3), (300, p, 4), (300, p - 4, 4), (300, p, 3)} <= seen, p
    assert (300, 10, 259) in seen and 10 < C.ROUND < 10 + 259                  # over one round boundary
    assert (520, 255, 259) in seen and 255 < C.ROUND and 2 * C.ROUND < 255 + 259   # starts in round 0, ends in round 2
    assert P.match_lengths(258) == [258]


def test_png_header_writer_faces():
    cases = C.png_header_cases()
    assert [what for _, _, what in cases] == [("gap", n) for n in C.GAPS] + [("highest", s) for s in (256, 257, 284, 285)]
    for name, img, (what, v) in cases:
        assert img.shape[0] == 1 and img.shape[2] == 1
        filtered = P.filter_rows(img)
        assert filtered[0, 0] == 0, (name, "filter 0 was to win")
        freq = P.symbol_frequencies(filtered)
        lengths = P.huffman_lengths(freq, P.MAX_BITS)
        used = [i for i, n in enumerate(lengths) if n]
        assert used == [i for i, n in enumerate(freq) if n], name
        hlit = max(257, used[-1] + 1) - 257
        seq = P.code_length_sequence(lengths[:hlit + 257] + [1])
        if what == "gap":
            assert used[:2] == [0, v + 1], (name, used)        # symbols 1..v are unused: a run of exactly v zero lengths
            want = C.GAP_CODES[v]
            assert seq[0] == (lengths[0], 0, 0) and seq[1:1 + len(want)] == want and seq[1 + len(want)] == (lengths[v + 1], 0, 0), \
                (name, seq[:6])
            zeros = 0
            for sym, _, value in want:
                zeros += 1 if sym == 0 else value + (3 if sym == 17 else 11)
            assert zeros == v, name
        else:
            assert used[-1] == v and hlit == max(257, v + 1) - 257, name
            if C.HIGHEST[v]:
                assert ("M", C.HIGHEST[v]) in P.tokens(filtered[0]) and P.length_symbol(C.HIGHEST[v])[0] == v, name
    kinds = {s for name, img, (what, v) in cases if what == "gap" for s, _, _ in C.GAP_CODES[v]}
    assert kinds == {0, 17, 18}


@pytest.fixture(scope="module")
def png_streams():
    return [(name, img, P.encode_stream(img)) for name, img in C.png_small_cases()]


def test_png_reference_streams_inflate_to_the_filtered_rows(png_streams):
    """zlib, an inflater this project did not write, reads the reference's stream of every case and checks its Adler-32."""
    assert len(png_streams) == 9 + 3 + 5 + len(C.GAPS) + 4
    for name, img, stream in png_streams:
        assert zlib.decompress(stream) == P.filter_rows(img).tobytes(), name
    names = [n for n, _, _ in png_streams]
    assert len(set(names)) == len(names)


# ---------------------------------------------------------------------------------------------------------- JPEG
def test_jpeg_groups_are_the_issues():
    groups = C.jpeg_groups()
    assert len(groups) == 2 * 4 * 2 + 2 + 4 * 2 * 2 and len({g[0] for g in groups}) == len(groups)
    assert C.QUALITY == 90 and C.CONTENTS == ("ramp", "checker", "lownoise")
    assert {(g[3], g[4]) for g in groups if g[1:3] in C.FULL_SIZES} == set(O.MODES)
    assert [(g[1:6]) for g in groups if g[1] == 1024] == [(1024, 1024, 3, "4:2:0", False), (1024, 1024, 3, "4:4:4", True)]
    assert all(g[6] == (g[1] != 1024) for g in groups)
    for _, h, w, ch, ss, opt, _ in groups:
        bh, bw, blocks, dummies = C.block_grid(h, w, ch, ss)
        if (h, w) in C.FULL_SIZES or h == 1024:
            assert blocks > 256 and dummies == 0               # more than one workgroup of blocks per face
        else:                                                  # extreme aspect: an odd block grid along the short side
            assert max(h, w) == 8192 and min(h, w) in (1, 3) and blocks >= 1024
            if ch == 3:
                hs, vs = O.LUMA_FACTORS[O.sub_index(ss)]
                short_blocks, factor = (bh, vs) if h < w else (bw, hs)
                assert short_blocks == 1
                assert dummies == (1024 if factor == 2 else 0), (h, w, ss, dummies)
    # dummy blocks in every MCU of the long row or column: 4:2:0 both ways, 4:2:2 for the tall faces
    assert C.block_grid(3, 8192, 3, "4:2:0")[3] == 1024 and C.block_grid(8192, 3, 3, "4:2:0")[3] == 1024
    assert C.block_grid(8192, 3, 3, "4:2:2")[3] == 1024 and C.block_grid(8192, 1, 3, "4:2:2")[3] == 1024


def test_jpeg_faces_differ_and_fit_the_default_slot():
    """Pillow's whole file (the fixture's length, which ``test_jpeg_fixture_is_pillows`` holds to Pillow), header
    included, is shorter than h * w * c: so is the scan, and no face leaves the device."""
    golden = np.load(os.path.join(ROOT, "tests", "golden", "encoder_audit.npz"))
    for name, h, w, ch, ss, opt, _ in C.jpeg_groups():
        kinds, imgs = C.jpeg_faces(h, w, ch)
        assert len({im.tobytes() for im in imgs}) == 3, name
        if min(h, w) < 8:
            continue                                           # the GPU test gives the slivers a slot of their whole blocks
        for kind in kinds:
            assert int(golden[C.fixture_key(name, kind)][0]) < h * w * ch, (name, kind)


def test_jpeg_fixture_is_pillows():
    golden = np.load(os.path.join(ROOT, "tests", "golden", "encoder_audit.npz"))
    keys = {C.fixture_key(g[0], kind) for g in C.jpeg_groups() for kind in C.CONTENTS}
    assert {k for k in golden.files if k.startswith("sum_")} == keys
    assert [v.split()[0] for v in golden["versions"].tolist()] == ["Pillow", "libjpeg-turbo", "numpy"]
    for name, h, w, ch, ss, opt, _ in C.jpeg_groups():
        kinds, imgs = C.jpeg_faces(h, w, ch)
        for kind, img in zip(kinds, imgs):
            assert int(golden[f"crc_{kind}_{h}x{w}x{ch}"]) == zlib.crc32(img.tobytes()), (name, kind, "the input changed")
            if _turbo():
                data = O.pillow(img, C.QUALITY, ss, opt)
                assert golden[C.fixture_key(name, kind)].tolist() == [len(data), zlib.crc32(data)], (name, kind)


def test_jpeg_restatement_equals_pillow_on_the_extreme_aspects():
    """The cheap part of the comparison the GPU test makes at every size: restatement, standard and optimised, against
    Pillow; and ``restate`` (symbols computed once) against jpeg_options_ref.encode_scan."""
    for h, w, ch in C.ASPECTS:
        kinds, imgs = C.jpeg_faces(h, w, ch)
        for ss in C.ASPECT_SUBSAMPLINGS:
            for kind, img in zip(kinds[1:], imgs[1:]):
                both = C.restate(img, C.QUALITY, ss)
                for opt in (False, True):
                    scan, records = both[opt]
                    assert scan == O.encode_scan(img, C.QUALITY, ss, opt), (h, w, ss, kind, opt)
                    if _turbo():
                        tables = O.tables_of(img, C.QUALITY, ss, opt)
                        assert O.header(h, w, ch, C.QUALITY, ss, tables) + scan == O.pillow(img, C.QUALITY, ss, opt), (h, w, ss, kind)
                    if opt:
                        assert records == b"".join(O.table_record(t) for t in O.tables_of(img, C.QUALITY, ss, True))
