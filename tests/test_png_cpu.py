"""Cropper(png_encoder="device") without a GPU: the definition in tests/png_ref.py makes valid zlib streams and PNG files
of every case of its list, its Huffman lengths and its match rule behave as stated, the files are no longer than the host's
on the contents a Cropper writes, and the keyword, the CLI flag, the bindings and the host wrapper exist and validate."""
import importlib.util
import io
import os
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("_png_ref", os.path.join(os.path.dirname(__file__), "png_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
CASES = R.cases()


def _decode(file):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(file)))


def _pillow_png(img):
    from PIL import Image
    from face_crop_plus_amd._io_codec import _ENCODER_KW
    assert _ENCODER_KW[".png"] == dict(format="PNG", compress_level=1)
    buf = io.BytesIO()
    Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(buf, **_ENCODER_KW[".png"])
    return buf.getvalue()


@pytest.fixture(scope="module")
def streams():
    return {name: R.encode_stream(img) for name, img in CASES}


def test_case_list_covers_the_shapes_and_contents():
    names = [n for n, _ in CASES]
    assert len(names) == len(set(names)) == 5 * 6 + 4
    for shape in ("1x1x1", "17x9x3", "37x53x3", "96x80x1", "96x80x3"):
        for kind in R.KINDS:
            assert f"{kind}_{shape}" in names
    for img in dict(CASES).values():
        assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in (1, 3)


@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_reference_stream_inflates_to_the_filtered_rows_and_pillow_decodes_the_file(streams, name):
    img = dict(CASES)[name]
    h, w, c = img.shape
    stream = streams[name]
    filtered = R.filter_rows(img)
    assert filtered.shape == (h, w * c + 1) and int(filtered[:, 0].max()) <= 4
    assert stream[:2] == b"\x78\x01" and (stream[0] * 256 + stream[1]) % 31 == 0
    assert zlib.decompress(stream) == filtered.tobytes()
    assert int.from_bytes(stream[-4:], "big") == zlib.adler32(filtered.tobytes())
    got = _decode(R.png_file(h, w, c, stream))
    assert got.dtype == np.uint8 and np.array_equal(got.reshape(img.shape), img)


def test_the_wide_smooth_case_uses_the_filters():
    types = set(R.filter_rows(dict(CASES)["smooth_64x300x3"])[:, 0].tolist())
    print("filter types on smooth_64x300x3:", sorted(types))
    assert len(types) >= 3 and types >= {1, 2, 3, 4}


def test_filters_are_the_png_filters():
    """Undo every row's filter as the PNG specification says a decoder does: the pixels come back."""
    img = dict(CASES)["noise_37x53x3"]
    h, w, c = img.shape
    f = R.filter_rows(img).astype(np.int64)
    assert set(f[:, 0].tolist()) == {0, 1, 2, 3, 4}
    out = np.zeros((h, w * c), np.int64)
    for y in range(h):
        for j in range(w * c):
            a = out[y, j - c] if j >= c else 0
            b = out[y - 1, j] if y else 0
            cc = out[y - 1, j - c] if (y and j >= c) else 0
            p = a + b - cc
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
            pred = (0, a, b, (a + b) // 2, a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc))[f[y, 0]]
            out[y, j] = (f[y, 1 + j] + pred) & 255
    assert np.array_equal(out.reshape(img.shape).astype(np.uint8), img)


def test_filter_choice_ties_go_to_the_lowest_type():
    assert R.filter_rows(np.zeros((3, 5, 3), np.uint8))[:, 0].tolist() == [0, 0, 0]
    flat = R.filter_rows(np.full((2, 700, 1), 255, np.uint8))
    assert flat[:, 0].tolist() == [1, 2]                       # Sub costs 1 (the first byte), Up costs 0 on the second row
    assert flat[0, 1] == 255 and not flat[0, 2:].any() and not flat[1, 1:].any()


@pytest.mark.parametrize("run, want", [(3, []), (4, [3]), (259, [258]), (260, [256, 3]), (261, [257, 3]), (262, [258, 3]),
                                       (517, [258, 258]), (518, [258, 256, 3]), (775, [258, 258, 258])])
def test_match_length_rule(run, want):
    toks = R.tokens([9] * run)
    lits = [t for t in toks if t[0] == "L"]
    assert [m for kind, m in toks if kind == "M"] == want
    assert lits == [("L", 9)] * (run if run < 4 else 1)
    assert len(lits) + sum(want) == run and all(3 <= m <= 258 for m in want)
    # never across rows, never across different bytes
    assert R.tokens([1] * 5 + [2] * 2 + [1] * 4) == [("L", 1), ("M", 4), ("L", 2), ("L", 2), ("L", 1), ("M", 3)]


def test_length_symbols_are_rfc_1951s():
    for m in range(3, 259):
        sym, nbits, value = R.length_symbol(m)
        k = sym - 257
        assert 0 <= k < 29 and R.LENGTH_BASE[k] + value == m and 0 <= value < (1 << nbits) and nbits == R.LENGTH_EXTRA[k]
    assert R.length_symbol(258) == (285, 0, 0) and R.length_symbol(257) == (284, 5, 30) and R.length_symbol(3) == (257, 0, 0)


def test_huffman_lengths():
    rows = R.huffman_rows()
    fib = R.huffman_lengths(rows["fib40"], 15)
    unlimited = R.huffman_lengths(rows["fib40"], 64)
    assert max(unlimited) == 39 and max(fib) == 15             # the tree is deeper than the limit; the limit holds
    assert sum(1 for n in fib if n) == 40 and sum(2.0 ** -n for n in fib if n) == 1.0
    assert all(fib[i] >= fib[i + 1] for i in range(39))        # rarer symbols never get shorter codes
    for name in ("fib33", "equal", "skew"):
        lengths = R.huffman_lengths(rows[name], 15)
        used = [n for n, f in zip(lengths, rows[name]) if f]
        assert all(1 <= n <= 15 for n in used) and sum(2.0 ** -n for n in used) == 1.0, name
        assert all(n == 0 for n, f in zip(lengths, rows[name]) if not f), name
    two = R.huffman_lengths(rows["two"], 15)
    assert two[7] == 1 and two[256] == 1 and sum(two) == 2
    single = R.huffman_lengths(rows["single_literal"], 15)
    assert single[65] == 1 and single[256] == 1 and sum(single) == 2
    assert not any(R.huffman_lengths(rows["lone"], 15)) and not any(R.huffman_lengths(rows["zeros"], 15))
    # the kernel's preconditions, and what the rows that aim at the shared table builder are for
    assert all(sum(r) < 2 ** 32 and max(r) < 2 ** 31 for r in rows.values())
    assert max(R.huffman_lengths(rows["fib45"], 64)) == 44 and max(R.huffman_lengths(rows["fib45"], 15)) == 15
    assert sum(rows["fib45"]) + rows["fib45"][44] + rows["fib45"][43] >= 2 ** 32       # a 46th Fibonacci count breaks the first
    assert {i % 64 for i, n in enumerate(rows["one_lane"]) if n} == {5} and sum(1 for n in rows["one_lane"] if n) == 5
    assert [(i, n) for i, n in enumerate(R.huffman_lengths(rows["one_lane"], 15)) if n] == [(5, 2), (69, 3), (133, 2), (197, 3), (261, 2)]
    tie = rows["butterfly_tie"]
    assert tie[0] == tie[63] == min(n for n in tie if n) and sum(1 for n in tie if n) == 3
    assert [(i, n) for i, n in enumerate(R.huffman_lengths(tie, 15)) if n] == [(0, 2), (63, 2), (130, 1)]
    # among equal frequencies the larger index merges first: 4 equal counts make a balanced tree, 3 leave the lowest short
    assert R.huffman_lengths([1, 1, 1, 1], 15) == [2, 2, 2, 2] and R.huffman_lengths([1, 1, 1], 15) == [1, 2, 2]
    codes = R.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4])          # the example of RFC 1951 section 3.2.2
    assert codes == [0b010, 0b011, 0b100, 0b101, 0b110, 0b00, 0b1110, 0b1111]


def test_code_length_code_is_complete_and_the_sequence_follows_the_rule():
    assert sum(2.0 ** -n for n in R.CLEN_LENGTHS if n) == 1.0 and R.CLEN_LENGTHS[16] == 0
    assert [s for s, n in enumerate(R.CLEN_LENGTHS) if n == 5] == [1, 2, 3, 14]
    seq = R.code_length_sequence([8] + [0] * 2 + [7] + [0] * 3 + [5] + [0] * 10 + [4] + [0] * 11 + [3] + [0] * 150 + [1])
    assert seq == [(8, 0, 0), (0, 0, 0), (0, 0, 0), (7, 0, 0), (17, 3, 0), (5, 0, 0), (17, 3, 7), (4, 0, 0), (18, 7, 0),
                   (3, 0, 0), (18, 7, 127), (18, 7, 1), (1, 0, 0)]
    assert all(s != 16 for s, _, _ in seq)


def test_adler_fold_equals_zlibs():
    data = np.random.default_rng(2).integers(0, 256, 70001, dtype=np.uint8).tobytes()
    assert R.adler32(data) == zlib.adler32(data) and R.adler32(b"") == 1


@pytest.mark.parametrize("what", ["smooth", "disc", "flat"])
def test_reference_files_are_no_longer_than_the_hosts(what):
    img = {"smooth": R.smooth(96, 80), "disc": R.disc(96, 80)[..., None], "flat": np.full((300, 700, 1), 255, np.uint8)}[what]
    h, w, c = img.shape
    mine = R.png_file(h, w, c, R.encode_stream(img))
    host = _pillow_png(img)
    print(what, "reference", len(mine), "Pillow level 1", len(host))
    assert np.array_equal(_decode(mine).reshape(img.shape), img)
    assert len(mine) <= len(host)


def test_host_wrapper_equals_the_reference_and_validates():
    from face_crop_plus_amd import pngenc
    stream = R.encode_stream(dict(CASES)["disc_17x9x3"])
    assert pngenc.png_file(17, 9, 3, stream) == R.png_file(17, 9, 3, stream)
    assert pngenc.png_file(4, 5, 1, b"abc") == R.png_file(4, 5, 1, b"abc")
    with pytest.raises(ValueError, match="channels"):
        pngenc.png_file(4, 5, 4, b"")
    with pytest.raises(ValueError, match="px"):
        pngenc.png_file(0, 5, 1, b"")
    assert pngenc.PNG_EXTENSIONS == (".png",)
    assert pngenc.supported(256, 256, 3) and pngenc.supported(1750, 1750, 3) and pngenc.supported(8192, 1000, 1)
    assert not pngenc.supported(8193, 8, 1) and not pngenc.supported(1760, 1760, 3) and not pngenc.supported(8, 8, 4)
    assert pngenc.MAX_SYMBOLS == R.MAX_SYMBOLS == 9227464 and pngenc.MAX_SIDE == R.MAX_SIDE


def test_keyword_is_validated_and_defaults_to_host():
    import inspect
    from face_crop_plus_amd import Cropper
    sig = inspect.signature(Cropper.__init__)
    assert sig.parameters["png_encoder"].default == "host" and sig.parameters["encoder"].default == "host"
    for bad in ("gpu", "", None, "Device"):
        with pytest.raises(ValueError, match="png_encoder"):
            Cropper(png_encoder=bad, det_threshold=None)
    assert hasattr(Cropper, "encode_png") and hasattr(Cropper, "_is_png_target")


def test_cli_parses_penc():
    from face_crop_plus_amd.__main__ import parse_args
    assert "png_encoder" not in parse_args(["-i", "x"])
    assert parse_args(["-i", "x", "-penc", "device"])["png_encoder"] == "device"
    assert parse_args(["-i", "x", "--png-encoder", "host"])["png_encoder"] == "host"
    with pytest.raises(SystemExit):
        parse_args(["-i", "x", "-penc", "gpu"])


def test_bindings_exist():
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import torch_ops as T
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    lib = N.lib()
    for name in ("fcp_png_workspace_bytes", "fcp_png_encode_u8", "fcp_png_huffman_lengths"):
        assert name in N.EXPORTS and name + "(" in hdr and hasattr(lib, name)
    assert "png_encode" in T.OPS and "png_huffman_lengths" in T.OPS
    if os.path.isfile(T.LIB_PATH):
        ops = T.load()
        assert hasattr(ops, "png_encode") and hasattr(ops, "png_huffman_lengths")
    # the refusals of the sizing call need no GPU
    assert lib.fcp_png_workspace_bytes(1, 8, 8, 3) > 0
    for args, word in (((1, 0, 8, 3), b"bad sizes"), ((1, 8, 8, 2), b"channels"), ((1, 8193, 8, 1), b"8192"),
                       ((1, 1760, 1760, 3), b"9227464"), ((65536, 8, 8, 1), b"65535")):
        assert lib.fcp_png_workspace_bytes(*args) == -1, args
        assert word in lib.fcp_last_error(), (args, lib.fcp_last_error())
    assert lib.fcp_png_workspace_bytes(1, 1750, 1750, 3) > 0
