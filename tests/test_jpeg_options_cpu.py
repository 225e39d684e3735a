"""Cropper(jpeg_quality=, jpeg_subsampling=, jpeg_optimize=) without a GPU: the restatement tests/jpeg_options_ref.py equals
Pillow (libjpeg-turbo) byte for byte on the whole case list, at run time and against the recorded
tests/golden/jpeg_options.npz; libjpeg's limit of the code lengths to 16 bits is reached and pinned; jpegenc.jpeg_header
is the file's prefix for every subsampling and for optimised tables; the host writers write Pillow's bytes for the
settings, the file that outgrows Pillow's buffer included; the new C entry points refuse bad arguments before any device
work; the ops, the constructor arguments, the CLI flags.

Every test fails without the feature: the keywords, the entry points and the ops do not exist there."""
import importlib.util
import inspect
import io
import json
import os
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("_jpeg_options_ref", os.path.join(os.path.dirname(__file__), "jpeg_options_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


O = _load()
R = O.R
CASES = O.cases()
GROUPS = sorted({(h, w, ch, ss) for _, h, w, ch, ss, _, _ in CASES})
_ENCODED = {}


def _encoded(case):
    """The restatement's file of a case, computed once for the Pillow and the fixture comparison."""
    if case not in _ENCODED:
        kind, h, w, ch, ss, opt, q = case
        _ENCODED[case] = O.encode(R.content(kind, h, w, ch), q, ss, opt)
    return _ENCODED[case]


def _need_turbo():
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo: its bytes are not the contract (the fixture still is)")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_options.npz"))


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    return N


def _golden_equals(golden, case, data):
    key = O.case_key(case)
    if "jpg_" + key in golden:
        return golden["jpg_" + key].tobytes() == data
    return golden["sum_" + key].tolist() == [len(data), zlib.crc32(data)]


def test_case_list_is_the_issues():
    assert O.SIZES == [(1, 1), (8, 8), (16, 16), (17, 9), (9, 17), (24, 40), (37, 53), (96, 80), (112, 112)]
    assert R.CONTENTS == ["constant", "ramp", "noise", "checker", "impulses"]
    assert O.MODES == [(3, "4:4:4"), (3, "4:2:2"), (3, "4:2:0"), (1, "4:2:0")]
    assert len(CASES) == len(set(CASES)) == 9 * 5 * 4 * 2 + 2 * 5 * 4 * 2 * 3
    for h, w in O.SIZES:
        qs = sorted({q for _, hh, ww, _, _, _, q in CASES if (hh, ww) == (h, w)})
        assert qs == ([1, 50, 95, 100] if (h, w) in ((17, 9), (37, 53)) else [95])
    assert {opt for *_, opt, _ in CASES} == {False, True}


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"{g[0]}x{g[1]}x{g[2]}_{g[3].replace(':', '')}")
def test_restatement_equals_pillow(group):
    _need_turbo()
    for case in CASES:
        kind, h, w, ch, ss, opt, q = case
        if (h, w, ch, ss) == group:
            assert _encoded(case) == O.pillow(R.content(kind, h, w, ch), q, ss, opt), case


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: f"{g[0]}x{g[1]}x{g[2]}_{g[3].replace(':', '')}")
def test_restatement_equals_fixture(golden, group):
    for case in CASES:
        kind, h, w, ch, ss, opt, q = case
        if (h, w, ch, ss) != group:
            continue
        img = R.content(kind, h, w, ch)
        key = f"{kind}_{h}x{w}x{ch}"
        if "in_" + key in golden:
            assert np.array_equal(golden["in_" + key], img)
        else:
            assert int(golden["crc_" + key]) == zlib.crc32(img.tobytes())
        assert _golden_equals(golden, case, _encoded(case)), case
        if ss == "4:2:0" and not opt:                       # the default settings: the restatement this one extends
            assert _encoded(case) == R.encode(img, q), case


def test_fixture_names_its_libraries(golden):
    versions = [str(v) for v in golden["versions"]]
    assert any(v.startswith("Pillow ") for v in versions) and any(v.startswith("libjpeg-turbo ") for v in versions)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_options.npz")) < 512 * 1024


def test_gray_subsampling_changes_one_byte():
    """Pillow writes the sampling byte of the lone gray component after the subsampling; the scan does not change."""
    _need_turbo()
    img = R.content("ramp", 17, 9, 1)
    files = [O.pillow(img, 95, ss, True) for ss in O.SUBSAMPLINGS]
    at = files[2].index(b"\xff\xc0") + 11
    assert [f[at] for f in files] == [0x11, 0x21, 0x22]
    assert all(f[:at] + f[at + 1:] == files[2][:at] + files[2][at + 1:] for f in files)
    assert [O.encode(img, 95, ss, True) for ss in O.SUBSAMPLINGS] == files


# ---- the limit of the code lengths to 16 bits
@pytest.mark.parametrize("shift,nsym,size,depth", [(0, 19, 10606, 12), (1, 18, 10716, 19)], ids=["issue", "one_chain"])
def test_length_limit_images(golden, shift, nsym, size, depth):
    """(0, 19) is the image of the feature's issue: every block quantises as intended and the optimised file is Pillow's,
    10 606 bytes.  The issue also says its tree is deeper than 16 before the limit; it is not — libjpeg breaks ties
    towards single symbols, the pseudo-symbol and the first 1 start two interleaved chains, and the tree is 12 deep (pinned
    here so that nobody takes this image for a test of the limit).  (1, 18), counts 1, 2, 3, 5, ... on the same
    construction, is one chain: 19 deep before the limit.  It is the image that cannot pass without the limiting branch,
    and all three things are asserted of it: the symbols, Pillow's bytes, the depth."""
    img, want = O.fibonacci_image(shift, nsym)
    assert img.shape == (840, 840) and int(golden[f"crc_fibonacci_{shift}_{nsym}"]) == zlib.crc32(img.tobytes())
    freq = O.histograms(O.block_symbols(O.scan_blocks(O.coefficients(img, 50))))
    assert {int(s): int(freq[1, s]) for s in np.nonzero(freq[1])[0]} == want and want[0] == 11025
    assert freq[0].tolist() == [11025] + [0] * 255 and not freq[2:].any()
    info = {}
    counts, symbols = O.gen_optimal_table(freq[1], info)
    print("depth before the limit", info["depth"], "counts", counts)
    assert info["depth"] == depth and sum(counts) == nsym + 1 and len(symbols) == nsym + 1
    if depth > 16:
        assert counts[15] > 0                               # codes were moved up to 16 bits
    mine = O.encode(img, 50, "4:2:0", True)
    assert len(mine) == size and mine == golden[f"jpg_fibonacci_{shift}_{nsym}"].tobytes()
    from PIL import features
    if features.check_feature("libjpeg_turbo"):
        assert mine == O.pillow(img, 50, "4:2:0", True)


def test_optimal_tables_of_special_rows():
    one = np.zeros(256, np.int64)
    one[7] = 5
    assert O.gen_optimal_table(one) == ([1] + [0] * 15, [7])
    two = np.zeros(256, np.int64)
    two[[3, 200]] = 9
    assert O.gen_optimal_table(two) == ([1, 1] + [0] * 14, [3, 200])           # the tie goes to the larger index: 200 joins the pseudo-symbol, one level down
    assert O.gen_optimal_table(np.zeros(256, np.int64)) == ([0] * 16, [])
    counts, symbols = O.gen_optimal_table(np.ones(256, np.int64))
    assert sum(counts) == 256 and sorted(symbols) == list(range(256)) and counts[7] == 255 and counts[8] == 1
    for nsym, shift, depth in ((19, 0, 11), (25, 0, 14), (30, 0, 16), (19, 1, 19), (25, 1, 25), (30, 1, 30)):
        info = {}
        counts, symbols = O.gen_optimal_table(O.fibonacci_row(nsym, shift), info)
        assert info["depth"] == depth and sum(counts) == nsym and O.fibonacci_row(nsym, shift).sum() < O.FIB35 - 1
        assert sum(c * 2 ** (16 - n) for n, c in enumerate(counts, 1)) < 2 ** 16          # Kraft, with room for the pseudo-symbol


# ---- the header
@pytest.mark.parametrize("channels", [1, 3])
def test_jpeg_header_is_the_prefix_for_every_setting(golden, channels):
    from face_crop_plus_amd import jpegenc
    assert jpegenc.TABLE_BYTES == 272
    for case in CASES:
        kind, h, w, ch, ss, opt, q = case
        if ch != channels or (h, w) not in ((17, 9), (37, 53), (24, 40)) or kind not in ("ramp", "constant", "noise"):
            continue
        img = R.content(kind, h, w, ch)
        tables = O.tables_of(img, q, ss, opt)
        record = b"".join(O.table_record(t) for t in tables) if opt else None
        if opt and ch == 1:
            assert record[2 * 272:] == bytes(2 * 272)
        head = jpegenc.jpeg_header(h, w, ch, q, subsampling=ss, tables=record)
        assert head == jpegenc.jpeg_header(h, w, ch, q, subsampling=O.sub_index(ss),
                                           tables=None if record is None else np.frombuffer(record, np.uint8).reshape(4, 272))
        assert head == O.header(h, w, ch, q, ss, tables)
        assert golden["jpg_" + O.case_key(case)].tobytes().startswith(head), case
        assert head + O.encode_scan(img, q, ss, opt) == golden["jpg_" + O.case_key(case)].tobytes()
        if ss == "4:2:0" and not opt:
            assert head == jpegenc.jpeg_header(h, w, ch, q)
    for k, ss in enumerate(O.SUBSAMPLINGS):                  # the gray SOF byte follows the subsampling
        head = jpegenc.jpeg_header(8, 8, 1, 95, subsampling=ss)
        assert head[head.index(b"\xff\xc0") + 11] == (0x11, 0x21, 0x22)[k]
    assert jpegenc.jpeg_header(8, 8, 3, 95, subsampling=2, tables=None) == jpegenc.jpeg_header(8, 8, 3, 95) == R.header(8, 8, 3, 95)
    for bad in ("4:1:1", 3, -1, None, True):
        with pytest.raises((ValueError, TypeError)):
            jpegenc.jpeg_header(8, 8, 3, 95, subsampling=bad)


# ---- the host writers
NOISE_444 = dict(quality=95, subsampling="4:4:4", optimize=True)


def _noise256():
    return R.content("noise", 256, 256, 3)


def test_naive_pillow_save_fails_where_the_writer_must_not():
    """The trap the writer has to avoid: 132 534 bytes do not fit the 131 072 Pillow gives libjpeg."""
    from PIL import Image, ImageFile
    assert ImageFile.MAXBLOCK < 132534
    with pytest.raises(OSError):
        Image.fromarray(_noise256()).save(io.BytesIO(), format="JPEG", **NOISE_444)


def test_write_image_with_jpeg_settings(tmp_path):
    _need_turbo()
    from PIL import ImageFile
    from face_crop_plus_amd._io_codec import JpegSettings, _ENCODER_KW, write_image
    from face_crop_plus_amd import jpegenc
    before = ImageFile.MAXBLOCK
    img = _noise256()
    want = O.encode(img, 95, "4:4:4", True)
    assert len(want) == 132534
    for ext in (".jpg", ".jpeg", ".jpe"):
        path = str(tmp_path / ("noise" + ext))
        assert write_image(path, img, jpeg=JpegSettings(**NOISE_444)) is True
        assert open(path, "rb").read() == want
        assert ImageFile.MAXBLOCK == before
    assert jpegenc._host_jpeg(img, 95, 0, True) == want and ImageFile.MAXBLOCK == before
    for ch in (3, 1):
        small = R.content("ramp", 37, 53, ch)
        for q, ss, opt in ((90, "4:4:4", True), (50, "4:2:2", False), (100, "4:2:0", True), (1, "4:2:2", True)):
            path = str(tmp_path / f"s{ch}.jpg")
            assert write_image(path, small, jpeg=(q, ss, opt))            # a plain tuple is as good
            assert open(path, "rb").read() == O.encode(small, q, ss, opt) == O.pillow(small, q, ss, opt)
            assert jpegenc._host_jpeg(small, q, ss, opt) == O.encode(small, q, ss, opt)
    # no settings: the table entry, as before; other formats never see them
    small = R.content("ramp", 37, 53, 3)
    write_image(str(tmp_path / "d.jpg"), small)
    assert open(tmp_path / "d.jpg", "rb").read() == R.encode(small)
    write_image(str(tmp_path / "a.png"), small)
    write_image(str(tmp_path / "b.png"), small, jpeg=JpegSettings(**NOISE_444))
    assert open(tmp_path / "a.png", "rb").read() == open(tmp_path / "b.png", "rb").read()
    assert _ENCODER_KW[".jpg"] == dict(format="JPEG", quality=95, subsampling="4:2:0")
    assert ImageFile.MAXBLOCK == before


def test_write_task_of_the_io_pool_carries_the_settings(tmp_path):
    _need_turbo()
    from face_crop_plus_amd._io_codec import JpegSettings
    from face_crop_plus_amd._io_pool import IOProcesses
    img, small = _noise256(), R.content("ramp", 17, 9, 1)
    pool = IOProcesses(1, 1, ring_mb=1)
    try:
        assert pool.write(str(tmp_path / "n.jpg"), img, JpegSettings(**NOISE_444)) is True
        assert pool.write(str(tmp_path / "g.jpeg"), small, jpeg=JpegSettings(50, "4:2:2", True)) is True
        assert pool.write(str(tmp_path / "d.jpg"), small) is True                    # and again: the buffer size was restored
        assert pool.write(str(tmp_path / "n2.jpg"), img, JpegSettings(**NOISE_444)) is True
    finally:
        pool.close()
    assert (tmp_path / "n.jpg").read_bytes() == (tmp_path / "n2.jpg").read_bytes() == O.encode(img, 95, "4:4:4", True)
    assert (tmp_path / "g.jpeg").read_bytes() == O.encode(small, 50, "4:2:2", True)
    assert (tmp_path / "d.jpg").read_bytes() == R.encode(small)


# ---- the C boundary and the ops
def test_abi_declares_the_entry_points(native):
    import ctypes
    import re
    N = native
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    norm = lambda s: re.sub(r"\s+", " ", s).strip()

    def params(ret, name):
        return [p.strip() for p in norm(re.search(ret + r" " + name + r"\(([^)]*)\)", hdr).group(1)).split(",")]
    assert params("int64_t", "fcp_jpeg_workspace_bytes_ex") == ["int f", "int h", "int w", "int channels", "int subsampling",
                                                               "int optimize"]
    assert params("int", "fcp_jpeg_encode_ex_u8") == [
        "const uint8_t* crops", "int f", "int h", "int w", "int channels", "int quality", "int subsampling", "int optimize",
        "uint8_t* out", "int64_t out_stride", "int64_t capacity", "int32_t* lengths", "uint8_t* tables", "void* workspace",
        "int64_t workspace_bytes", "fcp_stream_t stream"]
    assert params("int", "fcp_jpeg_huffman_tables") == ["const uint32_t* freq", "int n", "uint8_t* tables", "uint32_t* codes",
                                                        "fcp_stream_t stream"]
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert N.SIGNATURES["fcp_jpeg_encode_ex_u8"] == [P, I, I, I, I, I, I, I, P, L, L, P, P, P, L, P]
    assert N.SIGNATURES["fcp_jpeg_huffman_tables"] == [P, I, P, P, P]
    assert N.SIGNATURES["fcp_jpeg_encode_u8"] == [P, I, I, I, I, I, I, P, L, L, P, P, L, P]
    for name in ("fcp_jpeg_encode_ex_u8", "fcp_jpeg_huffman_tables", "fcp_jpeg_workspace_bytes_ex"):
        assert name in N.EXPORTS
    assert N.ABI_VERSION == 15 and "#define FCP_ABI_VERSION 15" in hdr
    assert "27 + 63 * 26" in hdr and "20 + 63 * 26" in hdr and "9 227 465" in hdr


def _ex(lib, **kw):
    a = dict(f=1, h=8, w=8, c=3, q=95, ss=0, opt=0, stride=64, cap=64, wsb=1 << 20)
    a.update(kw)
    return lib.fcp_jpeg_encode_ex_u8(None, a["f"], a["h"], a["w"], a["c"], a["q"], a["ss"], a["opt"], None, a["stride"], a["cap"],
                                     None, None, None, a["wsb"], None)


def test_new_entry_points_refuse_bad_arguments_before_any_device_work(native):
    lib = native.lib()
    for change, word in (({"h": 0}, b"bad sizes"), ({"w": 0}, b"bad sizes"), ({"f": -1}, b"bad sizes"), ({"c": 2}, b"channels"),
                         ({"c": 4}, b"channels"), ({"h": 8193}, b"8192"), ({"w": 8193}, b"8192"), ({"f": 65536}, b"65535"),
                         ({"q": 0}, b"quality"), ({"q": 101}, b"quality"), ({"ss": -1}, b"subsampling"), ({"ss": 3}, b"subsampling"),
                         ({"opt": 2}, b"optimize"), ({"opt": -1}, b"optimize"), ({"cap": -1}, b"capacity"),
                         ({"cap": 65}, b"capacity"),
                         ({"h": 8192, "w": 8192}, b"32-bit bit offsets"),                 # 4:4:4: 3 * 1024 * 1024 blocks
                         ({"h": 2480, "w": 2496, "ss": 2, "opt": 1}, b"optimised tables"),
                         ({"h": 1760, "w": 1760, "opt": 1}, b"optimised tables")):
        assert _ex(lib, **change) < 0, change
        assert word in lib.fcp_last_error(), (change, lib.fcp_last_error())
    for ss in (0, 1, 2):
        for opt in (0, 1):
            assert _ex(lib, ss=ss, opt=opt) < 0 and b"null pointer" in lib.fcp_last_error()
            assert _ex(lib, ss=ss, opt=opt, f=0, wsb=0) == 0                               # f == 0: a no-op
    # optimize with every other pointer in place but tables: still refused (host addresses: nothing may touch them)
    import ctypes
    crops, out, lengths = (ctypes.create_string_buffer(256) for _ in range(3))
    work = ctypes.create_string_buffer((1 << 16) + 16)
    base = (ctypes.addressof(work) + 15) & ~15
    rc = lib.fcp_jpeg_encode_ex_u8(ctypes.addressof(crops), 1, 8, 8, 3, 95, 0, 1, ctypes.addressof(out), 64, 64,
                                   ctypes.addressof(lengths), None, base, 1 << 16, None)
    assert rc < 0 and b"tables" in lib.fcp_last_error()
    assert lib.fcp_jpeg_huffman_tables(None, 1, None, None, None) < 0 and b"null pointer" in lib.fcp_last_error()
    assert lib.fcp_jpeg_huffman_tables(None, -1, None, None, None) < 0
    assert lib.fcp_jpeg_huffman_tables(None, 0, None, None, None) == 0


def test_workspace_sizes(native):
    lib = native.lib()
    ws = lib.fcp_jpeg_workspace_bytes_ex
    assert ws(1, 8, 8, 2, 0, 0) == -1 and ws(1, 0, 8, 3, 0, 0) == -1 and ws(1, 8, 8, 3, 3, 0) == -1 and ws(1, 8, 8, 3, 0, 2) == -1
    # 32-bit bit offsets: 4:4:4 at 8192 x 8192 overflows, 4:2:2 and 4:2:0 do not
    assert ws(1, 8192, 8192, 3, 0, 0) == -1 and ws(1, 8192, 8192, 3, 1, 0) > 0 and ws(1, 8192, 8192, 3, 2, 0) > 0
    assert 3 * 1024 * 1024 * 1658 > 2 ** 32 - 1 >= 4 * 512 * 1024 * 1658
    # optimised tables: 64 * blocks + 1 < 9 227 465, i.e. at most 144 179 blocks
    assert ws(1, 2048, 2048, 3, 2, 1) > 0                                            # 6 * 128^2 = 98 304
    assert ws(1, 2480, 2480, 3, 2, 1) > 0 and ws(1, 2480, 2496, 3, 2, 1) == -1       # 6 * 155^2 = 144 150, 6 * 155 * 156 = 145 080
    assert 64 * 144150 + 1 < O.FIB35 <= 64 * 145080 + 1
    assert ws(1, 1752, 1752, 3, 0, 1) > 0 and ws(1, 1760, 1760, 3, 0, 1) == -1       # 3 * 219^2 = 143 883, 3 * 220^2 = 145 200
    assert 64 * 143883 + 1 < O.FIB35 <= 64 * 145200 + 1
    assert ws(1, 3032, 3032, 1, 0, 1) > 0 and ws(1, 3040, 3040, 1, 2, 1) == -1       # gray: 379^2 = 143 641, 380^2 = 144 400
    # the defaults are the old sizer
    for f, h, w, c in ((1, 8, 8, 1), (3, 17, 9, 3), (2, 256, 256, 3), (1, 37, 53, 1)):
        assert ws(f, h, w, c, 2, 0) == lib.fcp_jpeg_workspace_bytes(f, h, w, c)
    # coefficients (128 bytes a block) + bit offsets (4) + the unstuffed bits (1658 bits a block, 1665 with optimised
    # tables) + with them the counts and the code tables (2 * 4096 bytes a face)
    for f, h, w, c, ss, blocks in ((1, 8, 8, 3, 0, 3), (3, 17, 9, 3, 0, 18), (3, 17, 9, 3, 1, 12), (3, 17, 9, 3, 2, 12),
                                   (2, 256, 256, 3, 0, 3072), (2, 256, 256, 3, 1, 2048), (1, 37, 53, 1, 1, 35), (1, 9, 17, 3, 1, 16)):
        for opt, bits in ((0, 1658), (1, 1665)):
            need = ws(f, h, w, c, ss, opt)
            least = f * (blocks * (128 + 4) + -(-blocks * bits // 8) + opt * 8192)
            assert least <= need <= least + 64 * f + 64, (f, h, w, c, ss, opt, need, least)


def test_ops_are_registered_and_refuse_cpu_tensors(native):
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    for name in ("jpeg_encode_ex", "jpeg_huffman_tables"):
        assert name in T.OPS
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"fcp::{name}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"fcp::{name}", "CPU")
    assert str(torch.ops.fcp.jpeg_encode_ex.default._schema) == \
        "fcp::jpeg_encode_ex(Tensor crops, int quality, int subsampling, Tensor(a!) out, Tensor(b!)? tables) -> Tensor"
    assert str(torch.ops.fcp.jpeg_huffman_tables.default._schema) == \
        "fcp::jpeg_huffman_tables(Tensor freq, bool with_codes) -> (Tensor, Tensor)"
    assert str(torch.ops.fcp.jpeg_encode.default._schema) == \
        "fcp::jpeg_encode(Tensor crops, int quality, int subsampling, Tensor(a!) out) -> Tensor"
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.jpeg_encode_ex(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 95, 0, torch.zeros(1, 64, dtype=torch.uint8), None)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.jpeg_huffman_tables(torch.zeros(1, 256, dtype=torch.int32), False)


# ---- Cropper arguments and the CLI
def test_cropper_checks_the_settings_without_a_device(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    sig = inspect.signature(Cropper).parameters
    assert (sig["jpeg_quality"].default, sig["jpeg_subsampling"].default, sig["jpeg_optimize"].default) == (95, "4:2:0", False)
    for bad in (0, 101, -5, True, False, 95.0, "95", None, [95]):
        with pytest.raises(ValueError, match="jpeg_quality"):
            Cropper(jpeg_quality=bad)
    for bad in ("4:1:1", "444", "", None, 2, "4:2:0 "):
        with pytest.raises(ValueError, match="jpeg_subsampling"):
            Cropper(jpeg_subsampling=bad)
    for bad in (0, 1, "yes", None):
        with pytest.raises(ValueError, match="jpeg_optimize"):
            Cropper(jpeg_optimize=bad)
    for good in (dict(), dict(jpeg_quality=1), dict(jpeg_quality=100, jpeg_subsampling="4:4:4", jpeg_optimize=True),
                 dict(jpeg_subsampling="4:2:2"), dict(jpeg_quality=np.int64(80))):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(**good)


def test_cropper_hands_its_settings_to_both_encoders(monkeypatch, tmp_path):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    from face_crop_plus_amd._io_codec import JpegSettings
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.Cropper, "_init_landmarks_target", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    c = Cropper(jpeg_quality=90, jpeg_subsampling="4:4:4", jpeg_optimize=True)
    assert c.jpeg == JpegSettings(90, "4:4:4", True) and (c.jpeg_quality, c.jpeg_subsampling, c.jpeg_optimize) == (90, "4:4:4", True)
    assert c._jpeg_kw() == dict(quality=90, subsampling="4:4:4", optimize=True)
    img = R.content("ramp", 37, 53, 3)
    c._emit(str(tmp_path / "a.jpg"), img)
    c._emit(str(tmp_path / "a.png"), img)
    assert (tmp_path / "a.jpg").read_bytes() == O.encode(img, 90, "4:4:4", True)
    d = Cropper()
    assert d.jpeg == JpegSettings() and d._jpeg_kw() == {}           # the defaults: the calls are the ones they always were
    d._emit(str(tmp_path / "d.jpg"), img)
    d._emit(str(tmp_path / "d.png"), img)
    assert (tmp_path / "d.jpg").read_bytes() == R.encode(img)
    assert (tmp_path / "d.png").read_bytes() == (tmp_path / "a.png").read_bytes()


def test_cli_flags_and_config_keys(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    got = parse_args(base + ["-jq", "90", "-jss", "4:4:4", "-jo"])
    assert (got["jpeg_quality"], got["jpeg_subsampling"], got["jpeg_optimize"]) == (90, "4:4:4", True)
    got = parse_args(base + ["--jpeg-quality", "50", "--jpeg-subsampling", "4:2:2", "--jpeg-optimize"])
    assert (got["jpeg_quality"], got["jpeg_subsampling"], got["jpeg_optimize"]) == (50, "4:2:2", True)
    plain = parse_args(base)
    assert not {"jpeg_quality", "jpeg_subsampling", "jpeg_optimize"} & set(plain)
    with pytest.raises(SystemExit):
        parse_args(base + ["-jss", "4:1:1"])
    with pytest.raises(SystemExit):
        parse_args(base + ["-jq", "high"])
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"jpeg_quality": 80, "jpeg-subsampling": "4:2:2", "jpeg_optimize": True}))
    got = parse_args(base + ["-c", str(cfg)])
    assert (got["jpeg_quality"], got["jpeg_subsampling"], got["jpeg_optimize"]) == (80, "4:2:2", True)
    assert parse_args(base + ["-c", str(cfg), "-jq", "70"])["jpeg_quality"] == 70
