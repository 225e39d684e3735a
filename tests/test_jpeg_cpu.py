"""Cropper(encoder="device") without a GPU: the restatement tests/jpeg_ref.py equals Pillow (libjpeg-turbo) byte for byte on
the whole case list, at run time and against the recorded tests/golden/jpeg_streams.npz; it emits ZRL where the list says
so; jpegenc.jpeg_header is the file's prefix; the C entry point refuses bad arguments before any device work; the op, the
constructor argument, the CLI flag and the bytes-write task of the I/O pool."""
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
    spec = importlib.util.spec_from_file_location("_jpeg_ref", os.path.join(os.path.dirname(__file__), "jpeg_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
CASES = R.cases()
IDS = [f"{k}_{h}x{w}x{c}" for k, h, w, c in CASES]


def _pillow(img, quality=None):
    from PIL import Image
    from face_crop_plus_amd._io_codec import _ENCODER_KW
    kw = dict(_ENCODER_KW[".jpg"])
    if quality is not None:
        kw["quality"] = quality
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, **kw)
    return buf.getvalue()


def _need_turbo():
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("this Pillow is not built on libjpeg-turbo: its bytes are not the contract (the fixture still is)")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_streams.npz"))


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    return N


def test_case_list_is_the_issues():
    assert R.SIZES == [(1, 1), (8, 8), (16, 16), (17, 9), (9, 17), (24, 40), (37, 53), (96, 80), (112, 112), (256, 256)]
    assert R.CONTENTS == ["constant", "ramp", "noise", "checker", "impulses"]
    for h, w in R.SIZES:
        for ch in (1, 3):
            kinds = [k for k, hh, ww, c in CASES if (hh, ww, c) == (h, w, ch)]
            assert kinds == (R.CONTENTS if (h, w) != (256, 256) else ["noise"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_pillow(case):
    _need_turbo()
    kind, h, w, ch = case
    img = R.content(kind, h, w, ch)
    assert img.dtype == np.uint8 and img.shape == ((h, w, 3) if ch == 3 else (h, w))
    assert R.encode(img) == _pillow(img)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_fixture(golden, case):
    kind, h, w, ch = case
    key = f"{kind}_{h}x{w}x{ch}"
    img = R.content(kind, h, w, ch)
    if "in_" + key in golden:
        assert np.array_equal(golden["in_" + key], img)
    else:
        assert int(golden["crc_" + key]) == zlib.crc32(img.tobytes())
    assert R.encode(img) == golden["jpg_" + key].tobytes()


def test_fixture_names_its_libraries(golden):
    versions = [str(v) for v in golden["versions"]]
    assert any(v.startswith("Pillow ") for v in versions) and any(v.startswith("libjpeg-turbo ") for v in versions)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_streams.npz")) < 512 * 1024


@pytest.mark.parametrize("quality", [1, 10, 49, 50, 75, 100])
def test_restatement_equals_pillow_at_other_qualities(quality):
    _need_turbo()
    for ch in (1, 3):
        for kind in ("noise", "ramp"):
            img = R.content(kind, 37, 53, ch)
            assert R.encode(img, quality) == _pillow(img, quality), (kind, ch)


def test_contents_reach_the_paths_they_are_listed_for():
    """The impulses content really gives ZRL symbols, noise stuffed FFs (24 of them in the 96x80 RGB case), constant
    blocks nothing but end-of-block, the odd block grids dummy blocks."""
    for h, w in R.SIZES:
        if h < 8 or w < 8 or (h, w) == (256, 256):
            continue
        for ch in (1, 3):
            stats = {}
            R.encode_scan(R.content("impulses", h, w, ch), 95, stats)
            assert stats["zrl"] > 0, (h, w, ch)
    stats = {}
    R.encode_scan(R.content("noise", 96, 80, 3), 95, stats)
    assert stats["stuffed"] == 24
    coefs = R.coefficients(R.content("constant", 24, 40, 3))
    assert all((c[..., 1:] == 0).all() for c in coefs)
    for (h, w), dummies in (((17, 9), 2), ((9, 17), 2), ((24, 40), 9), ((16, 16), 0)):
        blocks = R.scan_blocks(R.coefficients(R.content("ramp", h, w, 3)))
        assert sum(b is None for _, b in blocks) == dummies, (h, w)
    # the checker's DC differences are the largest there are: -512 <-> 508 at quality 95 (size category 10), category 11,
    # the last one, at quality 100
    for quality, size in ((95, 10), (100, 11)):
        zz = R.coefficients(R.content("checker", 16, 16, 1), quality)[0][..., 0].reshape(-1)
        assert int(np.abs(np.diff(zz)).max()).bit_length() == size


def test_reciprocal_quantisation_equals_the_division():
    """libjpeg-turbo multiplies by a 16-bit reciprocal instead of dividing; for every divisor 8..2040 and every magnitude a
    DCT coefficient can have that is the rounded division the restatement and the kernel use (the Pillow comparison above
    proves it on data; this spells the arithmetic out: reciprocal r = ceil-ish 2^(16+s) / d with correction c)."""
    mags = np.arange(0, 1 << 15, dtype=np.int64)
    for d in list(range(8, 2041, 8)):
        b = d.bit_length() - 1
        r = b + 16
        fq = (1 << r) // d
        fr = (1 << r) % d
        c = d // 2
        if fr == 0:
            fq >>= 1
            r -= 1
        elif fr <= d // 2:
            c += 1
        else:
            fq += 1
        if d == 1:
            continue
        got = ((mags + c) * fq) >> r
        assert np.array_equal(got, (mags + d // 2) // d), d


@pytest.mark.parametrize("channels", [1, 3])
def test_jpeg_header_is_what_pillow_writes_before_the_scan(golden, channels):
    from face_crop_plus_amd import jpegenc
    assert jpegenc.QUALITY == 95 and jpegenc.SUBSAMPLING == 2
    assert sorted(jpegenc.JPEG_EXTENSIONS) == [".jpe", ".jpeg", ".jpg"]
    for kind, h, w, ch in CASES:
        if ch != channels:
            continue
        head = jpegenc.jpeg_header(h, w, ch, 95)
        assert head == R.header(h, w, ch, 95)
        assert head[-14 if ch == 3 else -10:-12 if ch == 3 else -8] == b"\xff\xda"          # ends with the SOS segment
        assert golden[f"jpg_{kind}_{h}x{w}x{ch}"].tobytes().startswith(head)
        assert _pillow(R.content(kind, h, w, ch)).startswith(head)
    for quality in (1, 30, 50, 100):
        img = R.content("ramp", 24, 40, channels)
        assert _pillow(img, quality).startswith(jpegenc.jpeg_header(24, 40, channels, quality))
    for bad in ((8, 8, 2, 95), (8, 8, 3, 0), (8, 8, 3, 101), (0, 8, 3, 95), (8, 65536, 1, 95)):
        with pytest.raises(ValueError):
            jpegenc.jpeg_header(*bad)


# ---- the C boundary and the op
def test_abi_declares_the_entry_points(native):
    import ctypes
    import re
    N = native
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    params = [p.strip() for p in norm(re.search(r"int fcp_jpeg_encode_u8\(([^)]*)\)", hdr).group(1)).split(",")]
    assert params == ["const uint8_t* crops", "int f", "int h", "int w", "int channels", "int quality", "int subsampling",
                      "uint8_t* out", "int64_t out_stride", "int64_t capacity", "int32_t* lengths", "void* workspace",
                      "int64_t workspace_bytes", "fcp_stream_t stream"]
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert N.SIGNATURES["fcp_jpeg_encode_u8"] == [P, I, I, I, I, I, I, P, L, L, P, P, L, P]
    assert "fcp_jpeg_encode_u8" in N.EXPORTS and "fcp_jpeg_workspace_bytes" in N.EXPORTS
    assert "20 + 63 * 26" in hdr                   # the worst case of a block is documented where the capacity is


def test_entry_point_refuses_bad_arguments_before_any_device_work(native):
    lib = native.lib()
    ok = dict(f=1, h=8, w=8, c=3, q=95, ss=2, stride=64, cap=64, wsb=1 << 20)
    for change, word in (({"h": 0}, b"bad sizes"), ({"w": 0}, b"bad sizes"), ({"f": -1}, b"bad sizes"), ({"c": 2}, b"channels"),
                         ({"c": 4}, b"channels"), ({"h": 8193}, b"8192"), ({"w": 8193}, b"8192"), ({"f": 65536}, b"65535"),
                         ({"q": 0}, b"quality"), ({"q": 101}, b"quality"), ({"ss": 0}, b"4:2:0"), ({"ss": 1}, b"4:2:0"),
                         ({"cap": -1}, b"capacity"), ({"cap": 65}, b"capacity")):
        a = dict(ok, **change)
        rc = lib.fcp_jpeg_encode_u8(None, a["f"], a["h"], a["w"], a["c"], a["q"], a["ss"], None, a["stride"], a["cap"], None,
                                    None, a["wsb"], None)
        assert rc < 0, change
        assert word in lib.fcp_last_error(), (change, lib.fcp_last_error())
    assert lib.fcp_jpeg_encode_u8(None, 1, 8, 8, 3, 95, 2, None, 64, 64, None, None, 1 << 20, None) < 0
    assert b"null pointer" in lib.fcp_last_error()
    assert lib.fcp_jpeg_encode_u8(None, 0, 8, 8, 3, 95, 2, None, 64, 64, None, None, 0, None) == 0      # f == 0: a no-op
    assert lib.fcp_jpeg_workspace_bytes(1, 8, 8, 2) == -1 and lib.fcp_jpeg_workspace_bytes(1, 0, 8, 3) == -1
    # coefficients (128 bytes a block) + bit offsets (4) + the unstuffed bits (1658 bits a block at most); 6 blocks per MCU
    for f, h, w, c, blocks in ((1, 8, 8, 1, 1), (3, 17, 9, 3, 12), (2, 256, 256, 3, 1536), (1, 37, 53, 1, 35)):
        need = lib.fcp_jpeg_workspace_bytes(f, h, w, c)
        least = f * (blocks * (128 + 4) + -(-blocks * 1658 // 8))
        assert least <= need <= least + 64 * f + 64, (f, h, w, c, need)


def test_op_is_registered_and_refuses_cpu_tensors(native):
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    assert "jpeg_encode" in T.OPS
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcp::jpeg_encode", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcp::jpeg_encode", "CPU")
    assert str(torch.ops.fcp.jpeg_encode.default._schema) == \
        "fcp::jpeg_encode(Tensor crops, int quality, int subsampling, Tensor(a!) out) -> Tensor"
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.jpeg_encode(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 95, 2, torch.zeros(1, 64, dtype=torch.uint8))


# ---- Cropper arguments, CLI, the write task
def test_cropper_checks_encoder_without_a_device(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    assert inspect.signature(Cropper).parameters["encoder"].default == "host"
    for bad in ("gpu", "Device", "", None, 1):
        with pytest.raises(ValueError, match="encoder"):
            Cropper(encoder=bad)
    for good in ("host", "device"):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(encoder=good)
    assert callable(Cropper.encode_jpeg)


def test_cli_encoder_flag(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    assert parse_args(["-i", str(tmp_path), "-enc", "device"])["encoder"] == "device"
    assert parse_args(["-i", str(tmp_path), "--encoder", "host"])["encoder"] == "host"
    assert "encoder" not in parse_args(["-i", str(tmp_path)])
    with pytest.raises(SystemExit):
        parse_args(["-i", str(tmp_path), "-enc", "gpu"])
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"encoder": "device"}))
    assert parse_args(["-i", str(tmp_path), "-c", str(cfg)])["encoder"] == "device"


def test_target_extension_rule():
    from face_crop_plus_amd import Cropper
    c = Cropper.__new__(Cropper)
    c.output_format = None
    assert c._is_jpeg_target(np.array(["a.jpg", "b.JPEG", "c.Jpe", "d.png", "e", "f.jpg.webp"])).tolist() == \
        [True, True, True, False, False, False]
    c.output_format = "JPG"
    assert c._is_jpeg_target(np.array(["a.png", "b.jpg"])).tolist() == [True, True]
    c.output_format = "png"
    assert c._is_jpeg_target(np.array(["a.jpg"])).tolist() == [False]


def test_bytes_write_task_of_the_io_pool(tmp_path):
    """Encoded files are only written: inline, and by a worker process, through a temporary name; a failed write leaves
    nothing behind and surfaces as an error."""
    from face_crop_plus_amd._io_codec import write_bytes
    from face_crop_plus_amd._io_pool import IOProcesses
    data = R.encode(R.content("ramp", 17, 9, 3))
    assert write_bytes(str(tmp_path / "a.jpg"), data) and (tmp_path / "a.jpg").read_bytes() == data
    with pytest.raises(OSError):
        write_bytes(str(tmp_path / "missing" / "a.jpg"), data)
    pool = IOProcesses(1, 1, ring_mb=1)
    try:
        assert pool.write_bytes(str(tmp_path / "b.jpg"), data) is True
        assert (tmp_path / "b.jpg").read_bytes() == data
        with pytest.raises(RuntimeError, match="I/O worker"):
            pool.write_bytes(str(tmp_path / "missing" / "b.jpg"), data)
        assert pool.write(str(tmp_path / "c.png"), R.content("ramp", 8, 8, 3)) is True     # the pixel task still works after it
    finally:
        pool.close()
    assert sorted(os.listdir(tmp_path)) == ["a.jpg", "b.jpg", "c.png"]
