"""Cropper(encoder="device") on the GPU: the JPEG kernels' lengths and bytes against the restatement tests/jpeg_ref.py,
Pillow at run time and the recorded fixture, byte for byte on the whole case list, through both boundaries and between
guard bytes; overflowing slots; determinism; refusals; and process_dir end to end, device against host, file by file.

Every test fails without the feature: the op, the entry point and the ``encoder`` keyword do not exist there.

The issue quotes 8047 bytes for "96x80 gray noise" without its generator; the overflow test here uses this list's own
96x80 gray noise, whose file has the length Pillow (and the fixture) give it, and asserts the same things of it: a stream
longer than the raw 7680 bytes, reported in full, with nothing written past the slot."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def _load():
    spec = importlib.util.spec_from_file_location("_jpeg_ref", os.path.join(os.path.dirname(__file__), "jpeg_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
SHAPES = [(h, w, ch) for h, w in R.SIZES for ch in (3, 1)]


def _pillow(img):
    from PIL import Image
    from face_crop_plus_amd._io_codec import _ENCODER_KW
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, **_ENCODER_KW[".jpg"])
    return buf.getvalue()


def _turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_streams.npz"))


@pytest.fixture(scope="module")
def batches():
    """(h, w, channels) -> (kinds, batch (F,h,w[,3]) u8 mixing every content of the list at that size, reference scans),
    computed once."""
    out = {}
    for h, w, ch in SHAPES:
        kinds = [k for k, hh, ww, c in R.cases() if (hh, ww, c) == (h, w, ch)]
        imgs = np.stack([R.content(k, h, w, ch) for k in kinds])
        out[(h, w, ch)] = (kinds, imgs, [R.encode_scan(im) for im in imgs])
    return out


def _encode(device, imgs, capacity, boundary, quality=95):
    """One call between guard bytes -> (lengths (F,) host, slots (F, capacity) host, the whole guarded buffer (host))."""
    from face_crop_plus_amd import jpegenc
    from face_crop_plus_amd import torch_ops as T
    f = imgs.shape[0]
    buf = torch.full((f, capacity + 2 * GUARD), 0xA5, dtype=torch.uint8, device=device)
    out = buf[:, GUARD:GUARD + capacity]
    old = T.ENABLED
    T.ENABLED = boundary == "op"
    try:
        lengths = jpegenc.encode_scans(torch.from_numpy(imgs).to(device), out, quality)
    finally:
        T.ENABLED = old
    assert lengths.dtype == torch.int32 and tuple(lengths.shape) == (f,) and lengths.device.type == "cuda"
    host = buf.cpu().numpy()
    return lengths.cpu().numpy(), host[:, GUARD:GUARD + capacity], host


def _check(lengths, slots, whole, want, capacity, what):
    assert lengths.tolist() == [len(s) for s in want], what
    for i, s in enumerate(want):
        n = min(len(s), capacity)
        assert slots[i, :n].tobytes() == s[:n], (what, i)
        assert (slots[i, n:] == 0xA5).all(), (what, i, "bytes written past the stream")
    assert (whole[:, :GUARD] == 0xA5).all() and (whole[:, GUARD + capacity:] == 0xA5).all(), (what, "guard bytes")


@pytest.mark.parametrize("boundary", ["op", "cabi"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_kernel_bytes_equal_restatement_pillow_and_fixture(device, batches, golden, shape, boundary):
    from face_crop_plus_amd import jpegenc
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    h, w, ch = shape
    kinds, imgs, want = batches[shape]
    capacity = max(len(s) for s in want) + 5                 # every stream fits, with room that has to stay untouched
    lengths, slots, whole = _encode(device, imgs, capacity, boundary)
    print(shape, boundary, "lengths", lengths.tolist(), "reference", [len(s) for s in want])
    _check(lengths, slots, whole, want, capacity, (shape, boundary))
    head = jpegenc.jpeg_header(h, w, ch)
    for i, kind in enumerate(kinds):
        got = head + slots[i, :lengths[i]].tobytes()
        assert got == golden[f"jpg_{kind}_{h}x{w}x{ch}"].tobytes(), (shape, kind, "fixture")
        if _turbo():
            assert got == _pillow(imgs[i]), (shape, kind, "Pillow")


def test_pillow_comparison_ran():
    """The run-time comparison above is skipped only where Pillow is not built on libjpeg-turbo; say so."""
    if not _turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo: compared with the fixture only")


@pytest.mark.parametrize("shape", [(17, 9, 3), (37, 53, 1), (96, 80, 3), (256, 256, 3)], ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}")
def test_streams_decode_like_pillows_own_files(device, batches, shape):
    from PIL import Image
    from face_crop_plus_amd import jpegenc
    kinds, imgs, _ = batches[shape]
    files = jpegenc.encode_jpeg(torch.from_numpy(imgs).to(device), capacity=4 * imgs[0].size + 1024)
    for i, data in enumerate(files):
        mine = np.asarray(Image.open(io.BytesIO(data)))
        assert mine.shape == imgs[i].shape
        assert np.array_equal(mine, np.asarray(Image.open(io.BytesIO(_pillow(imgs[i]))))), (shape, kinds[i])


@pytest.mark.parametrize("f", [1, 3, 65])
@pytest.mark.parametrize("channels", [3, 1])
def test_batch_sizes(device, f, channels):
    """Per-face offsets: F faces of differing content and length in one call (65: more faces than any one workgroup row)."""
    h, w = 17, 9
    imgs = np.stack([R.content(R.CONTENTS[i % 5], h, w, channels, seed=i) for i in range(f)])
    want = [R.encode_scan(im) for im in imgs]
    capacity = max(len(s) for s in want)                     # the longest fits exactly
    for boundary in ("op", "cabi"):
        lengths, slots, whole = _encode(device, imgs, capacity, boundary)
        _check(lengths, slots, whole, want, capacity, (f, channels, boundary))


@pytest.mark.parametrize("quality", [1, 50, 100])
def test_other_qualities(device, quality):
    for ch in (3, 1):
        imgs = np.stack([R.content(k, 37, 53, ch) for k in ("noise", "checker", "impulses")])
        want = [R.encode_scan(im, quality) for im in imgs]
        capacity = max(len(s) for s in want) + 3
        lengths, slots, whole = _encode(device, imgs, capacity, "cabi", quality)
        _check(lengths, slots, whole, want, capacity, (quality, ch))


def test_overflowing_slot_reports_the_true_length_and_stays_inside(device, golden):
    from face_crop_plus_amd import Cropper
    img = R.content("noise", 96, 80, 1)
    want = R.encode_scan(img)
    file = golden["jpg_noise_96x80x1"].tobytes()
    raw = img.size
    assert raw == 7680 and len(want) > raw and len(file) == len(R.header(96, 80, 1, 95)) + len(want)
    print("96x80 gray noise: file", len(file), "stream", len(want), "raw", raw)
    rgb = R.content("noise", 96, 80, 3)
    for boundary in ("op", "cabi"):
        for capacity in (raw, 1, 0, len(want) - 1):
            lengths, slots, whole = _encode(device, img[None], capacity, boundary)
            _check(lengths, slots, whole, [want], capacity, (boundary, capacity))
    # mixed with faces that fit: only the overflowing one takes the host path, the bytes are Pillow's either way
    c = Cropper(output_size=48, det_threshold=None, device="cuda:0")
    grays = np.stack([img, R.content("ramp", 96, 80, 1), R.content("noise", 96, 80, 1, seed=3)])
    files = c.encode_jpeg(grays)
    assert files[0] == file
    assert [len(x) for x in files] == [len(R.encode(g)) for g in grays] and files == [R.encode(g) for g in grays]
    assert c.encode_jpeg(rgb[None]) == [golden["jpg_noise_96x80x3"].tobytes()]
    assert c.encode_jpeg(np.zeros((0, 8, 8, 3), np.uint8)) == []
    with pytest.raises(ValueError, match="uint8"):
        c.encode_jpeg(np.zeros((1, 8, 8, 3), np.float32))


def test_two_runs_give_identical_bytes(device, batches):
    for shape in ((37, 53, 3), (112, 112, 1)):
        _, imgs, want = batches[shape]
        capacity = max(len(s) for s in want)
        a = _encode(device, imgs, capacity, "cabi")
        b = _encode(device, imgs, capacity, "cabi")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


def test_refusals_carry_a_message(device):
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import jpegenc
    from face_crop_plus_amd import torch_ops as T
    crops = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=device)
    out = torch.full((1, 64), 7, dtype=torch.uint8, device=device)
    lengths = torch.full((1,), -5, dtype=torch.int32, device=device)
    lib = N.lib()
    need = lib.fcp_jpeg_workspace_bytes(1, 8, 8, 3)
    work = torch.empty((need,), dtype=torch.uint8, device=device)

    def call(h=8, w=8, c=3, q=95, ss=2, cap=64, wsb=need, ws=work):
        return lib.fcp_jpeg_encode_u8(N.ptr(crops), 1, h, w, c, q, ss, N.ptr(out), 64, cap, N.ptr(lengths), N.ptr(ws), wsb,
                                      N.stream_ptr())
    for kw, word in ((dict(h=0), b"bad sizes"), (dict(c=2), b"channels"), (dict(q=0), b"quality"), (dict(ss=0), b"4:2:0"),
                     (dict(ss=1), b"4:2:0"), (dict(cap=65), b"capacity"), (dict(wsb=need - 1), b"workspace"),
                     (dict(w=8193), b"8192")):
        assert call(**kw) < 0, kw
        assert word in lib.fcp_last_error(), (kw, lib.fcp_last_error())
    assert lib.fcp_jpeg_encode_u8(N.ptr(crops), 1, 8, 8, 3, 95, 2, N.ptr(out), 64, 64, N.ptr(lengths), N.ptr(work, 4), need,
                                  N.stream_ptr()) < 0
    assert b"aligned" in lib.fcp_last_error()
    torch.cuda.synchronize()
    assert (out.cpu() == 7).all() and lengths.cpu().tolist() == [-5]          # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    want = R.encode_scan(np.zeros((8, 8, 3), np.uint8))
    assert lengths.cpu().tolist() == [len(want)] and out.cpu().numpy()[0, :len(want)].tobytes() == want
    ops = T.load()
    with pytest.raises(RuntimeError, match="quality"):
        ops.jpeg_encode(crops, 0, 2, out)
    with pytest.raises(RuntimeError, match="4:2:0"):
        ops.jpeg_encode(crops, 95, 0, out)
    with pytest.raises(RuntimeError, match="capacity"):
        ops.jpeg_encode(crops, 95, 2, torch.zeros((2, 64), dtype=torch.uint8, device=device))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.jpeg_encode(crops, 95, 2, torch.zeros((1, 128), dtype=torch.uint8, device=device)[:, ::2])
    with pytest.raises(RuntimeError):
        ops.jpeg_encode(crops.float(), 95, 2, out)
    empty = jpegenc.encode_scans(torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=device),
                                 torch.zeros((0, 16), dtype=torch.uint8, device=device))
    assert tuple(empty.shape) == (0,)


# ---- end to end: process_dir, device against host
def _noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _smooth(h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([127.5 + 100 * np.sin(xx / 30.0 + 0.4 * c) * np.cos(yy / 20.0 - 0.3 * c) for c in range(3)],
                    -1).round().astype(np.uint8)


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for n in files:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def photos(tmp_path_factory):
    """Three generated files (one of them a JPEG, one with two faces) and a landmark table for them."""
    from PIL import Image
    d = tmp_path_factory.mktemp("jpeg_in")
    rng = np.random.default_rng(31)
    imgs = {"a.png": _smooth(240, 320), "b.jpg": _smooth(300, 260)[:, ::-1].copy(), "c.png": _noise(rng, 200, 220)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name)
    size = (96, 80)
    tgt = A.landmarks_target(size, 0.65)
    rows, names = [], []
    for name, scale, shift in (("a.png", 1.3, (100.0, 60.0)), ("a.png", 0.9, (30.0, 20.0)), ("b.jpg", 1.6, (40.0, 90.0)),
                               ("c.png", 1.1, (50.0, 40.0))):
        rows.append(tgt * scale + np.array(shift, np.float32))
        names.append(name)
    return d, (np.stack(rows).astype(np.float32), np.array(names)), size


def _run(photos, out, **kw):
    from face_crop_plus_amd import Cropper
    d, landmarks, size = photos
    if kw.get("strategy") != "all":              # one face per file: two would race for the same file name
        first = [list(landmarks[1]).index(n) for n in sorted(set(landmarks[1]))]
        landmarks = (landmarks[0][first], landmarks[1][first])
    c = Cropper(output_size=size, landmarks=landmarks, device="cuda:0", padding="reflect_101", batch_size=2, **kw)
    c.process_dir(str(d), str(out), desc=None)
    return _tree(out)


@pytest.mark.parametrize("extra", [dict(), dict(crop_source="original", interpolation="cubic"), dict(min_sharpness=5.0)],
                         ids=["plain", "original_cubic", "min_sharpness"])
def test_process_dir_jpg_device_equals_host(device, photos, tmp_path, extra):
    host = _run(photos, tmp_path / "host", output_format="jpg", encoder="host", **extra)
    dev = _run(photos, tmp_path / "dev", output_format="jpg", encoder="device", **extra)
    assert sorted(host) and sorted(dev) == sorted(host)
    assert all(n.endswith(".jpg") for n in host)
    for n in host:
        assert dev[n] == host[n], n
    if not extra:
        assert sorted(host) == ["a.jpg", "b.jpg", "c.jpg"]
        assert len(host["c.jpg"]) > 96 * 80 * 3 // 3                 # the noise crop: a long stream, still the same file


def test_process_dir_strategy_all_with_mask_groups(device, photos, tmp_path):
    kw = dict(output_format="jpg", strategy="all", mask_groups={"all": list(range(19)), "low": list(range(10))},
              attr_groups=None, weights={"bisenet": "generated"})
    host = _run(photos, tmp_path / "host", encoder="host", **kw)
    dev = _run(photos, tmp_path / "dev", encoder="device", **kw)
    assert sorted(dev) == sorted(host)
    assert any(os.sep + "all_mask" + os.sep in os.sep + n for n in host) and any(n.endswith("a_1.jpg") for n in host)
    for n in host:
        assert dev[n] == host[n], n


def test_process_dir_other_formats_take_the_host_path(device, photos, tmp_path, monkeypatch):
    """png: nothing is encoded on the device, the files are identical; source extensions (no output_format): only the
    crop of b.jpg is a JPEG target, the others keep the host encoder, and everything is identical again."""
    from face_crop_plus_amd import jpegenc
    calls = []
    real = jpegenc.encode_jpeg
    monkeypatch.setattr(jpegenc, "encode_jpeg", lambda crops, *a, **k: (calls.append(int(crops.shape[0])), real(crops, *a, **k))[1])
    host = _run(photos, tmp_path / "host", output_format="png", encoder="host")
    assert calls == []
    dev = _run(photos, tmp_path / "dev", output_format="png", encoder="device")
    assert calls == [] and dev == host and sorted(host) == ["a.png", "b.png", "c.png"]
    host = _run(photos, tmp_path / "host2", encoder="host")
    assert calls == []
    dev = _run(photos, tmp_path / "dev2", encoder="device")
    assert sum(calls) == 1 and dev == host and sorted(host) == ["a.png", "b.jpg", "c.png"]
