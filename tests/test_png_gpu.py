"""Cropper(png_encoder="device") on the GPU: the PNG kernels' lengths and bytes against the definition in tests/png_ref.py,
byte for byte on its whole case list, through both boundaries and between guard bytes; batches; the Huffman kernel alone;
overflowing slots; determinism; refusals; Pillow decoding every file to the input; and process_dir end to end, device
against host: the same file names, the same pixels (not the same bytes: the stream is this project's own).

Every test fails without the feature: the op, the entry points and the ``png_encoder`` keyword do not exist there."""
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
    spec = importlib.util.spec_from_file_location("_png_ref", os.path.join(os.path.dirname(__file__), "png_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
CASES = R.cases()
SHAPES = sorted({img.shape for _, img in CASES})


def _decode(file):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(file)))


@pytest.fixture(scope="module")
def batches():
    """(h, w, c) -> (names, batch (F,h,w,c) u8 of every case of the list at that shape, reference streams), computed once."""
    out = {}
    for shape in SHAPES:
        names = [n for n, img in CASES if img.shape == shape]
        imgs = np.stack([img for n, img in CASES if img.shape == shape])
        out[shape] = (names, imgs, [R.encode_stream(img) for img in imgs])
    return out


def _encode(device, imgs, capacity, boundary):
    """One call between guard bytes -> (lengths (F,) host, slots (F, capacity) host, the whole guarded buffer (host)).
    (F,h,w,1) batches go in as (F,h,w): that is how masks arrive."""
    from face_crop_plus_amd import pngenc
    from face_crop_plus_amd import torch_ops as T
    f = imgs.shape[0]
    px = imgs[..., 0] if imgs.shape[-1] == 1 else imgs
    buf = torch.full((f, capacity + 2 * GUARD), 0xA5, dtype=torch.uint8, device=device)
    out = buf[:, GUARD:GUARD + capacity]
    old = T.ENABLED
    T.ENABLED = boundary == "op"
    try:
        lengths = pngenc.encode_streams(torch.from_numpy(np.ascontiguousarray(px)).to(device), out)
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
def test_kernel_bytes_equal_the_definition(device, batches, shape, boundary):
    from face_crop_plus_amd import pngenc
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    h, w, c = shape
    names, imgs, want = batches[shape]
    capacity = max(len(s) for s in want) + 5                 # every stream fits, with room that has to stay untouched
    lengths, slots, whole = _encode(device, imgs, capacity, boundary)
    print(shape, boundary, names, "lengths", lengths.tolist(), "reference", [len(s) for s in want])
    _check(lengths, slots, whole, want, capacity, (shape, boundary))
    for i, name in enumerate(names):
        file = pngenc.png_file(h, w, c, slots[i, :lengths[i]].tobytes())
        assert np.array_equal(_decode(file).reshape(imgs[i].shape), imgs[i]), name


@pytest.mark.parametrize("f", [1, 3, 65])
@pytest.mark.parametrize("channels", [3, 1])
def test_batch_sizes(device, f, channels):
    imgs = np.stack([R.content(R.KINDS[i % len(R.KINDS)], 17, 9, channels, seed=i) for i in range(f)])
    want = [R.encode_stream(im) for im in imgs]
    capacity = max(len(s) for s in want) + 1
    for boundary in ("op", "cabi"):
        lengths, slots, whole = _encode(device, imgs, capacity, boundary)
        _check(lengths, slots, whole, want, capacity, (f, channels, boundary))


def test_huffman_lengths_kernel(device):
    from face_crop_plus_amd import pngenc
    from face_crop_plus_amd import torch_ops as T
    rows = R.huffman_rows()
    names = sorted(rows)
    freq = torch.tensor([rows[n] for n in names], dtype=torch.int64).to(torch.int32).to(device)
    want = [R.huffman_lengths(rows[n], 15) for n in names]
    assert max(want[names.index("fib40")]) == 15 and all(sum(rows[n]) < 2 ** 32 for n in names)
    assert max(R.huffman_lengths(rows["fib45"], 64)) == 44            # the deepest tree a row below 2^32 makes: bound 48
    old = T.ENABLED
    try:
        for enabled in (True, False):
            T.ENABLED = enabled
            lengths, codes = pngenc.huffman_lengths(freq, with_codes=True)
            only = pngenc.huffman_lengths(freq)
            assert lengths.dtype == torch.uint8 and tuple(lengths.shape) == (len(names), 286) and torch.equal(only, lengths)
            got, got_codes = lengths.cpu().numpy(), codes.cpu().numpy().astype(np.int64) & 0xffffffff
            for i, n in enumerate(names):
                assert got[i].tolist() == want[i], (n, enabled)
                canon = R.canonical_codes(want[i]) if any(want[i]) else [0] * 286
                expect = [R.reverse_bits(c, l) | (l << 16) for c, l in zip(canon, want[i])]
                assert got_codes[i].tolist() == expect, (n, enabled, "codes")
    finally:
        T.ENABLED = old
    assert tuple(pngenc.huffman_lengths(torch.zeros((0, 286), dtype=torch.int32, device=device)).shape) == (0, 286)


def test_overflowing_slot_reports_the_true_length_and_stays_inside(device):
    from face_crop_plus_amd import Cropper, pngenc
    img = R.content("noise", 96, 80, 1)
    want = R.encode_stream(img)
    assert len(want) > img.size                                  # noise: the stream is longer than the pixels
    for boundary in ("op", "cabi"):
        for capacity in (0, 1, len(want) - 1, len(want)):
            lengths, slots, whole = _encode(device, img[None], capacity, boundary)
            _check(lengths, slots, whole, [want], capacity, (boundary, capacity))
    # mixed with faces that fit: only the overflowing one takes the host path
    grays = np.stack([img[..., 0], R.content("disc", 96, 80, 1)[..., 0], R.content("noise", 96, 80, 1, seed=3)[..., 0]])
    dev = torch.from_numpy(grays).to(device)
    refs = [R.png_file(96, 80, 1, R.encode_stream(g)) for g in grays]
    host = [pngenc._host_png(g) for g in grays]
    fits_one = len(R.encode_stream(grays[1])) + 7
    files = pngenc.encode_png(dev, capacity=fits_one)
    assert files == [host[0], refs[1], host[2]]
    assert pngenc.encode_png(dev) == refs                        # the default slot holds even noise
    c = Cropper(output_size=48, det_threshold=None, device="cuda:0")
    assert c.encode_png(grays) == refs
    rgb = R.content("smooth", 37, 53, 3)
    assert c.encode_png(rgb[None]) == [R.png_file(37, 53, 3, R.encode_stream(rgb))]
    assert c.encode_png(np.zeros((0, 8, 8, 3), np.uint8)) == []
    with pytest.raises(ValueError, match="uint8"):
        c.encode_png(np.zeros((1, 8, 8, 3), np.float32))
    # Cropper.encode_png with a face that overflows: the host's file for it, device files for the others
    real = pngenc.encode_png
    try:
        pngenc.encode_png = lambda px, capacity=None: real(px, capacity=fits_one)
        assert c.encode_png(grays) == [host[0], refs[1], host[2]]
    finally:
        pngenc.encode_png = real
    for file, g in zip(files, grays):
        assert np.array_equal(_decode(file), g)


def test_two_runs_give_identical_bytes(device, batches):
    for shape in ((37, 53, 3), (96, 80, 1)):
        _, imgs, want = batches[shape]
        capacity = max(len(s) for s in want)
        a = _encode(device, imgs, capacity, "cabi")
        b = _encode(device, imgs, capacity, "cabi")
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])


def test_refusals_carry_a_message(device):
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import pngenc
    from face_crop_plus_amd import torch_ops as T
    pixels = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=device)
    out = torch.full((1, 64), 7, dtype=torch.uint8, device=device)
    lengths = torch.full((1,), -5, dtype=torch.int32, device=device)
    lib = N.lib()
    need = lib.fcp_png_workspace_bytes(1, 8, 8, 3)
    work = torch.empty((need,), dtype=torch.uint8, device=device)

    def call(f=1, h=8, w=8, c=3, cap=64, wsb=need, ws=work, px=pixels):
        return lib.fcp_png_encode_u8(N.ptr(px), f, h, w, c, N.ptr(out), 64, cap, N.ptr(lengths), N.ptr(ws), wsb, N.stream_ptr())
    for kw, word in ((dict(h=0), b"bad sizes"), (dict(f=-1), b"bad sizes"), (dict(c=2), b"channels"), (dict(cap=65), b"capacity"),
                     (dict(cap=-1), b"capacity"), (dict(wsb=need - 1), b"workspace"), (dict(w=8193), b"8192"),
                     (dict(h=1760, w=1760), b"9227464"), (dict(px=None), b"null")):
        assert call(**kw) < 0, kw
        assert word in lib.fcp_last_error(), (kw, lib.fcp_last_error())
    assert lib.fcp_png_encode_u8(N.ptr(pixels), 1, 8, 8, 3, N.ptr(out), 64, 64, N.ptr(lengths), N.ptr(work, 4), need,
                                 N.stream_ptr()) < 0
    assert b"aligned" in lib.fcp_last_error()
    freq = torch.zeros((1, 286), dtype=torch.int32, device=device)
    code_lengths = torch.full((1, 286), 9, dtype=torch.uint8, device=device)
    assert lib.fcp_png_huffman_lengths(N.ptr(freq), -1, N.ptr(code_lengths), None, N.stream_ptr()) < 0
    assert b"rows" in lib.fcp_last_error()
    assert lib.fcp_png_huffman_lengths(None, 1, N.ptr(code_lengths), None, N.stream_ptr()) < 0
    assert b"null" in lib.fcp_last_error()
    assert lib.fcp_png_huffman_lengths(N.ptr(freq, 2), 1, N.ptr(code_lengths), None, N.stream_ptr()) < 0
    assert b"aligned" in lib.fcp_last_error()
    torch.cuda.synchronize()
    assert (out.cpu() == 7).all() and lengths.cpu().tolist() == [-5] and (code_lengths.cpu() == 9).all()   # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    want = R.encode_stream(np.zeros((8, 8, 3), np.uint8))
    assert lengths.cpu().tolist() == [len(want)] and out.cpu().numpy()[0, :len(want)].tobytes() == want
    ops = T.load()
    with pytest.raises(RuntimeError, match="capacity"):
        ops.png_encode(pixels, torch.zeros((2, 64), dtype=torch.uint8, device=device))
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.png_encode(pixels, torch.zeros((1, 128), dtype=torch.uint8, device=device)[:, ::2])
    with pytest.raises(RuntimeError, match="9227464"):
        ops.png_encode(torch.zeros((1, 1760, 1760, 3), dtype=torch.uint8, device=device), out)
    with pytest.raises(RuntimeError):
        ops.png_encode(pixels.float(), out)
    with pytest.raises(RuntimeError, match="286"):
        ops.png_huffman_lengths(torch.zeros((1, 256), dtype=torch.int32, device=device), False)
    empty = pngenc.encode_streams(torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=device),
                                  torch.zeros((0, 16), dtype=torch.uint8, device=device))
    assert tuple(empty.shape) == (0,)
    # a face the kernels refuse goes to the host, whole
    assert not pngenc.supported(8200, 4, 1)
    tall = torch.zeros((1, 8200, 4), dtype=torch.uint8, device=device)
    assert pngenc.encode_png(tall) == [pngenc._host_png(np.zeros((8200, 4), np.uint8))]


# ---- end to end: process_dir, device against host
def _noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


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
    d = tmp_path_factory.mktemp("png_in")
    rng = np.random.default_rng(31)
    imgs = {"a.png": R.smooth(240, 320), "b.jpg": R.smooth(300, 260)[:, ::-1].copy(), "c.png": _noise(rng, 200, 220)}
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


def _same_pixels(dev, host):
    assert sorted(host) and sorted(dev) == sorted(host)
    for n in host:
        a, b = _decode(dev[n]), _decode(host[n])
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), n


@pytest.mark.parametrize("extra", [dict(), dict(crop_source="original")], ids=["plain", "original"])
def test_process_dir_png_device_decodes_like_host(device, photos, tmp_path, monkeypatch, extra):
    """Every target is a PNG: the same names and pixels, the streams of the definition.  With crop_source="original" the
    crops are made on the device and stay there: the host run reads them back, the device run does not (with the
    default crop_source and a landmark table, ``Cropper.crop_align`` hands the crops over as numpy arrays either way)."""
    readbacks = []
    real = torch.Tensor.cpu

    def spy(self, *a, **k):
        if self.dtype == torch.uint8 and self.dim() == 4 and tuple(self.shape[1:]) == (80, 96, 3):
            readbacks.append(tuple(self.shape))
        return real(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", spy)
    host = _run(photos, tmp_path / "host", output_format="png", png_encoder="host", **extra)
    on_host, readbacks[:] = list(readbacks), []
    dev = _run(photos, tmp_path / "dev", output_format="png", png_encoder="device", **extra)
    monkeypatch.undo()
    print(extra, "crop read-backs: host", on_host, "device", readbacks)
    if extra:
        assert on_host and readbacks == []
    assert sorted(host) == ["a.png", "b.png", "c.png"]
    _same_pixels(dev, host)
    for n in dev:
        assert dev[n] != host[n] and dev[n][:8] == b"\x89PNG\r\n\x1a\n", n
        px = _decode(host[n])
        assert px.shape == (80, 96, 3)                                         # output_size is (width, height)
        assert dev[n] == R.png_file(80, 96, 3, R.encode_stream(px)), n         # the definition, to the byte
    print({n: (len(dev[n]), len(host[n])) for n in sorted(dev)})
    assert len(dev["a.png"]) < len(host["a.png"]) and len(dev["b.png"]) < len(host["b.png"])


def test_process_dir_strategy_all_with_mask_groups(device, photos, tmp_path):
    kw = dict(output_format="png", strategy="all", mask_groups={"all": list(range(19)), "low": list(range(10))},
              attr_groups=None, weights={"bisenet": "generated"})
    host = _run(photos, tmp_path / "host", png_encoder="host", **kw)
    dev = _run(photos, tmp_path / "dev", png_encoder="device", **kw)
    assert any(os.sep + "all_mask" + os.sep in os.sep + n for n in host) and any(n.endswith("a_1.png") for n in host)
    _same_pixels(dev, host)
    masks = [n for n in dev if "_mask" + os.sep in n]
    assert masks and all(_decode(dev[n]).ndim == 2 for n in masks)


@pytest.mark.parametrize("encoder", ["host", "device"])
def test_process_dir_source_extensions_keep_the_jpeg(device, photos, tmp_path, encoder):
    """No output_format: b.jpg stays a JPEG, byte for byte the host's through either JPEG encoder; the PNG targets match in
    pixels."""
    host = _run(photos, tmp_path / "host", encoder="host", png_encoder="host")
    dev = _run(photos, tmp_path / "dev", encoder=encoder, png_encoder="device")
    assert sorted(host) == ["a.png", "b.jpg", "c.png"]
    assert dev["b.jpg"] == host["b.jpg"]
    _same_pixels({n: v for n, v in dev.items() if n.endswith(".png")}, {n: v for n, v in host.items() if n.endswith(".png")})
    assert dev["a.png"] != host["a.png"]
