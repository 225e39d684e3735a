"""Cropper(background="transparent") / Cropper(decontaminate=...) on the GPU: fcp_feather_alpha_u8 against
tests/matte_ref.py, fcp_cutout_u8 against tests/cutout_ref.py in both modes, the PNG kernels at four channels against
tests/png_ref.py, Cropper.matte against the references chained, and process_dir end to end.  Every comparison is byte
for byte: equality everywhere, no tolerance.

Every test fails without the feature: the entry points, the ops and the keywords do not exist there."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(os.path.dirname(__file__), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("cutout_ref")
P = _load("png_ref")
RF = _load("matte_refine_ref")
S = _load("subject_ref")
MR = R.MR
FILL = (0, 177, 64)
GUARD = 64
_TAPS = {}


def _taps(sigma):
    from face_crop_plus_amd import matte as M
    if sigma not in _TAPS:
        _TAPS[sigma] = None if sigma is None else M.blur_taps(sigma)
    return _TAPS[sigma]


def _decode(file):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(file)))


def _boundary(enabled):
    """Context: the torch-op boundary (True) or ctypes (False)."""
    from face_crop_plus_amd import torch_ops as T

    class Ctx:
        def __enter__(self):
            self.old, T.ENABLED = T.ENABLED, enabled

        def __exit__(self, *exc):
            T.ENABLED = self.old
    return Ctx()


@pytest.fixture(scope="module")
def inputs():
    """(h, w) -> (crops (3,h,w,3), {alpha kind: plane (3,h,w)}), made once, read-only."""
    out = {}
    for h, w in R.SHAPES:
        rng = np.random.default_rng(1000 * h + w)
        crops = MR.random_crops(rng, 3, h, w)
        planes = {kind: R.alpha_of(kind, rng, 3, h, w) for kind in R.ALPHAS}
        crops.setflags(write=False)
        for p in planes.values():
            p.setflags(write=False)
        out[(h, w)] = (crops, planes)
    return out


# ---- fcp_feather_alpha_u8
@pytest.mark.parametrize("shape", R.SHAPES + [(33, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_feather_alpha_equals_matte_ref(device, shape):
    """(33, 130): more than one 64 x 32 tile both ways, neither a multiple."""
    from face_crop_plus_amd import matte as M
    h, w = shape
    rng = np.random.default_rng(7 * h + w)
    for labels, bits in ((R.disc_labels(3, h, w), 1 << 1), (MR.random_labels(rng, 3, h, w), MR.DEFAULT_BITS)):
        ld = torch.from_numpy(labels).to(device)
        for feather in MR.FEATHERS:
            want = R.feathered(labels, bits, feather)
            for f in (1, 3):
                got = {}
                for enabled in (True, False):
                    with _boundary(enabled):
                        got[enabled] = M.feather_alpha(ld[:f].contiguous(), bits, feather)
                assert got[True].dtype == torch.uint8 and tuple(got[True].shape) == (f, h, w)
                assert torch.equal(got[True], got[False])
                assert np.array_equal(got[True].cpu().numpy(), want[:f]), (shape, feather, f)
                # it is the alpha the matte kernel composites through
                _, alpha = M.matte(torch.zeros((f, h, w, 3), dtype=torch.uint8, device=device), ld[:f].contiguous(), bits, feather,
                                   FILL, with_alpha=True)
                assert torch.equal(alpha, got[True])


# ---- fcp_cutout_u8
@pytest.mark.parametrize("sigma", [None, 0.5, 4, 16], ids=lambda s: f"sigma{s}")
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cutout_equals_the_reference(device, inputs, shape, sigma):
    """Both modes, F in {1, 3}, every alpha kind; the disc planes come from fcp_feather_alpha_u8 on the device.  Fill mode
    without an estimate is refused: that composite is fcp_matte_alpha_u8."""
    from face_crop_plus_amd import matte as M
    h, w = shape
    crops, planes = inputs[shape]
    taps = _taps(sigma)
    cd = torch.from_numpy(crops.copy()).to(device)
    labels = torch.from_numpy(R.disc_labels(3, h, w)).to(device)
    for kind in R.ALPHAS:
        plane = planes[kind]
        if kind.startswith("disc"):
            ad = M.feather_alpha(labels, 1 << 1, int(kind[4:]))
            assert np.array_equal(ad.cpu().numpy(), plane), kind
        else:
            ad = torch.from_numpy(plane.copy()).to(device)
        fg = R.foreground(crops, plane, taps)                        # once for both modes
        want = {R.RGBA: R.rgba(crops, plane, taps, fg)}
        if taps is not None:
            want[R.FILL] = R.fill(crops, plane, taps, FILL, fg)
        for f in (1, 3):
            for mode, expect in want.items():
                got = M.cutout(cd[:f].contiguous(), ad[:f].contiguous(), None if mode == R.RGBA else FILL, taps)
                assert got.dtype == torch.uint8 and tuple(got.shape) == (f, h, w, 4 if mode == R.RGBA else 3)
                got = got.cpu().numpy()
                bad = int((got != expect[:f]).sum())
                assert bad == 0, ((shape, sigma, kind, f, mode), bad, np.argwhere(got != expect[:f])[:4].tolist())
    if taps is None:
        with pytest.raises(RuntimeError, match="fcp_matte_alpha_u8"):
            M.cutout(cd, ad, FILL, None)


def test_boundaries_agree_and_guard_bytes_stay(device, inputs):
    """ctypes against the ops; the C entry between guard bytes, on crops and alpha that start at odd bytes."""
    import ctypes
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import matte as M
    shape = (37, 53)
    h, w = shape
    crops, planes = inputs[shape]
    plane = planes["mixed0"]
    cd, ad = torch.from_numpy(crops.copy()).to(device), torch.from_numpy(plane.copy()).to(device)
    for fill in (None, FILL):
        for sigma in ((None, 4) if fill is None else (4,)):
            res = {}
            for enabled in (True, False):
                with _boundary(enabled):
                    res[enabled] = M.cutout(cd, ad, fill, _taps(sigma))
            assert torch.equal(res[True], res[False]), (fill, sigma)
    lib = N.lib()
    taps = _taps(4)
    t16 = (ctypes.c_uint16 * len(taps))(*taps)
    need = lib.fcp_cutout_workspace_bytes(3, h, w)
    assert need == 32 * 3 * h * w
    work = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device=device)
    # inputs at an odd byte: a copy of each one byte into a larger buffer
    cbuf = torch.zeros((crops.size + 8,), dtype=torch.uint8, device=device)
    abuf = torch.zeros((plane.size + 8,), dtype=torch.uint8, device=device)
    cbuf[1:1 + crops.size] = cd.flatten()
    abuf[3:3 + plane.size] = ad.flatten()
    cases = [(R.RGBA, len(taps) - 1, 0, R.rgba(crops, plane, taps)), (R.FILL, len(taps) - 1, 1, R.fill(crops, plane, taps, FILL)),
             (R.RGBA, 0, 0, R.rgba(crops, plane, None))]
    for mode, radius, off, expect in cases:
        n = expect.size
        buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device)
        rc = lib.fcp_cutout_u8(N.ptr(cbuf, 1), N.ptr(abuf, 3), 3, h, w, mode, *FILL, t16, radius, N.ptr(buf, GUARD + off),
                               N.ptr(work), need, N.stream_ptr())
        assert rc == 0, lib.fcp_last_error()
        host = buf.cpu().numpy()
        assert np.array_equal(host[GUARD + off:GUARD + off + n].reshape(expect.shape), expect), (mode, radius)
        assert (host[:GUARD + off] == 0xA5).all() and (host[GUARD + off + n:] == 0xA5).all(), (mode, radius, "guard bytes")
    assert (work[need:].cpu() == 0x5A).all()


def test_refusals_carry_their_messages(device):
    import ctypes
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import matte as M
    from face_crop_plus_amd import torch_ops as T
    lib = N.lib()
    crops = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=device)
    alpha = torch.full((1, 8, 8), 128, dtype=torch.uint8, device=device)
    out = torch.full((1, 8, 8, 4), 7, dtype=torch.uint8, device=device)
    taps = _taps(4)
    t16 = (ctypes.c_uint16 * len(taps))(*taps)
    need = lib.fcp_cutout_workspace_bytes(1, 8, 8)
    work = torch.empty((need + 16,), dtype=torch.uint8, device=device)

    def call(mode=0, radius=len(taps) - 1, o=N.ptr(out), ws=N.ptr(work), wsb=need, a=N.ptr(alpha), f=1, t=t16):
        return lib.fcp_cutout_u8(N.ptr(crops), a, f, 8, 8, mode, 1, 2, 3, t, radius, o, ws, wsb, N.stream_ptr())
    zero_tap, short_sum = (ctypes.c_uint16 * 4)(4090, 2, 0, 1), (ctypes.c_uint16 * 4)(4089, 1, 1, 1)   # sums 4096 and 4095
    for kw, word in ((dict(mode=3), b"mode"), (dict(radius=2), b"radius"), (dict(radius=49), b"radius"),
                     (dict(mode=1, radius=0), b"fcp_matte_alpha_u8"), (dict(radius=11), b"sum to 4096"),
                     (dict(wsb=need - 1), b"workspace"), (dict(ws=None), b"workspace"), (dict(ws=N.ptr(work, 4)), b"16-byte aligned"),
                     (dict(o=N.ptr(out, 1)), b"4-byte aligned"), (dict(a=None), b"null pointer"), (dict(o=None), b"null pointer"),
                     (dict(f=65536), b"65535"), (dict(radius=3, t=zero_tap), b"tap 2 is 0"),
                     (dict(radius=3, t=short_sum), b"sum to 4096")):
        assert call(**kw) < 0, kw
        assert word in lib.fcp_last_error() and b"cutout" in lib.fcp_last_error(), (kw, lib.fcp_last_error())
        assert lib.fcp_last_error().startswith(b"cutout:"), lib.fcp_last_error()
    torch.cuda.synchronize()
    assert (out.cpu() == 7).all()                                    # nothing was launched
    assert call() == 0 and call(radius=0, ws=None, wsb=0) == 0       # radius 0 reads no workspace
    ops = T.load()
    with pytest.raises(RuntimeError, match="radius 3..48"):
        ops.cutout(crops, alpha, 0, 0, 0, 0, [4096, 0])
    with pytest.raises(RuntimeError, match="16 bits"):
        ops.cutout(crops, alpha, 0, 0, 0, 0, [70000, 1, 1, 1])
    with pytest.raises(RuntimeError, match="sum to 4096"):
        ops.cutout(crops, alpha, 0, 0, 0, 0, [4000, 1, 1, 1])
    with pytest.raises(RuntimeError, match="mode"):
        ops.cutout(crops, alpha, 2, 0, 0, 0, taps)
    with pytest.raises(RuntimeError, match="fill"):
        ops.cutout(crops, alpha, 1, 0, 300, 0, taps)
    with pytest.raises(RuntimeError, match="alpha"):
        ops.cutout(crops, alpha[:, :4], 0, 0, 0, 0, taps)
    with pytest.raises(RuntimeError, match="feather"):
        ops.feather_alpha(alpha, 2, 4)
    with pytest.raises(RuntimeError, match="class_bits"):
        ops.feather_alpha(alpha, 1 << 19, 5)
    with pytest.raises(RuntimeError):
        ops.feather_alpha(alpha.float(), 2, 5)
    for enabled in (True, False):
        with _boundary(enabled):
            assert tuple(M.cutout(crops[:0], alpha[:0], None, taps).shape) == (0, 8, 8, 4)
            assert tuple(M.cutout(crops[:0], alpha[:0], FILL, taps).shape) == (0, 8, 8, 3)
            assert tuple(M.feather_alpha(alpha[:0], 2, 5).shape) == (0, 8, 8)
            with pytest.raises(RuntimeError, match="radius"):
                M.cutout(crops, alpha, None, [4094, 1])


# ---- PNG at four channels
def _rgba_images():
    rng = np.random.default_rng(77)
    a = rng.integers(0, 256, (17, 9, 4), dtype=np.uint8)
    b = np.concatenate([P.smooth(37, 53), rng.integers(0, 256, (37, 53, 1), dtype=np.uint8)], -1)
    c = np.concatenate([P.smooth(96, 80), P.disc(96, 80)[..., None]], -1)
    c[c[..., 3] == 0] = 0                                            # a cut-out: zeros outside the disc
    return [a, b, c]


@pytest.mark.parametrize("boundary", ["op", "cabi"])
def test_png_streams_at_four_channels_equal_the_definition(device, boundary):
    from face_crop_plus_amd import pngenc
    for img in _rgba_images():
        h, w, _ = img.shape
        want = P.encode_stream(img)
        capacity = len(want) + 5
        buf = torch.full((1, capacity + 2 * GUARD), 0xA5, dtype=torch.uint8, device=device)
        with _boundary(boundary == "op"):
            lengths = pngenc.encode_streams(torch.from_numpy(img[None].copy()).to(device), buf[:, GUARD:GUARD + capacity])
        host = buf.cpu().numpy()[0]
        assert lengths.cpu().tolist() == [len(want)], (img.shape, boundary)
        assert host[GUARD:GUARD + len(want)].tobytes() == want, (img.shape, boundary)
        assert (host[:GUARD] == 0xA5).all() and (host[GUARD + len(want):] == 0xA5).all()
        file = pngenc.png_file_rgba(h, w, want)
        assert pngenc.encode_png(torch.from_numpy(img[None].copy()).to(device)) == [file]
        got = _decode(file)
        assert got.shape == img.shape and np.array_equal(got, img)


def test_png_slot_overflow_falls_back_to_the_host_rgba_file(device):
    from face_crop_plus_amd import Cropper, pngenc
    imgs = _rgba_images()
    noise = np.random.default_rng(3).integers(0, 256, (96, 80, 4), dtype=np.uint8)
    cut = imgs[2]
    batch = np.stack([noise, cut])
    dev = torch.from_numpy(batch).to(device)
    refs = [pngenc.png_file_rgba(96, 80, P.encode_stream(b)) for b in batch]
    host = [pngenc._host_png(b) for b in batch]
    fits_one = len(P.encode_stream(cut)) + 7
    assert len(P.encode_stream(noise)) > fits_one
    files = pngenc.encode_png(dev, capacity=fits_one)
    assert files == [host[0], refs[1]]
    for file, b in zip(files, batch):
        got = _decode(file)
        assert got.shape == (96, 80, 4) and np.array_equal(got, b)
    assert pngenc.encode_png(dev) == refs
    c = Cropper(output_size=48, det_threshold=None, device="cuda:0")
    assert c.encode_png(batch) == refs
    # a size the kernels refuse at four channels goes to the host, whole
    assert pngenc.supported(1, 8192, 1) and not pngenc.supported_rgba(8192, 282)
    tall = torch.zeros((1, 8192, 282, 4), dtype=torch.uint8, device=device)
    assert pngenc.encode_png(tall) == [pngenc._host_png(np.zeros((8192, 282, 4), np.uint8))]


# ---- Cropper.matte
def test_cropper_matte_transparent_equals_the_references_chained(device):
    from face_crop_plus_amd import Cropper
    shape = (96, 80)
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    labels = S.labels_of(S.GROUPS[0], rng, *shape).copy()
    crops = MR.random_crops(np.random.default_rng(12), 3, *shape)
    lm = (np.zeros((1, 5, 2), np.float32), np.array(["a"]))
    kw = dict(output_size=48, landmarks=lm, det_threshold=None, device="cuda:0", weights={"bisenet": "generated"})
    c = Cropper(background="transparent", output_format="png", refine=4, subject="largest", decontaminate=4, **kw)
    assert c.par_model is not None and c.feather == 0
    clean = S.subject_mask(labels, S.DEFAULT_BITS, True, 0)
    want_a = RF.alpha_of(crops, clean, S.SUBJECT_BITS, 4, 64)
    assert ((want_a > 0) & (want_a < 255)).any()
    out, alpha = c.matte(crops, labels)
    assert out.shape == (3, 96, 80, 4) and np.array_equal(alpha, want_a)
    assert np.array_equal(out, R.rgba(crops, want_a, _taps(4)))
    # without the estimate: the crop's colours under the same alpha
    c = Cropper(background="transparent", output_format="png", refine=4, subject="largest", **kw)
    out, alpha = c.matte(crops, labels)
    assert np.array_equal(alpha, want_a) and np.array_equal(out, R.rgba(crops, want_a, None))
    # the feathered mask as the alpha, and the decontaminated composite over a fill
    feathered = R.feathered(labels, S.DEFAULT_BITS, 7)
    c = Cropper(background="transparent", output_format="PNG", feather=7, decontaminate=2, **kw)
    out, alpha = c.matte(crops, labels)
    assert np.array_equal(alpha, feathered) and np.array_equal(out, R.rgba(crops, feathered, _taps(2)))
    c = Cropper(background=FILL, feather=7, decontaminate=2, **kw)
    out, alpha = c.matte(crops, labels)
    assert out.shape == (3, 96, 80, 3) and np.array_equal(alpha, feathered)
    assert np.array_equal(out, R.fill(crops, feathered, _taps(2), FILL))
    # decontaminate off: the composite of the crop's own colours, as before
    out, alpha = Cropper(background=FILL, feather=7, **kw).matte(crops, labels)
    assert np.array_equal(out, MR.matte(crops, labels, S.DEFAULT_BITS, 7, FILL)[0])


# ---- end to end: process_dir
def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for n in files:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def photos(tmp_path_factory):
    """Three generated files (one of them a JPEG) and a landmark table for them."""
    from PIL import Image
    d = tmp_path_factory.mktemp("cutout_in")
    rng = np.random.default_rng(31)
    imgs = {"a.png": P.smooth(240, 320), "b.jpg": P.smooth(300, 260)[:, ::-1].copy(),
            "c.png": rng.integers(0, 256, (200, 220, 3), dtype=np.uint8)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name)
    size = (96, 80)
    tgt = A.landmarks_target(size, 0.65)
    rows, names = [], []
    for name, scale, shift in (("a.png", 1.3, (100.0, 60.0)), ("b.jpg", 1.6, (40.0, 90.0)), ("c.png", 1.1, (50.0, 40.0))):
        rows.append(tgt * scale + np.array(shift, np.float32))
        names.append(name)
    return d, (np.stack(rows).astype(np.float32), np.array(names)), size


def _cropper(photos, **kw):
    from face_crop_plus_amd import Cropper
    d, landmarks, size = photos
    return Cropper(output_size=size, landmarks=landmarks, device="cuda:0", padding="reflect_101", batch_size=2,
                   weights={"bisenet": "generated"}, **kw)


def test_process_dir_writes_rgba_cutouts_through_both_encoders(device, photos, tmp_path):
    from PIL import Image
    from face_crop_plus_amd import cropper as CR
    from face_crop_plus_amd import pngenc
    trees, seen = {}, []
    real = CR.Cropper._matte_device

    def spy(self, crops_dev, labels_dev, with_alpha=False):
        out, alpha = real(self, crops_dev, labels_dev, with_alpha=True)
        seen.append((crops_dev.cpu().numpy(), alpha.cpu().numpy(), out.cpu().numpy()))
        return out, (alpha if with_alpha else None)
    CR.Cropper._matte_device = spy
    try:
        for enc in ("host", "device"):
            c = _cropper(photos, background="transparent", output_format="png", decontaminate=4, png_encoder=enc)
            c.process_dir(str(photos[0]), str(tmp_path / enc), desc=None)
            trees[enc] = _tree(tmp_path / enc)
    finally:
        CR.Cropper._matte_device = real
    assert sorted(trees["host"]) == sorted(trees["device"]) == ["a.png", "b.png", "c.png"]
    for n in trees["host"]:
        imgs = {enc: Image.open(io.BytesIO(trees[enc][n])) for enc in trees}
        for enc, im in imgs.items():
            assert im.mode == "RGBA" and im.size == photos[2], (n, enc)           # output_size is (width, height)
        a, b = np.asarray(imgs["host"]), np.asarray(imgs["device"])
        assert a.shape == (80, 96, 4) and np.array_equal(a, b), n
        assert trees["device"][n] != trees["host"][n]
        assert trees["device"][n] == pngenc.png_file_rgba(80, 96, P.encode_stream(a)), n
    # what was written is the reference's cut-out of what the matte step saw
    assert seen
    written = {np.asarray(Image.open(io.BytesIO(v))).tobytes() for v in trees["host"].values()}
    for crops, alpha, out in seen:
        assert out.shape[1:] == (80, 96, 4) and np.array_equal(out, R.rgba(crops, alpha, _taps(4)))
    assert written == {o.tobytes() for _, _, out in seen[:len(seen) // 2] for o in out}


def test_process_dir_fill_without_decontaminate_is_unchanged(device, photos, tmp_path, monkeypatch):
    """background=(R,G,B) alone: nothing new is launched, and the files are byte for byte those of the matte step as it
    was before this feature (``matte.matte`` on the crops and the parser's labels)."""
    from face_crop_plus_amd import cropper as CR
    from face_crop_plus_amd import matte as M
    calls = []
    for name in ("cutout", "feather_alpha"):
        monkeypatch.setattr(M, name, lambda *a, _n=name, **k: calls.append(_n) or (_ for _ in ()).throw(AssertionError(_n)))
    c = _cropper(photos, background=FILL, output_format="png")
    assert c.decontaminate is None and c.decontaminate_taps is None
    c.process_dir(str(photos[0]), str(tmp_path / "now"), desc=None)
    assert calls == []

    def before(self, crops_dev, labels_dev, with_alpha=False):
        return M.matte(crops_dev, labels_dev, self.foreground_bits, self.feather, self.background, with_alpha=with_alpha)
    monkeypatch.setattr(CR.Cropper, "_matte_device", before)
    c = _cropper(photos, background=FILL, output_format="png")
    c.process_dir(str(photos[0]), str(tmp_path / "before"), desc=None)
    now, was = _tree(tmp_path / "now"), _tree(tmp_path / "before")
    assert sorted(now) == ["a.png", "b.png", "c.png"] and now == was
    assert all(_decode(v).shape == (80, 96, 3) for v in now.values())
