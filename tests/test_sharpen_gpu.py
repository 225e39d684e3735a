"""Cropper(sharpen=A) on the GPU: the unsharp-mask kernel against tests/sharpen_ref.py byte for byte (no tolerance
anywhere), through ctypes and through the torch op: crops smaller than one tile and smaller than the halo, sizes that are
no multiple of a tile, several tiles in both directions, both tile shapes and the radii on either side of the radius at
which the host changes between them, contents that reach both clamps of the output, any taps, the crops of a batch one by
one, F = 0, Cropper.unsharp, and process_dir end to end."""
import ctypes
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu


def _load():
    spec = importlib.util.spec_from_file_location("_sharpen_ref", os.path.join(os.path.dirname(__file__), "sharpen_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
SHAPES = [(1, 1), (1, 7), (5, 3), (33, 47), (64, 64), (70, 130)]
# sigma -> (radius, amount, threshold): r = 3 and 5 run the 32 x 64 tiles, r = 48 the 48 x 64 tiles
SETTINGS = {0.5: (3, 4, 0), 1.5: (5, 1.0, 2), 16: (48, 0.6, 0)}
_CROPS, _WANT = {}, {}


def _crops(shape):
    """(uniform noise, gradient plus noise, 0/255 checkerboard of period 1, constant 255) of one shape, (4,h,w,3) uint8."""
    if shape not in _CROPS:
        h, w = shape
        rng = np.random.default_rng(1000 * h + w)
        y, x = np.mgrid[0:h, 0:w]
        ramp = np.stack([30 + 180 * x / max(w - 1, 1), 200 - 150 * y / max(h - 1, 1), 60 + 60 * (x + y) / max(h + w - 2, 1)], -1)
        gradient = np.clip(np.rint(ramp + rng.normal(0, 6, (h, w, 3))), 0, 255).astype(np.uint8)
        checker = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
        _CROPS[shape] = np.stack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), gradient, checker, np.full((h, w, 3), 255, np.uint8)])
    return _CROPS[shape]


def _want(shape, sigma):
    """The reference for the four crops of a shape, computed once."""
    if (shape, sigma) not in _WANT:
        _, amount, threshold = SETTINGS[sigma]
        _WANT[shape, sigma] = R.sharpen(_crops(shape), amount, sigma, threshold)
    return _WANT[shape, sigma]


def _run(crops, taps, amount_q, threshold, device):
    from face_crop_plus_amd import sharpen as S
    return S.unsharp(torch.from_numpy(np.ascontiguousarray(crops)).to(device), taps, amount_q, threshold).cpu().numpy()


@pytest.mark.parametrize("sigma", list(SETTINGS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_reference(device, shape, sigma):
    from face_crop_plus_amd import matte as M
    from face_crop_plus_amd import sharpen as S
    crops, want = _crops(shape), _want(shape, sigma)
    radius, amount, threshold = SETTINGS[sigma]
    assert len(M.blur_taps(sigma)) - 1 == radius and M.blur_taps(sigma) == R.blur_taps(sigma)
    src = torch.from_numpy(crops).to(device)
    three = S.sharpen(src[:3].contiguous(), amount, sigma, threshold)               # F = 3
    assert three.dtype == torch.uint8 and tuple(three.shape) == (3, *shape, 3)
    assert np.array_equal(three.cpu().numpy(), want[:3])
    one = S.sharpen(src[3:].contiguous(), amount, sigma, threshold)                 # F = 1: constant 255 stays
    assert np.array_equal(one.cpu().numpy(), want[3:]) and (one == 255).all()
    assert np.array_equal(src.cpu().numpy(), crops)                                 # the input is untouched
    assert torch.equal(S.sharpen(src[:3].contiguous(), amount, sigma, threshold), three)     # the same bytes from run to run
    # crops 0 and 2 of the batch equal the same crops run alone
    assert torch.equal(S.sharpen(src[0:1].contiguous(), amount, sigma, threshold)[0], three[0])
    assert torch.equal(S.sharpen(src[2:3].contiguous(), amount, sigma, threshold)[0], three[2])
    if min(shape) > 1:
        assert not np.array_equal(want[0], crops[0])                                # the filter does something
    empty = S.sharpen(src[:0], amount, sigma, threshold)                            # F = 0
    assert tuple(empty.shape) == (0, *shape, 3) and empty.dtype == torch.uint8


def test_the_contents_reach_both_clamps():
    """What the contents are for, shown on the reference's own intermediates (no GPU needed, kept beside its users)."""
    parts = R.unsharp_parts(_crops((33, 47))[2], R.blur_taps(1.5), 1024, 0)
    assert parts["v"].min() < 0 and (parts["v"] >> 16).max() > 255                  # the checkerboard: both clamps
    parts = R.unsharp_parts(_crops((33, 47))[0], R.blur_taps(1.5), 256, 2)
    assert (parts["e"] == 0).any() and (parts["e"] > 0).any() and (parts["e"] < 0).any()     # noise: all three branches of the coring


TAPS = {"identity": [4096, 0, 0, 0],
        "r1": [2048, 1024],
        "r8": R.blur_taps(8 / 3),                              # the largest radius of the 32 x 64 tiles
        "r9": R.blur_taps(2.7),                                # the smallest of the 48 x 64 tiles
        "box31": [4096 - 2 * 64 * 31] + [64] * 31,
        "ends48": [2] + [0] * 47 + [2047]}                     # reads only the far ends of the halo


@pytest.mark.parametrize("shape", [(5, 3), (33, 47), (70, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_any_taps(device, shape):
    assert len(TAPS["r8"]) == 9 and len(TAPS["r9"]) == 10 and len(TAPS["ends48"]) == 49
    crops = _crops(shape)
    assert np.array_equal(_run(crops, TAPS["identity"], 1024, 0, device), crops)    # identity taps copy the crop
    for name, taps in TAPS.items():
        for amount_q, threshold in ((1, 0), (1024, 0), (256, 3), (700, 255)):
            got = _run(crops, taps, amount_q, threshold, device)
            assert np.array_equal(got, R.unsharp(crops, taps, amount_q, threshold)), (name, amount_q, threshold)
            if threshold == 255:
                assert np.array_equal(got, crops)                                   # T = 255 copies the crop


def test_boundaries_give_identical_tensors_and_refuse_bad_inputs(device, monkeypatch):
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import sharpen as S
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    shape = (33, 47)
    src = torch.from_numpy(_crops(shape)).to(device)
    for sigma, (_, amount, threshold) in SETTINGS.items():
        res = {}
        for enabled in (True, False):
            monkeypatch.setattr(T, "ENABLED", enabled)
            res[enabled] = S.sharpen(src, amount, sigma, threshold)
        assert torch.equal(res[True], res[False])
        assert np.array_equal(res[True].cpu().numpy(), _want(shape, sigma))
    taps = R.blur_taps(1.5)
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        with pytest.raises(RuntimeError, match="must sum to 4096"):
            S.unsharp(src, taps[:-1], 256, 0)
        with pytest.raises(RuntimeError, match="amount_q8 must be 1..1024"):
            S.unsharp(src, taps, 1025, 0)
        with pytest.raises(RuntimeError, match="threshold must be 0..255"):
            S.unsharp(src, taps, 256, 256)
        with pytest.raises(RuntimeError, match="radius 1..48"):
            S.unsharp(src, [4096], 256, 0)
        for bad in (src.float(), src[:, :, ::2], src[..., :2], src[0]):
            with pytest.raises(AssertionError):
                S.unsharp(bad, taps, 256, 0)
    ops = T.load()
    for bad in (src.float(), src[:, :, ::2], src[0]):                                   # the op itself refuses them too
        with pytest.raises(RuntimeError):
            ops.unsharp(bad, taps, 256, 0)
    with pytest.raises(RuntimeError):
        ops.unsharp(src.cpu(), taps, 256, 0)
    # in place and overlapping outputs, on real device memory: refused before any launch
    f, h, w, _ = src.shape
    nbytes = f * h * w * 3
    buf = torch.zeros(2 * nbytes, dtype=torch.uint8, device=device)
    buf[:nbytes] = src.reshape(-1)
    t16 = (ctypes.c_uint16 * len(taps))(*taps)
    base = buf.data_ptr()
    for offset in (0, 1, nbytes - 1, -1):
        rc = N.lib().fcp_unsharp_u8(ctypes.c_void_p(base + max(-offset, 0)), f, h, w, t16, len(taps) - 1, 256, 0,
                                    ctypes.c_void_p(base + max(offset, 0)), N.stream_ptr())
        assert rc == -1 and b"must not overlap" in N.lib().fcp_last_error(), offset
    torch.cuda.synchronize()
    assert np.array_equal(buf[:nbytes].cpu().numpy(), src.reshape(-1).cpu().numpy()) and int(buf[nbytes:].max()) == 0
    # the disjoint second half is accepted
    rc = N.lib().fcp_unsharp_u8(ctypes.c_void_p(base), f, h, w, t16, len(taps) - 1, 256, 2, ctypes.c_void_p(base + nbytes), N.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(buf[nbytes:].cpu().numpy().reshape(src.shape), _want(shape, 1.5))


def test_cropper_unsharp_equals_reference(device):
    from face_crop_plus_amd import Cropper
    given = dict(landmarks=(np.zeros((1, 5, 2), np.float32), np.array(["a"])), det_threshold=None, device="cuda:0")
    shape = (33, 47)
    cr = Cropper(output_size=48, sharpen=1.0, sharpen_threshold=2, **given)
    assert (cr.sharpen, cr.sharpen_sigma, cr.sharpen_threshold) == (1.0, 1.5, 2) and cr.par_model is None
    out = cr.unsharp(_crops(shape))
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8
    assert np.array_equal(out, _want(shape, 1.5))
    assert cr.unsharp(_crops(shape)[:0]).shape == (0, *shape, 3)
    cr = Cropper(output_size=48, sharpen=0.6, sharpen_sigma=16, **given)
    assert np.array_equal(cr.unsharp(_crops(shape)), _want(shape, 16))
    with pytest.raises(ValueError, match="sharpen"):
        Cropper(output_size=48, **given).unsharp(_crops(shape))


# ---- end to end: process_dir on given landmarks
SIZE = (64, 64)
AMOUNT, SIGMA, THRESHOLD = 1.5, 1.5, 1
OPTIONS = dict(sharpen=AMOUNT, sharpen_threshold=THRESHOLD)


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for n in files:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _cropper(landmarks, **kw):
    from face_crop_plus_amd import Cropper
    kw.setdefault("output_format", "png")
    return Cropper(output_size=SIZE, landmarks=landmarks, device="cuda:0", padding="reflect_101", batch_size=2,
                   weights={"bisenet": "generated"}, **kw)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """Three files with a landmark set each (the faces of the BiSeNet golden fixture, the landmarks the target points, so
    that the generated parser splits every crop into subject and background), the crops a Cropper without ``sharpen``
    writes for them, the reference applied to those crops, the parser's labels and their most common class as the foreground."""
    from PIL import Image
    d = tmp_path_factory.mktemp("sharpen_in")
    faces = np.load(os.path.join(os.path.dirname(__file__), "golden", "bisenet.npz"))["faces"]
    assert faces.shape == (3, *SIZE, 3)
    imgs = {f"{n}.png": face for n, face in zip("abc", faces)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name, compress_level=1)
    tgt = A.landmarks_target(SIZE, 0.65)
    landmarks = (np.stack([tgt, tgt, tgt]).astype(np.float32), np.array(sorted(imgs)))
    out = tmp_path_factory.mktemp("sharpen_plain")
    _cropper(landmarks).process_dir(str(d), str(out), desc=None)
    plain = _tree(out)
    assert sorted(plain) == sorted(imgs)
    crops = np.stack([_pixels(plain[n]) for n in sorted(plain)])
    want = R.sharpen(crops, AMOUNT, SIGMA, THRESHOLD)
    assert all(not np.array_equal(a, b) for a, b in zip(want, crops))
    labels = _cropper(landmarks, background=0).par_model.parse(torch.from_numpy(crops).to("cuda:0"))[0].cpu().numpy()
    foreground = [int(np.bincount(labels.reshape(-1), minlength=19).argmax())]        # the most common class: some of each side
    assert all(m.any() and not m.all() for m in np.isin(labels, foreground)), "the generated parser does not split the crops"
    return {"dir": d, "landmarks": landmarks, "plain": plain, "crops": crops, "want": want, "labels": labels, "foreground": foreground}


def test_process_dir_writes_the_sharpened_crops(device, scene, tmp_path):
    c = _cropper(scene["landmarks"], **OPTIONS)
    assert (c.sharpen, c.sharpen_sigma, c.sharpen_threshold) == (AMOUNT, SIGMA, THRESHOLD) and c.par_model is None
    c.process_dir(str(scene["dir"]), str(tmp_path / "sh"), desc=None)
    got = _tree(tmp_path / "sh")
    assert sorted(got) == sorted(scene["plain"])
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), scene["want"][k]), n


def test_device_encoders_see_the_sharpened_crop(device, scene, tmp_path):
    c = _cropper(scene["landmarks"], png_encoder="device", **OPTIONS)
    c.process_dir(str(scene["dir"]), str(tmp_path / "png"), desc=None)
    got = _tree(tmp_path / "png")
    assert sorted(got) == sorted(scene["plain"])
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), scene["want"][k]), n
    c = _cropper(scene["landmarks"], encoder="device", output_format="jpg", **OPTIONS)
    c.process_dir(str(scene["dir"]), str(tmp_path / "jpg"), desc=None)
    got = _tree(tmp_path / "jpg")
    assert sorted(got) == ["a.jpg", "b.jpg", "c.jpg"]
    for data, ref in zip([got[n] for n in sorted(got)], c.encode_jpeg(scene["want"])):
        assert data == ref


def test_the_whole_chain_is_its_public_pieces(device, scene, tmp_path):
    """denoise, clahe, sharpen, matte: the files are matte(sharpen(clahe(denoise(crop)))) with the labels of the plain crop,
    and the fill is exact where the alpha is 0."""
    c = _cropper(scene["landmarks"], denoise=8, clahe=2.0, background=0, foreground=scene["foreground"], **OPTIONS)
    sharpened = c.unsharp(c.equalize(c.remove_noise(scene["crops"])))
    assert np.array_equal(sharpened, R.sharpen(c.equalize(c.remove_noise(scene["crops"])), AMOUNT, SIGMA, THRESHOLD))
    want, alpha = c.matte(sharpened, scene["labels"])
    assert (alpha == 0).any() and (alpha == 255).any()
    c.process_dir(str(scene["dir"]), str(tmp_path / "all"), desc=None)
    got = _tree(tmp_path / "all")
    assert sorted(got) == sorted(scene["plain"])
    unsharpened, _ = c.matte(c.equalize(c.remove_noise(scene["crops"])), scene["labels"])
    for k, n in enumerate(sorted(got)):
        px = _pixels(got[n])
        assert np.array_equal(px, want[k]), n
        assert (px[alpha[k] == 0] == 0).all()                                       # the fill is exact
        assert not np.array_equal(px, unsharpened[k])


def test_min_sharpness_scores_the_original_crop(device, scene, tmp_path):
    c = _cropper(scene["landmarks"])
    score = c.sharpness(scene["crops"])
    order = np.sort(score)
    assert order[0] < order[1]
    t = float(np.sqrt(max(order[0], 1e-9) * order[1])) if order[0] > 0 else float(order[1]) / 2
    kept = sorted(n for n, s in zip(sorted(scene["plain"]), score) if s >= t)
    assert 0 < len(kept) < 3
    assert not np.array_equal(c.sharpness(scene["want"]), score)                    # the sharpened crops score differently
    _cropper(scene["landmarks"], min_sharpness=t).process_dir(str(scene["dir"]), str(tmp_path / "plain"), desc=None)
    _cropper(scene["landmarks"], min_sharpness=t, **OPTIONS).process_dir(str(scene["dir"]), str(tmp_path / "sh"), desc=None)
    base, got = _tree(tmp_path / "plain"), _tree(tmp_path / "sh")
    assert sorted(got) == sorted(base) == kept                                      # the same set of files
    names = sorted(scene["plain"])
    for n in got:
        assert np.array_equal(_pixels(got[n]), scene["want"][names.index(n)]), n
