"""Cropper(denoise=H) on the GPU: the non-local-means kernel against tests/denoise_ref.py byte for byte (no tolerance
anywhere), through ctypes and through the torch op: the minimum size, sizes that are no multiple of the 32 x 64 tile,
several tiles in both directions, contents that reach both ends and the middle of the weight table, hostile tables, the
crops of a batch one by one, F = 0, Cropper.remove_noise, and process_dir end to end."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu


def _load():
    spec = importlib.util.spec_from_file_location("_denoise_ref", os.path.join(os.path.dirname(__file__), "denoise_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
SHAPES = [(14, 14), (14, 37), (33, 47), (64, 64), (70, 130)]
STRENGTHS = (1, 8, 32)
_CROPS, _WANT = {}, {}


def _crops(shape):
    """(uniform noise, gradient plus noise, 0/255 checkerboard of period 1, constant 255) of one shape, (4,h,w,3) uint8."""
    if shape not in _CROPS:
        h, w = shape
        rng = np.random.default_rng(1000 * h + w)
        y, x = np.mgrid[0:h, 0:w]
        ramp = np.stack([30 + 180 * x / (w - 1), 200 - 150 * y / (h - 1), 60 + 60 * (x + y) / (h + w - 2)], -1)
        gradient = np.clip(np.rint(ramp + rng.normal(0, 6, (h, w, 3))), 0, 255).astype(np.uint8)
        checker = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
        _CROPS[shape] = np.stack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), gradient, checker, np.full((h, w, 3), 255, np.uint8)])
    return _CROPS[shape]


def _want(shape, strength):
    """The reference for the four crops of a shape, computed once."""
    if (shape, strength) not in _WANT:
        _WANT[shape, strength] = R.denoise(_crops(shape), strength)
    return _WANT[shape, strength]


def _run(crops, lut, shift, device):
    from face_crop_plus_amd import denoise as D
    return D.nlm(torch.from_numpy(np.ascontiguousarray(crops)).to(device), torch.from_numpy(lut).to(device), shift).cpu().numpy()


@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_reference(device, shape, strength):
    from face_crop_plus_amd import denoise as D
    crops, want = _crops(shape), _want(shape, strength)
    lut, shift = D.weight_lut(strength)
    assert shift == R.TABLE[strength][1]
    src = torch.from_numpy(crops).to(device)
    three = D.denoise(src[:3].contiguous(), strength)                              # F = 3
    assert three.dtype == torch.uint8 and tuple(three.shape) == (3, *shape, 3)
    assert np.array_equal(three.cpu().numpy(), want[:3])
    one = D.denoise(src[3:].contiguous(), strength)                                # F = 1: constant 255, every weight 4096
    assert np.array_equal(one.cpu().numpy(), want[3:]) and (one == 255).all()
    assert np.array_equal(src.cpu().numpy(), crops)                                # the input is untouched
    assert torch.equal(D.denoise(src[:3].contiguous(), strength), three)           # the same bytes from run to run
    # crops 0 and 2 of the batch equal the same crops run alone
    assert torch.equal(D.denoise(src[0:1].contiguous(), strength)[0], three[0])
    assert torch.equal(D.denoise(src[2:3].contiguous(), strength)[0], three[2])
    if strength >= 8:
        assert not np.array_equal(want[1], crops[1])                               # the filter does something
    empty = D.denoise(src[:0], strength)                                           # F = 0
    assert tuple(empty.shape) == (0, *shape, 3) and empty.dtype == torch.uint8


def test_the_contents_reach_both_ends_of_the_table():
    """What the four contents are for, shown on the reference's own distances (no GPU needed, kept beside its users)."""
    crops = _crops((33, 47))
    g = np.pad(R.gray(crops[2]), 13, mode="reflect")
    d = int(((g[10:17, 10:17] - g[10:17, 11:18]) ** 2).sum())
    assert d == 49 * 255 ** 2                                                      # the checkerboard: maximal d
    lut, shift = R.weight_lut(1)
    noise = np.pad(R.gray(crops[0]), 13, mode="reflect")
    far = sum(int(((noise[20:27, 20:27] - noise[20 + oy:27 + oy, 20 + ox:27 + ox]) ** 2).sum()) >> shift >= len(lut)
              for oy in range(-10, 11) for ox in range(-10, 11))
    assert far >= 400                                                              # uniform noise at H = 1: most k >= n


@pytest.mark.parametrize("shape", [(14, 14), (33, 47), (70, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_any_table(device, shape):
    crops = _crops(shape)[:2]
    for lut, shift in ((np.full(4096, 65535, np.uint16), 10),        # every k < n: all weights clamp to ONE, sums at their maxima
                       (np.full(7, 65535, np.uint16), 3),            # the clamp and k >= n
                       (np.array([0, 0, 9, 70, 5000, 1, 0, 4096], np.uint16), 6),      # not monotone, zeros first: W == 0 happens
                       (np.full(1, 1, np.uint16), 0)):
        got = _run(crops, lut, shift, device)
        assert np.array_equal(got, R.nlm(crops, lut, shift)), (len(lut), shift)
    for n in (1, 100, 4096):
        assert np.array_equal(_run(crops, np.zeros(n, np.uint16), 0, device), crops)               # an all-zero table copies
    white = _crops(shape)[3:]
    assert (_run(white, np.full(4096, 65535, np.uint16), 0, device) == 255).all()                  # 441 * 4096 * 255 + W / 2 fits


def test_boundaries_give_identical_tensors_and_refuse_bad_inputs(device, monkeypatch):
    from face_crop_plus_amd import denoise as D
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    shape = (33, 47)
    src = torch.from_numpy(_crops(shape)).to(device)
    for strength in STRENGTHS:
        res = {}
        for enabled in (True, False):
            monkeypatch.setattr(T, "ENABLED", enabled)
            res[enabled] = D.denoise(src, strength)
        assert torch.equal(res[True], res[False])
        assert np.array_equal(res[True].cpu().numpy(), _want(shape, strength))
    lut = torch.from_numpy(D.weight_lut(8)[0]).to(device)
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        with pytest.raises(RuntimeError, match="at least 14 x 14"):
            D.nlm(src[:, :13].contiguous(), lut, 3)
        with pytest.raises(RuntimeError, match="shift must be 0..10"):
            D.nlm(src, lut, 11)
        with pytest.raises(RuntimeError, match="lut_len must be 1..4096"):
            D.nlm(src, lut[:0], 3)
        for bad in (src.float(), src[:, :, ::2], src[..., :2], src[0]):
            with pytest.raises(AssertionError):
                D.nlm(bad, lut, 3)
    ops = T.load()
    for bad in (src.float(), src[:, :, ::2], src[0]):                                   # the op itself refuses them too
        with pytest.raises(RuntimeError):
            ops.nlm_denoise(bad, lut, 3)
    with pytest.raises(RuntimeError):
        ops.nlm_denoise(src, lut.to(torch.int32), 3)
    with pytest.raises(RuntimeError):
        ops.nlm_denoise(src, lut.cpu(), 3)


def test_cropper_remove_noise_equals_reference(device):
    from face_crop_plus_amd import Cropper
    given = dict(landmarks=(np.zeros((1, 5, 2), np.float32), np.array(["a"])), det_threshold=None, device="cuda:0")
    shape = (33, 47)
    cr = Cropper(output_size=48, denoise=8, **given)
    assert cr.denoise == 8.0 and cr.par_model is None
    out = cr.remove_noise(_crops(shape))
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8
    assert np.array_equal(out, _want(shape, 8))
    assert cr.remove_noise(_crops(shape)[:0]).shape == (0, *shape, 3)
    with pytest.raises(ValueError, match="denoise"):
        Cropper(output_size=48, **given).remove_noise(_crops(shape))


# ---- end to end: process_dir on given landmarks
SIZE = (64, 64)
STRENGTH = 8


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
    """Three files with a landmark set each (the scene of tests/denoise_ref.py with seeded noise, the landmarks the target
    points), the crops a Cropper without ``denoise`` writes for them, and the reference applied to those crops."""
    from PIL import Image
    d = tmp_path_factory.mktemp("denoise_in")
    faces = np.stack([R.noisy(R.scene(*SIZE), 8.0, seed) for seed in (1, 2, 3)])
    imgs = {f"{n}.png": face for n, face in zip("abc", faces)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name, compress_level=1)
    tgt = A.landmarks_target(SIZE, 0.65)
    landmarks = (np.stack([tgt, tgt, tgt]).astype(np.float32), np.array(sorted(imgs)))
    out = tmp_path_factory.mktemp("denoise_plain")
    _cropper(landmarks).process_dir(str(d), str(out), desc=None)
    plain = _tree(out)
    assert sorted(plain) == sorted(imgs)
    crops = np.stack([_pixels(plain[n]) for n in sorted(plain)])
    want = R.denoise(crops, STRENGTH)
    assert all(not np.array_equal(a, b) for a, b in zip(want, crops))
    return {"dir": d, "landmarks": landmarks, "plain": plain, "crops": crops, "want": want}


def test_process_dir_writes_the_denoised_crops(device, scene, tmp_path):
    c = _cropper(scene["landmarks"], denoise=STRENGTH)
    assert c.denoise == 8.0 and c.par_model is None
    c.process_dir(str(scene["dir"]), str(tmp_path / "dn"), desc=None)
    got = _tree(tmp_path / "dn")
    assert sorted(got) == sorted(scene["plain"])
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), scene["want"][k]), n
    # the device encoders see the denoised crop as well
    c = _cropper(scene["landmarks"], denoise=STRENGTH, png_encoder="device")
    c.process_dir(str(scene["dir"]), str(tmp_path / "dev"), desc=None)
    for k, (n, data) in enumerate(sorted(_tree(tmp_path / "dev").items())):
        assert np.array_equal(_pixels(data), scene["want"][k]), n


def test_clahe_equalises_the_denoised_crop(device, scene, tmp_path):
    c = _cropper(scene["landmarks"], denoise=STRENGTH, clahe=2.0)
    want = c.equalize(c.remove_noise(scene["crops"]))
    assert np.array_equal(c.remove_noise(scene["crops"]), scene["want"])
    c.process_dir(str(scene["dir"]), str(tmp_path / "both"), desc=None)
    got = _tree(tmp_path / "both")
    assert sorted(got) == sorted(scene["plain"])
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), want[k]), n
        assert not np.array_equal(want[k], scene["want"][k])


def test_mask_files_are_the_same_with_and_without_denoise(device, scene, tmp_path):
    """The parser sees the original crop: the files of mask_groups do not move, the crops do."""
    groups = {"all": list(range(19))}
    _cropper(scene["landmarks"], mask_groups=groups).process_dir(str(scene["dir"]), str(tmp_path / "plain"), desc=None)
    _cropper(scene["landmarks"], mask_groups=groups, denoise=STRENGTH).process_dir(str(scene["dir"]), str(tmp_path / "dn"), desc=None)
    base, got = _tree(tmp_path / "plain"), _tree(tmp_path / "dn")
    assert sorted(base) == sorted(got)
    masks = [n for n in got if "_mask" + os.sep in n]
    assert len(masks) == 3
    names = sorted(scene["plain"])
    for n in got:
        if n in masks:
            assert got[n] == base[n], n
        else:
            assert np.array_equal(_pixels(got[n]), scene["want"][names.index(os.path.basename(n))]), n
