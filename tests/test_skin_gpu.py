"""Cropper(smooth_skin=S) on the GPU: the skin kernel against tests/skin_ref.py byte for byte (no tolerance anywhere),
through ctypes and through the torch op: sizes below the feather radius and the window, no multiple of the 32 x 64 tile,
exactly one tile, several tiles both ways; the three radii 3, 9 and 24; label maps with random classes, blocks, all skin,
no skin and labels that never count; arbitrary tables at the sums' maxima; the crops of a batch one by one, F = 0,
Cropper.retouch, and process_dir end to end."""
import ctypes
import importlib.util
import io
import itertools
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(os.path.dirname(__file__), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("skin_ref")
M = _load("matte_ref")
SHAPES = [(1, 1), (3, 5), (33, 47), (64, 64), (70, 130)]
SETTINGS = [(0.5, 1, 1.0), (3, 10, 1.0), (8, 64, 0.05), (3, 64, 0.05), (8, 10, 1.0)]     # (sigma, S, amount): r = 3, 9, 24
BITS = R.DEFAULT_BITS
_CASES, _WANT = {}, {}


def _case(shape):
    """(crops (4,h,w,3), {name: labels (4,h,w)}) of one shape.  Crops: uniform noise, gradient plus noise, a 0/255
    checkerboard, constant 255.  Labels: random classes 0..18; blocks of 5 x 7 of skin, hair and background; all skin; no
    skin; and labels that never count (19, 31, 32, 255) with a few skin pixels among them."""
    if shape not in _CASES:
        h, w = shape
        rng = np.random.default_rng(1000 * h + w)
        y, x = np.mgrid[0:h, 0:w]
        ramp = np.stack([30 + 180 * x / max(w - 1, 1), 200 - 150 * y / max(h - 1, 1), 60 + 60 * (x + y) / max(h + w - 2, 1)], -1)
        gradient = np.clip(np.rint(ramp + rng.normal(0, 6, (h, w, 3))), 0, 255).astype(np.uint8)
        checker = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
        crops = np.stack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), gradient, checker, np.full((h, w, 3), 255, np.uint8)])
        blocks = np.array([1, 17, 0, 10, 14, 2], np.uint8)[((y // 5) * 3 + x // 7) % 6]
        never = np.array([19, 31, 32, 255], np.uint8)[rng.integers(0, 4, (4, h, w))]
        never[rng.random((4, h, w)) < 0.2] = 1
        labels = {"random": rng.integers(0, 19, (4, h, w)).astype(np.uint8),
                  "blocks": np.stack([blocks, np.roll(blocks, 3, 1), blocks.T[:h, :w] if h == w else blocks[::-1], blocks[:, ::-1]]),
                  "skin": np.full((4, h, w), 1, np.uint8), "none": np.full((4, h, w), 17, np.uint8), "never": never}
        _CASES[shape] = crops, {k: np.ascontiguousarray(v) for k, v in labels.items()}
    return _CASES[shape]


def _want(shape, name, setting):
    """The reference of the four crops of a shape under one label map and one setting, computed once."""
    key = (shape, name, setting)
    if key not in _WANT:
        crops, labels = _case(shape)
        sigma, strength, amount = setting
        _WANT[key] = R.smooth_skin(crops, labels[name], strength, sigma, amount)
    return _WANT[key]


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _unchanged_off_the_skin(got, crops, labels, bits=BITS):
    off = R.mask01(labels, bits) == 0
    return np.array_equal(got[off], crops[off])


@pytest.mark.parametrize("setting", SETTINGS[:3], ids=lambda s: f"sigma{s[0]}-S{s[1]}-a{s[2]}")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_reference(device, shape, setting):
    from face_crop_plus_amd import skin as S
    sigma, strength, amount = setting
    assert len(S.taps_of(sigma)) - 1 == {0.5: 3, 3: 9, 8: 24}[sigma]
    crops, labels = _case(shape)
    src = _dev(crops, device)
    for name in ("random", "blocks", "skin", "none", "never"):
        want = _want(shape, name, setting)
        got = S.smooth(src, _dev(labels[name], device), strength, sigma, amount)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (4, *shape, 3)
        got = got.cpu().numpy()
        assert np.array_equal(got, want), name
        assert _unchanged_off_the_skin(got, crops, labels[name]), name          # a condition, not a measurement
        if name == "none":
            assert np.array_equal(got, crops)
    assert np.array_equal(src.cpu().numpy(), crops)                              # the input is untouched
    if min(shape) >= 33 and amount == 1.0:
        assert not np.array_equal(_want(shape, "skin", setting)[0], crops[0])    # the filter does something


@pytest.mark.parametrize("setting", SETTINGS[3:], ids=lambda s: f"sigma{s[0]}-S{s[1]}-a{s[2]}")
def test_the_other_pairings_of_strength_and_amount(device, setting):
    """S = 64 at r = 9 with the smallest amount, and S = 10 at r = 24 with the whole: on the shape of several tiles."""
    from face_crop_plus_amd import skin as S
    sigma, strength, amount = setting
    shape = (70, 130)
    crops, labels = _case(shape)
    for name in ("random", "blocks"):
        got = S.smooth(_dev(crops, device), _dev(labels[name], device), strength, sigma, amount).cpu().numpy()
        assert np.array_equal(got, _want(shape, name, setting)), name
        assert _unchanged_off_the_skin(got, crops, labels[name]), name


def test_batch_behaviour(device):
    from face_crop_plus_amd import skin as S
    shape, setting = (33, 47), SETTINGS[1]
    sigma, strength, amount = setting
    crops, labels = _case(shape)
    src, lab = _dev(crops, device), _dev(labels["blocks"], device)
    whole = S.smooth(src, lab, strength, sigma, amount)
    assert np.array_equal(whole.cpu().numpy(), _want(shape, "blocks", setting))
    assert torch.equal(S.smooth(src, lab, strength, sigma, amount), whole)                 # the same bytes from run to run
    for k in (0, 2):                                                                        # a crop of the batch equals it run alone
        assert torch.equal(S.smooth(src[k:k + 1].contiguous(), lab[k:k + 1].contiguous(), strength, sigma, amount)[0], whole[k])
    empty = S.smooth(src[:0], lab[:0], strength, sigma, amount)                            # F = 0
    assert tuple(empty.shape) == (0, *shape, 3) and empty.dtype == torch.uint8
    assert np.array_equal(src.cpu().numpy(), crops) and np.array_equal(lab.cpu().numpy(), labels["blocks"])
    # other class sets: one class, every class, a class that is absent
    for bits in (1 << 17, (1 << 19) - 1, 1 << 5):
        got = S.smooth(src, lab, strength, sigma, amount, class_bits=bits).cpu().numpy()
        assert np.array_equal(got, R.smooth(crops, labels["blocks"], bits, R.blur_taps(sigma), R.range_lut(strength), 256)), bits
        assert _unchanged_off_the_skin(got, crops, labels["blocks"], bits)


def _entry(crops, labels, bits, taps, table, amount, device):
    from face_crop_plus_amd import skin as S
    return S.skin_smooth(_dev(crops, device), _dev(labels, device), bits, taps, _dev(np.asarray(table, np.uint16), device), amount).cpu().numpy()


@pytest.mark.parametrize("shape", [(33, 47), (70, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_any_table(device, shape):
    crops, labels = _case(shape)
    white, skin = crops[3:], labels["skin"][3:]
    full = np.full(256, 65535, np.uint16)
    # all taps 4096 at r = 24, every table entry clamps to 4096, all skin, all 255: the sums sit at their maxima
    got = _entry(white, skin, BITS, [4096] * 25, full, 256, device)
    assert (got == 255).all() and np.array_equal(got, R.smooth(white, skin, BITS, [4096] * 25, full, 256))
    got = _entry(crops[:2], labels["skin"][:2], BITS, [4096] * 25, full, 256, device)       # a box mean over the crop's pixels
    assert np.array_equal(got, R.smooth(crops[:2], labels["skin"][:2], BITS, [4096] * 25, full, 256))
    # centre tap 0 and a zero table: W == 0 copies
    assert np.array_equal(_entry(crops, labels["random"], BITS, [0, 7, 7, 7], np.zeros(256, np.uint16), 256, device), crops)
    assert np.array_equal(_entry(crops, labels["skin"], BITS, [0] * 10, full, 256, device), crops)       # every s == 0
    # a table that is not monotone, with zeros first, and taps that are not a Gaussian
    rng = np.random.default_rng(7)
    odd = rng.integers(0, 9000, 256).astype(np.uint16)
    odd[:3] = 0
    for taps, amount in (([5, 4096, 0, 900, 64], 256), ([4096, 1, 1, 2000], 77)):
        for name in ("random", "blocks"):
            got = _entry(crops, labels[name], BITS, taps, odd, amount, device)
            assert np.array_equal(got, R.smooth(crops, labels[name], BITS, taps, odd, amount)), (taps, name)
            assert _unchanged_off_the_skin(got, crops, labels[name])


def test_unaligned_views_and_guard_bytes(device):
    """Crops, labels and out that start at odd bytes, with guard bytes around out: nothing outside out is written."""
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import skin as S
    shape, setting = (33, 47), SETTINGS[1]
    crops, labels = _case(shape)
    h, w = shape
    n, guard = crops[:2].size, 64
    cbuf = torch.zeros(n + 3, dtype=torch.uint8, device=device)
    cbuf[3:] = _dev(crops[:2].reshape(-1), device)
    lbuf = torch.zeros(n // 3 + 1, dtype=torch.uint8, device=device)
    lbuf[1:] = _dev(labels["blocks"][:2].reshape(-1), device)
    obuf = torch.full((n + 2 * guard + 1,), 0xA5, dtype=torch.uint8, device=device)
    table = _dev(R.range_lut(10), device)
    taps = R.blur_taps(3)
    t16 = (ctypes.c_uint16 * len(taps))(*taps)
    N.check(N.lib().fcp_skin_smooth_u8(ctypes.c_void_p(cbuf.data_ptr() + 3), ctypes.c_void_p(lbuf.data_ptr() + 1), 2, h, w, BITS, t16,
                                       len(taps) - 1, N.ptr(table), 256, ctypes.c_void_p(obuf.data_ptr() + guard + 1), N.stream_ptr()),
            "fcp_skin_smooth_u8")
    torch.cuda.synchronize()
    out = obuf.cpu().numpy()
    assert (out[:guard + 1] == 0xA5).all() and (out[guard + 1 + n:] == 0xA5).all()
    assert np.array_equal(out[guard + 1:guard + 1 + n].reshape(2, h, w, 3), _want(shape, "blocks", setting)[:2])


def test_boundaries_give_identical_tensors_and_refuse_bad_inputs(device, monkeypatch):
    from face_crop_plus_amd import skin as S
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    shape = (33, 47)
    crops, labels = _case(shape)
    src, lab = _dev(crops, device), _dev(labels["random"], device)
    for setting in SETTINGS[:3]:
        sigma, strength, amount = setting
        res = {}
        for enabled in (True, False):
            monkeypatch.setattr(T, "ENABLED", enabled)
            res[enabled] = S.smooth(src, lab, strength, sigma, amount)
        assert torch.equal(res[True], res[False])
        assert np.array_equal(res[True].cpu().numpy(), _want(shape, "random", setting))
    table = _dev(R.range_lut(10), device)
    taps = R.blur_taps(3)
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        with pytest.raises(RuntimeError, match="radius 3..24"):
            S.skin_smooth(src, lab, BITS, taps[:3], table, 256)
        with pytest.raises(RuntimeError, match="radius 3..24"):
            S.skin_smooth(src, lab, BITS, [1] * 26, table, 256)
        with pytest.raises(RuntimeError, match="tap 1 is 4097"):
            S.skin_smooth(src, lab, BITS, [1, 4097, 1, 1], table, 256)
        with pytest.raises(RuntimeError, match="amount_q8 must be 1..256"):
            S.skin_smooth(src, lab, BITS, taps, table, 0)
        with pytest.raises(RuntimeError, match="class at or above 19"):
            S.skin_smooth(src, lab, 1 << 19, taps, table, 256)
        for bad in (src.float(), src[:, :, ::2], src[..., :2], src[0]):
            with pytest.raises(AssertionError):
                S.skin_smooth(bad, lab, BITS, taps, table, 256)
        for bad in (lab.float(), lab[:, :, ::2], lab[:3], lab.cpu()):
            with pytest.raises(AssertionError):
                S.skin_smooth(src, bad, BITS, taps, table, 256)
        for bad in (table.to(torch.int32), table[:255], table.cpu()):
            with pytest.raises(AssertionError):
                S.skin_smooth(src, lab, BITS, taps, bad, 256)
    ops = T.load()
    for bad in (src.float(), src[:, :, ::2], src[0]):                                   # the op itself refuses them too
        with pytest.raises(RuntimeError):
            ops.skin_smooth(bad, lab, BITS, taps, table, 256)
    for bad in (lab.float(), lab[:, :, ::2], lab[:3], lab.cpu()):
        with pytest.raises(RuntimeError):
            ops.skin_smooth(src, bad, BITS, taps, table, 256)
    for bad in (table.to(torch.int32), table[:255], table.cpu(), table[None]):
        with pytest.raises(RuntimeError):
            ops.skin_smooth(src, lab, BITS, taps, bad, 256)


def test_cropper_retouch_equals_reference(device):
    from face_crop_plus_amd import Cropper
    given = dict(landmarks=(np.zeros((1, 5, 2), np.float32), np.array(["a"])), det_threshold=None, device="cuda:0",
                 weights={"bisenet": "generated"})
    shape = (33, 47)
    crops, labels = _case(shape)
    cr = Cropper(output_size=48, smooth_skin=10, **given)
    assert cr.smooth_skin == 10.0 and cr.par_model is not None and cr._has_background() is False
    out = cr.retouch(crops, labels["blocks"])
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8
    assert np.array_equal(out, _want(shape, "blocks", SETTINGS[1]))
    assert cr.retouch(crops[:0], labels["blocks"][:0]).shape == (0, *shape, 3)
    cr = Cropper(output_size=48, smooth_skin=64, smooth_sigma=8, smooth_amount=0.05, skin_classes=[17, 1], **given)
    want = R.smooth_skin(crops, labels["blocks"], 64, 8, 0.05, (1, 17))
    assert np.array_equal(cr.retouch(crops, labels["blocks"]), want)
    with pytest.raises(ValueError, match="smooth_skin"):
        Cropper(output_size=48, **given).retouch(crops, labels["blocks"])


# ---- end to end: process_dir on given landmarks
SIZE = (64, 64)
STRENGTH = 10
FILL = (10, 200, 30)


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
    the crops are about those faces), their plain crops, the label maps the Cropper's own parser gives those crops, a
    class set under which every crop has plenty of skin and of other pixels, and the reference applied to the plain crops."""
    from PIL import Image
    d = tmp_path_factory.mktemp("skin_in")
    faces = np.load(os.path.join(os.path.dirname(__file__), "golden", "bisenet.npz"))["faces"]
    assert faces.shape == (3, *SIZE, 3)
    imgs = {f"{n}.png": face for n, face in zip("abc", faces)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name, compress_level=1)
    tgt = A.landmarks_target(SIZE, 0.65)
    landmarks = (np.stack([tgt, tgt, tgt]).astype(np.float32), np.array(sorted(imgs)))
    out = tmp_path_factory.mktemp("skin_plain")
    c = _cropper(landmarks)
    assert c.par_model is None
    c.process_dir(str(d), str(out), desc=None)
    plain = _tree(out)
    assert sorted(plain) == sorted(imgs)
    crops = np.stack([_pixels(plain[n]) for n in sorted(plain)])
    parser = _cropper(landmarks, smooth_skin=STRENGTH).par_model                 # smooth_skin alone creates the parser
    assert parser is not None
    labels = parser.predict(torch.from_numpy(crops).to("cuda:0"), return_labels=True)[-1].cpu().numpy()
    present = [np.unique(l) for l in labels]
    print("classes per crop:", [p.tolist() for p in present])
    classes = sorted(set(np.concatenate(present).tolist()))
    skin = None
    for n in (1, 2, 3):
        for cand in itertools.combinations(classes, n):
            hard = np.isin(labels, cand)
            if all(m.sum() > 200 and (~m).sum() > 200 for m in hard):
                skin = list(cand)
                break
        if skin is not None:
            break
    # not vacuous: without such a set the step would copy the crop or smooth all of it
    assert skin is not None, f"the generated parser gives no class set that splits every crop: {present}"
    want = R.smooth_skin(crops, labels, STRENGTH, classes=skin)
    assert all(not np.array_equal(a, b) for a, b in zip(want, crops))
    return {"dir": d, "landmarks": landmarks, "plain": plain, "crops": crops, "labels": labels, "skin": skin, "want": want}


def test_process_dir_writes_the_smoothed_crops(device, scene, tmp_path):
    c = _cropper(scene["landmarks"], smooth_skin=STRENGTH, skin_classes=scene["skin"])
    assert c.smooth_skin == 10.0 and c.par_model is not None and not c._has_background()
    c.process_dir(str(scene["dir"]), str(tmp_path / "sk"), desc=None)
    got = _tree(tmp_path / "sk")
    assert sorted(got) == sorted(scene["plain"])
    off = ~np.isin(scene["labels"], scene["skin"])
    for k, n in enumerate(sorted(got)):
        px = _pixels(got[n])
        assert np.array_equal(px, scene["want"][k]), n
        assert np.array_equal(px[off[k]], scene["crops"][k][off[k]]), n
    assert np.array_equal(c.retouch(scene["crops"], scene["labels"]), scene["want"])
    # the device encoder sees the smoothed crop as well
    c = _cropper(scene["landmarks"], smooth_skin=STRENGTH, skin_classes=scene["skin"], png_encoder="device")
    c.process_dir(str(scene["dir"]), str(tmp_path / "dev"), desc=None)
    dev = _tree(tmp_path / "dev")
    assert sorted(dev) == sorted(scene["plain"])
    for k, n in enumerate(sorted(dev)):
        assert np.array_equal(_pixels(dev[n]), scene["want"][k]), n


def test_mask_files_are_the_same_with_and_without_smooth_skin(device, scene, tmp_path):
    """The parser sees the original crop: the files of mask_groups do not move, the crops do."""
    groups = {"all": list(range(19))}
    _cropper(scene["landmarks"], mask_groups=groups).process_dir(str(scene["dir"]), str(tmp_path / "plain"), desc=None)
    _cropper(scene["landmarks"], mask_groups=groups, smooth_skin=STRENGTH, skin_classes=scene["skin"]).process_dir(
        str(scene["dir"]), str(tmp_path / "sk"), desc=None)
    base, got = _tree(tmp_path / "plain"), _tree(tmp_path / "sk")
    assert sorted(base) == sorted(got)
    masks = [n for n in got if "_mask" + os.sep in n]
    assert len(masks) == 3
    names = sorted(scene["plain"])
    for n in got:
        if n in masks:
            assert got[n] == base[n], n
        else:
            assert np.array_equal(_pixels(got[n]), scene["want"][names.index(os.path.basename(n))]), n


def test_a_background_mattes_the_smoothed_crop_and_the_batch_is_parsed_once(device, scene, tmp_path, monkeypatch):
    from face_crop_plus_amd import bise
    calls = []
    real = bise.BiSeNet.parse
    monkeypatch.setattr(bise.BiSeNet, "parse", lambda self, faces: (calls.append(int(faces.shape[0])), real(self, faces))[1])
    c = _cropper(scene["landmarks"], smooth_skin=STRENGTH, skin_classes=scene["skin"], background=FILL, foreground=scene["skin"])
    c.process_dir(str(scene["dir"]), str(tmp_path / "bg"), desc=None)
    assert sorted(calls) == [1, 2]                                   # three files in batches of two: one parse per batch
    bits = sum(1 << k for k in scene["skin"])
    want, _ = M.matte(scene["want"], scene["labels"], bits, 5, FILL)
    plain, _ = M.matte(scene["crops"], scene["labels"], bits, 5, FILL)
    got = _tree(tmp_path / "bg")
    assert sorted(got) == sorted(scene["plain"])
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), want[k]), n
        assert not np.array_equal(want[k], plain[k])
    del calls[:]
    c = _cropper(scene["landmarks"], smooth_skin=STRENGTH, skin_classes=scene["skin"])
    c.process_dir(str(scene["dir"]), str(tmp_path / "alone"), desc=None)
    assert sorted(calls) == [1, 2]


def test_denoise_first_and_clahe_after(device, scene, tmp_path):
    c = _cropper(scene["landmarks"], smooth_skin=STRENGTH, skin_classes=scene["skin"], denoise=8, clahe=2.0)
    want = c.equalize(c.retouch(c.remove_noise(scene["crops"]), scene["labels"]))
    c.process_dir(str(scene["dir"]), str(tmp_path / "all"), desc=None)
    got = _tree(tmp_path / "all")
    assert sorted(got) == sorted(scene["plain"])
    other = c.equalize(c.remove_noise(c.retouch(scene["crops"], scene["labels"])))
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), want[k]), n
    assert not np.array_equal(want, other)                           # the order shows
