"""Cropper(refine=...) on the GPU: the two guided-filter launches against tests/matte_refine_ref.py byte for byte (sizes
below and around the 64 x 32 tile, radii 1, 2 and 16 -- at 16 the halo of both sides is a tile's height --, eps 1, 64 and
4096, the label patterns of the background blur and the stripes that need the wide accumulators), the two composites
through the refined alpha, label bytes past the classes, guard bytes around offset views, repeated calls, in place, both
boundaries, Cropper.matte, and process_dir end to end on given landmarks."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 32                      # kTileW, kTileH of csrc/fcp_matte_refine.hip, both kernels
SMALL = [(1, 1), (1, 2), (2, 1), (3, 3), (5, 4), (7, 7), (33, 65), (96, 80),
         (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1)]
SMALL = list(dict.fromkeys(SMALL))           # (33, 65) is the tile plus one as well
RADII = (1, 2, 16)                           # 2 * 16 == TILE_H: the halo is as tall as the tile
EPS = (1, 64, 4096)
BIG, BIG_RADIUS, BIG_EPS = (256, 256), 8, 64
ONE_17 = (1 << 1) | (1 << 17)
FILL = (0, 177, 64)


def _load(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(os.path.dirname(__file__), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("matte_refine_ref")
RB = _load("matte_blur_ref")
MR = R.MR
_INPUTS, _ALPHA = {}, {}


def _inputs(shape):
    """shape -> crops (3,h,w,3) and {pattern: labels (3,h,w)}, made once."""
    if shape not in _INPUTS:
        h, w = shape
        rng = np.random.default_rng(1000 * h + w)
        _INPUTS[shape] = (MR.random_crops(rng, 3, h, w), {p: RB.labels_of(p, rng, 3, h, w) for p in RB.PATTERNS})
    return _INPUTS[shape]


def _case(shape, pattern, r):
    """(crops, labels) of a case: the stripes bring their own crops (gray 254 / 255) and a width of r + 1."""
    if pattern == "stripes":
        return R.stripe_inputs(3, shape[0], shape[1], r)
    crops, labels = _inputs(shape)
    return crops, labels[pattern]


def _alpha(shape, pattern, bits, r, eps):
    """The reference alpha of a case, computed once and shared by every test."""
    key = (shape, pattern, bits, r, eps)
    if key not in _ALPHA:
        crops, labels = _case(shape, pattern, r)
        _ALPHA[key] = R.alpha_of(crops, labels, bits, r, eps)
    return _ALPHA[key]


def _combos(shape):
    if shape == BIG:
        return [("random", ONE_17)]
    if shape[0] * shape[1] > 3000:
        return [("random", ONE_17), ("one_bg", MR.DEFAULT_BITS), ("stripes", MR.DEFAULT_BITS)]
    return [(p, MR.DEFAULT_BITS) for p in RB.PATTERNS] + [("random", ONE_17), ("checker", 1), ("stripes", MR.DEFAULT_BITS)]


def _refine(crops, labels, bits, r, eps, alpha):
    """The C entry point itself, on the pointers as given (views)."""
    from face_crop_plus_amd import _native as N
    f, h, w, _ = crops.shape
    need = N.lib().fcp_matte_refine_workspace_bytes(f, h, w)
    assert need == 8 * f * h * w
    work = torch.empty((need,), dtype=torch.uint8, device=crops.device)
    N.check(N.lib().fcp_matte_refine_u8(N.ptr(crops), N.ptr(labels), f, h, w, bits, r, eps, N.ptr(alpha), N.ptr(work), need,
                                        N.stream_ptr()), "fcp_matte_refine_u8")


def _fill(crops, alpha, fill, out):
    from face_crop_plus_amd import _native as N
    f, h, w, _ = crops.shape
    N.check(N.lib().fcp_matte_alpha_u8(N.ptr(crops), N.ptr(alpha), f, h, w, *fill, N.ptr(out), N.stream_ptr()), "fcp_matte_alpha_u8")


def _blur(crops, labels, alpha, bits, taps, out):
    import ctypes
    from face_crop_plus_amd import _native as N
    f, h, w, _ = crops.shape
    need = N.lib().fcp_matte_blur_workspace_bytes(f, h, w)
    work = torch.empty((need,), dtype=torch.uint8, device=crops.device)
    t16 = (ctypes.c_uint16 * len(taps))(*taps)
    N.check(N.lib().fcp_matte_blur_alpha_u8(N.ptr(crops), N.ptr(labels), N.ptr(alpha), f, h, w, bits, t16, len(taps) - 1, N.ptr(out),
                                            N.ptr(work), need, N.stream_ptr()), "fcp_matte_blur_alpha_u8")


@pytest.mark.parametrize("shape", SMALL + [BIG], ids=lambda s: f"{s[0]}x{s[1]}")
def test_alpha_equals_reference(device, shape):
    from face_crop_plus_amd import matte as M
    checked = 0
    for pattern, bits in _combos(shape):
        for r in ((BIG_RADIUS,) if shape == BIG else RADII):
            crops, labels = _case(shape, pattern, r)
            crops_dev, lab_dev = torch.from_numpy(crops).to(device), torch.from_numpy(labels).to(device)
            for eps in ((BIG_EPS,) if shape == BIG else EPS):
                want = _alpha(shape, pattern, bits, r, eps)
                for f in (3, 1):
                    alpha = M.refine_alpha(crops_dev[:f], lab_dev[:f], bits, r, eps)
                    assert alpha.dtype == torch.uint8 and tuple(alpha.shape) == (f, *shape)
                    got = alpha.cpu().numpy()
                    assert np.array_equal(got, want[:f]), ((shape, pattern, hex(bits), r, eps, f), int((got != want[:f]).sum()))
                    checked += 1
    assert checked == len(_combos(shape)) * (1 if shape == BIG else len(RADII) * len(EPS)) * 2


def test_the_cases_are_not_trivial():
    """From the reference alone: soft values, a dependence on the guide, on the radius and on eps, and the wide sums."""
    shape = (33, 65)
    crops, labels = _inputs(shape)
    for r in RADII:
        for eps in EPS:
            alpha = _alpha(shape, "random", ONE_17, r, eps)
            assert len(np.unique(alpha)) > 16
    assert not np.array_equal(_alpha(shape, "random", ONE_17, 2, 64), _alpha(shape, "random", ONE_17, 16, 64))
    assert not np.array_equal(_alpha(shape, "random", ONE_17, 2, 1), _alpha(shape, "random", ONE_17, 2, 4096))
    other = R.alpha_of(crops[::-1], labels["random"], ONE_17, 2, 64)
    assert not np.array_equal(other, _alpha(shape, "random", ONE_17, 2, 64))
    assert (_alpha(shape, "all_fg", MR.DEFAULT_BITS, 16, 1) == 255).all() and (_alpha(shape, "all_bg", MR.DEFAULT_BITS, 16, 1) == 0).all()
    guide, p = R.stripes(96, 80, 16)
    a, b = R.coefficients(guide, p, 16, 1)
    assert np.abs(b).max() > 2 ** 25 and np.abs(R.box(b, 16)).max() > 2 ** 35
    sc, sl = R.stripe_inputs(3, 96, 80, 16)
    assert np.array_equal(R.gray(sc[0]), guide) and np.array_equal(MR.mask(sl[0], MR.DEFAULT_BITS), p)


@pytest.mark.parametrize("shape", [(33, 65), (5, 4), (96, 80)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_composites_equal_reference(device, shape):
    """Fill mode and blur mode through the refined alpha; the blurred background is the hard mask's, as without refine."""
    from face_crop_plus_amd import matte as M
    crops, labels = _inputs(shape)
    crops_dev = torch.from_numpy(crops).to(device)
    checked = met = 0
    for pattern, bits in (("random", ONE_17), ("one_bg", MR.DEFAULT_BITS), ("corners", MR.DEFAULT_BITS)):
        lab = labels[pattern]
        lab_dev = torch.from_numpy(lab).to(device)
        for r, eps, sigma in ((16, 1, 0.5), (2, 64, 5.34), (1, 4096, 16)):
            taps = M.blur_taps(sigma)
            want_a = _alpha(shape, pattern, bits, r, eps)
            alpha = M.refine_alpha(crops_dev, lab_dev, bits, r, eps)
            assert np.array_equal(alpha.cpu().numpy(), want_a)
            out, back = M.matte(crops_dev, lab_dev, bits, 0, FILL, with_alpha=True, alpha=alpha)
            assert back is alpha and np.array_equal(out.cpu().numpy(), MR.composite(crops, want_a, FILL)), (shape, pattern, r, eps)
            assert M.matte(crops_dev, lab_dev, bits, 0, FILL, alpha=alpha)[1] is None
            bg, d = RB.background(crops, lab, bits, taps)
            met += int(((want_a < 255) & (d == 0)).sum())
            out, back = M.matte_blur(crops_dev, lab_dev, bits, 0, taps, with_alpha=True, alpha=alpha)
            got = out.cpu().numpy()
            assert back is alpha and np.array_equal(got, RB.over(crops, want_a, bg)), (shape, pattern, r, eps, sigma)
            hidden = (want_a < 255) & (d == 0)
            assert np.array_equal(got[hidden], crops[hidden])                 # no background in sight: the pixel keeps its crop
            checked += 1
    assert checked == 9
    if shape == (33, 65):
        assert met > 0                                                        # alpha < 255 met D == 0


def test_labels_past_the_classes_are_background(device):
    from face_crop_plus_amd import matte as M
    rng = np.random.default_rng(5)
    h, w = 37, 70
    labels = rng.choice(np.array([0, 1, 17, 18, 19, 31, 32, 33, 63, 64, 128, 255], np.uint8), (2, h, w))
    crops = MR.random_crops(rng, 2, h, w)
    for bits in (MR.DEFAULT_BITS, ONE_17, 1, (1 << 19) - 1):
        hard = MR.mask(labels, bits)
        assert not hard[labels >= 19].any() and hard.any()
        for r, eps in ((1, 1), (16, 64)):
            alpha = M.refine_alpha(torch.from_numpy(crops).to(device), torch.from_numpy(labels).to(device), bits, r, eps)
            assert np.array_equal(alpha.cpu().numpy(), R.alpha_of(crops, labels, bits, r, eps)), (hex(bits), r)


@pytest.mark.parametrize("shape", [(7, 7), (33, 65), (5, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bytes_and_offset_views(device, shape):
    crops, labels = _inputs(shape)
    lab = labels["random"]
    f, (h, w) = 3, shape
    G = 64
    bits = MR.DEFAULT_BITS
    taps = RB.blur_taps(0.5)
    bg = RB.background(crops, lab, bits, taps)[0]
    for lead in (1, 2, 3):
        for r, eps in ((1, 1), (16, 64), (2, 4096)):
            want_a = _alpha(shape, "random", bits, r, eps)
            # inputs: views that start `lead` bytes into a buffer and end exactly where it ends
            cbuf = torch.zeros(lead + crops.size, dtype=torch.uint8, device=device)
            lbuf = torch.zeros(lead + lab.size, dtype=torch.uint8, device=device)
            cbuf[lead:].copy_(torch.from_numpy(crops.reshape(-1)).to(device))
            lbuf[lead:].copy_(torch.from_numpy(lab.reshape(-1)).to(device))
            cv, lv = cbuf[lead:].view(crops.shape), lbuf[lead:].view(f, h, w)
            assert cv.data_ptr() % 4 == lead and lv.data_ptr() % 4 == lead
            # outputs: between 64 guard bytes, at the same odd offsets
            abuf = torch.full((G + lead + f * h * w + G,), 0x5A, dtype=torch.uint8, device=device)
            av = abuf[G + lead:G + lead + f * h * w].view(f, h, w)
            _refine(cv, lv, bits, r, eps, av)
            a = abuf.cpu().numpy()
            what = (shape, lead, r, eps)
            assert (a[:G + lead] == 0x5A).all() and (a[G + lead + f * h * w:] == 0x5A).all(), what
            assert np.array_equal(a[G + lead:G + lead + f * h * w].reshape(f, h, w), want_a), what
            # the composites read the alpha at its odd offset and, ending at its buffer's end, as an input
            ain = torch.zeros(lead + f * h * w, dtype=torch.uint8, device=device)
            ain[lead:].copy_(av.reshape(-1))
            ainv = ain[lead:].view(f, h, w)
            for mode, want in (("fill", MR.composite(crops, want_a, FILL)), ("blur", RB.over(crops, want_a, bg))):
                obuf = torch.full((G + lead + crops.size + G,), 0xA5, dtype=torch.uint8, device=device)
                ov = obuf[G + lead:G + lead + crops.size].view(crops.shape)
                if mode == "fill":
                    _fill(cv, ainv, FILL, ov)
                else:
                    _blur(cv, lv, ainv, bits, taps, ov)
                o = obuf.cpu().numpy()
                assert (o[:G + lead] == 0xA5).all() and (o[G + lead + crops.size:] == 0xA5).all(), (what, mode)
                assert np.array_equal(o[G + lead:G + lead + crops.size].reshape(crops.shape), want), (what, mode)
            assert np.array_equal(ain[lead:].cpu().numpy(), want_a.reshape(-1))             # the inputs are untouched
            assert np.array_equal(cbuf[lead:].cpu().numpy(), crops.reshape(-1))
            assert np.array_equal(lbuf[lead:].cpu().numpy(), lab.reshape(-1))


@pytest.mark.parametrize("shape", [(33, 65), (96, 80), (5, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_in_place_equals_out_of_place_and_calls_repeat(device, shape):
    crops, labels = _inputs(shape)
    lab = torch.from_numpy(labels["random"]).to(device)
    taps = RB.blur_taps(5.34)
    bg = RB.background(crops, labels["random"], ONE_17, taps)[0]
    for r, eps in ((1, 1), (16, 64)):
        want_a = _alpha(shape, "random", ONE_17, r, eps)
        src = torch.from_numpy(crops).to(device)
        alphas = []
        for _ in range(2):
            alpha = torch.empty_like(lab)
            _refine(src, lab, ONE_17, r, eps, alpha)
            alphas.append(alpha.cpu().numpy())
        assert np.array_equal(alphas[0], alphas[1]) and np.array_equal(alphas[0], want_a)
        for mode, want in (("fill", MR.composite(crops, want_a, FILL)), ("blur", RB.over(crops, want_a, bg))):
            outs = []
            for _ in range(2):
                out = torch.empty_like(src)
                _fill(src, alpha, FILL, out) if mode == "fill" else _blur(src, lab, alpha, ONE_17, taps, out)
                outs.append(out.cpu().numpy())
            assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], want), (shape, r, mode)
            place = src.clone()
            _fill(place, alpha, FILL, place) if mode == "fill" else _blur(place, lab, alpha, ONE_17, taps, place)   # out is crops
            assert np.array_equal(place.cpu().numpy(), want), (shape, r, mode)
        assert np.array_equal(src.cpu().numpy(), crops) and np.array_equal(alpha.cpu().numpy(), want_a)


def test_boundaries_give_identical_tensors(device, monkeypatch):
    from face_crop_plus_amd import matte as M
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    shape = (96, 80)
    crops, labels = _inputs(shape)
    cd, ld = torch.from_numpy(crops).to(device), torch.from_numpy(labels["random"]).to(device)
    taps = M.blur_taps(2.0)
    for r, eps in ((1, 1), (16, 64), (2, 4096)):
        res = {}
        for enabled in (True, False):
            monkeypatch.setattr(T, "ENABLED", enabled)
            alpha = M.refine_alpha(cd, ld, ONE_17, r, eps)
            res[enabled] = (alpha, M.matte(cd, ld, ONE_17, 0, FILL, alpha=alpha)[0], M.matte_blur(cd, ld, ONE_17, 0, taps, alpha=alpha)[0])
        for a, b in zip(res[True], res[False]):
            assert torch.equal(a, b)
        assert np.array_equal(res[True][0].cpu().numpy(), _alpha(shape, "random", ONE_17, r, eps))
    alpha = res[True][0]
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        for bad in (0, 17):
            with pytest.raises(RuntimeError, match="radius"):
                M.refine_alpha(cd, ld, ONE_17, bad, 64)
        for bad in (0, 4097):
            with pytest.raises(RuntimeError, match="eps"):
                M.refine_alpha(cd, ld, ONE_17, 4, bad)
        with pytest.raises(RuntimeError, match="class_bits"):
            M.refine_alpha(cd, ld, 1 << 19, 4, 64)
        with pytest.raises(RuntimeError, match="fill"):
            M.matte(cd, ld, ONE_17, 0, (0, 256, 0), alpha=alpha)
        with pytest.raises(RuntimeError, match="class_bits"):
            M.matte_blur(cd, ld, 1 << 19, 0, taps, alpha=alpha)
        with pytest.raises(RuntimeError, match="sum to 4096"):
            M.matte_blur(cd, ld, ONE_17, 0, taps[:-1], alpha=alpha)
        empty = M.refine_alpha(cd[:0], ld[:0], ONE_17, 4, 64)
        assert tuple(empty.shape) == (0, 96, 80)
        assert tuple(M.matte(cd[:0], ld[:0], ONE_17, 0, FILL, alpha=empty)[0].shape) == (0, 96, 80, 3)
        assert tuple(M.matte_blur(cd[:0], ld[:0], ONE_17, 0, taps, alpha=empty)[0].shape) == (0, 96, 80, 3)
    ops = T.load()
    with pytest.raises(RuntimeError, match="labels"):
        ops.matte_refine(cd, ld[:, :-1].contiguous(), ONE_17, 4, 64)
    with pytest.raises(RuntimeError, match="alpha"):
        ops.matte_alpha(cd, alpha[:, :-1].contiguous(), 0, 0, 0)
    with pytest.raises(RuntimeError, match="alpha"):
        ops.matte_blur_alpha(cd, ld, alpha[:2], ONE_17, taps)
    with pytest.raises(RuntimeError):
        ops.matte_refine(cd.float(), ld, ONE_17, 4, 64)


def test_cropper_matte_equals_reference(device):
    from face_crop_plus_amd import Cropper
    shape = (33, 65)
    crops, labels = _inputs(shape)
    lm = (np.zeros((1, 5, 2), np.float32), np.array(["a"]))
    c = Cropper(output_size=48, landmarks=lm, det_threshold=None, device="cuda:0", background=FILL, foreground=[1, 17], refine=2,
                weights={"bisenet": "generated"})
    assert (c.refine, c.refine_eps, c.feather) == (2, 64, 0) and c.par_model is not None
    out, alpha = c.matte(crops, labels["random"])
    want_a = _alpha(shape, "random", ONE_17, 2, 64)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and alpha.dtype == np.uint8
    assert np.array_equal(alpha, want_a) and np.array_equal(out, MR.composite(crops, want_a, FILL))
    out0, alpha0 = c.matte(crops[:0], labels["random"][:0])
    assert out0.shape == (0, 33, 65, 3) and alpha0.shape == (0, 33, 65)
    c = Cropper(output_size=48, landmarks=lm, det_threshold=None, device="cuda:0", background_blur=5.34, foreground=[1, 17], refine=16,
                refine_eps=1, weights={"bisenet": "generated"})
    out, alpha = c.matte(crops, labels["random"])
    want_a = _alpha(shape, "random", ONE_17, 16, 1)
    bg = RB.background(crops, labels["random"], ONE_17, RB.blur_taps(5.34))[0]
    assert np.array_equal(alpha, want_a) and np.array_equal(out, RB.over(crops, want_a, bg))


# ---- end to end: process_dir on given landmarks
SIGMA = 3.0
SIZE = (64, 64)
RADIUS, EPSILON = 4, 64


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
    """The recipe of tests/test_matte_blur_gpu.py: three files with a landmark set each, their plain crops, the label maps
    the Cropper's own parser gives them, and a foreground class set under which every crop has subject and background."""
    import itertools
    from PIL import Image
    d = tmp_path_factory.mktemp("refine_in")
    faces = np.load(os.path.join(os.path.dirname(__file__), "golden", "bisenet.npz"))["faces"]
    assert faces.shape == (3, *SIZE, 3)
    imgs = {f"{n}.png": face for n, face in zip("abc", faces)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name, compress_level=1)
    tgt = A.landmarks_target(SIZE, 0.65)
    landmarks = (np.stack([tgt, tgt, tgt]).astype(np.float32), np.array(sorted(imgs)))
    out = tmp_path_factory.mktemp("refine_plain")
    c = _cropper(landmarks)
    assert c.par_model is None
    c.process_dir(str(d), str(out), desc=None)
    plain = _tree(out)
    assert sorted(plain) == sorted(imgs)
    crops = np.stack([_pixels(plain[n]) for n in sorted(plain)])
    parser = _cropper(landmarks, background=0).par_model
    assert parser is not None
    labels = parser.parse(torch.from_numpy(crops).to("cuda:0"))[0].cpu().numpy()
    present = [np.unique(l) for l in labels]
    classes = sorted(set(np.concatenate(present).tolist()))
    foreground = None
    for n in (1, 2, 3):
        for cand in itertools.combinations(classes, n):
            hard = np.isin(labels, cand)
            if all(m.sum() > 10 and (~m).sum() > 10 for m in hard):
                foreground = list(cand)
                break
        if foreground is not None:
            break
    assert foreground is not None, f"the generated parser gives no class set that splits every crop: {present}"
    return {"dir": d, "landmarks": landmarks, "plain": plain, "crops": crops, "labels": labels, "foreground": foreground}


MODES = {"fill": {"background": FILL}, "blur": {"background_blur": SIGMA}}


def _expected(scene, mode, crops=None):
    bits = sum(1 << c for c in scene["foreground"])
    crops = scene["crops"] if crops is None else crops
    alpha = R.alpha_of(crops, scene["labels"], bits, RADIUS, EPSILON)
    for a in alpha:
        assert a.min() < a.max() and len(np.unique(a)) > 2          # subject, background and a soft edge in every crop
    if mode == "fill":
        return MR.composite(crops, alpha, FILL)
    return RB.over(crops, alpha, RB.background(crops, scene["labels"], bits, RB.blur_taps(SIGMA))[0])


@pytest.mark.parametrize("mode", sorted(MODES))
def test_process_dir_masks_and_one_parse(device, scene, tmp_path, monkeypatch, mode):
    """The composite is the reference's, the mask files are those of a run without refine byte for byte, and a batch is
    parsed once."""
    from face_crop_plus_amd import bise
    want = _expected(scene, mode)
    groups = {"fg": scene["foreground"], "all": list(range(19))}
    calls = []
    real = bise.BiSeNet.parse
    monkeypatch.setattr(bise.BiSeNet, "parse", lambda self, faces: (calls.append(int(faces.shape[0])), real(self, faces))[1])
    c = _cropper(scene["landmarks"], mask_groups=groups, foreground=scene["foreground"], **MODES[mode])
    assert c.feather == 5 and c.refine is None
    c.process_dir(str(scene["dir"]), str(tmp_path / "feather"), desc=None)
    assert sorted(calls) == [1, 2]                                   # three files in batches of two: one parse per batch
    del calls[:]
    c = _cropper(scene["landmarks"], mask_groups=groups, foreground=scene["foreground"], refine=RADIUS, **MODES[mode])
    assert (c.feather, c.refine, c.refine_eps) == (0, RADIUS, EPSILON)
    c.process_dir(str(scene["dir"]), str(tmp_path / "refine"), desc=None)
    assert sorted(calls) == [1, 2]
    before, got = _tree(tmp_path / "feather"), _tree(tmp_path / "refine")
    assert sorted(before) == sorted(got)
    masks = [n for n in before if "_mask" + os.sep in n]
    assert len(masks) == 6
    for n in masks:
        assert got[n] == before[n], n                                # byte-identical files
    names = sorted(scene["plain"])
    for n in set(before) - set(masks):
        k = names.index(os.path.basename(n))
        px = _pixels(got[n])
        assert np.array_equal(px, want[k]), n
        assert not np.array_equal(px, _pixels(before[n])) and not np.array_equal(px, scene["crops"][k])


@pytest.mark.parametrize("mode", sorted(MODES))
def test_device_encoder_writes_the_jpeg_of_the_composite(device, scene, tmp_path, mode):
    want = _expected(scene, mode)
    kw = dict(foreground=scene["foreground"], output_format="jpg", refine=RADIUS, refine_eps=EPSILON, **MODES[mode])
    c = _cropper(scene["landmarks"], encoder="device", **kw)
    c.process_dir(str(scene["dir"]), str(tmp_path / "dev"), desc=None)
    got = _tree(tmp_path / "dev")
    assert sorted(got) == ["a.jpg", "b.jpg", "c.jpg"]
    for data, ref in zip([got[n] for n in sorted(got)], c.encode_jpeg(want)):
        assert data == ref
    host = _cropper(scene["landmarks"], encoder="host", **kw)
    host.process_dir(str(scene["dir"]), str(tmp_path / "host"), desc=None)
    assert _tree(tmp_path / "host") == got


@pytest.mark.parametrize("mode", sorted(MODES))
def test_clahe_runs_before_the_refinement(device, scene, tmp_path, mode):
    c = _cropper(scene["landmarks"], clahe=2.0, foreground=scene["foreground"], refine=RADIUS, **MODES[mode])
    equalised = c.equalize(scene["crops"])
    assert not np.array_equal(equalised, scene["crops"])
    want = _expected(scene, mode, crops=equalised)            # the guide is the equalised crop, the labels the original's
    assert not np.array_equal(want, _expected(scene, mode))
    c.process_dir(str(scene["dir"]), str(tmp_path / "cl"), desc=None)
    got = _tree(tmp_path / "cl")
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), want[k]), n


def test_min_sharpness_scores_the_original_crop(device, scene, tmp_path):
    c = _cropper(scene["landmarks"])
    score = c.sharpness(scene["crops"])
    order = np.sort(score)
    assert order[0] < order[1]
    t = float(np.sqrt(max(order[0], 1e-9) * order[1])) if order[0] > 0 else float(order[1]) / 2
    kept_names = sorted(n for n, s in zip(sorted(scene["plain"]), score) if s >= t)
    assert 0 < len(kept_names) < 3
    c = _cropper(scene["landmarks"], min_sharpness=t, background=FILL, foreground=scene["foreground"], refine=RADIUS)
    c.process_dir(str(scene["dir"]), str(tmp_path / "ms"), desc=None)
    assert sorted(_tree(tmp_path / "ms")) == kept_names


def test_without_refine_nothing_new_runs(device, scene, tmp_path, monkeypatch):
    from face_crop_plus_amd import matte as M

    def never(*a, **k):
        raise AssertionError("refine_alpha without refine")
    monkeypatch.setattr(M, "refine_alpha", never)
    bits = sum(1 << c for c in scene["foreground"])
    want, _ = MR.matte(scene["crops"], scene["labels"], bits, 5, FILL)
    c = _cropper(scene["landmarks"], background=FILL, foreground=scene["foreground"])
    assert c.refine is None and c.feather == 5
    c.process_dir(str(scene["dir"]), str(tmp_path / "bg"), desc=None)
    got = _tree(tmp_path / "bg")
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), want[k]), n
    out, alpha = c.matte(scene["crops"], scene["labels"])
    assert np.array_equal(out, want)
    c = _cropper(scene["landmarks"], background=FILL, foreground=scene["foreground"], refine=RADIUS)
    with pytest.raises(AssertionError, match="without refine"):
        c.matte(scene["crops"], scene["labels"])
