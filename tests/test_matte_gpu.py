"""Cropper(background=...) on the GPU: the matte kernel's alpha and composite against tests/matte_ref.py byte for byte
(sizes below and around the 64 x 32 tile, every feather, label patterns, class sets, fills), label bytes past the classes,
guard bytes around offset views, in place, both boundaries, Cropper.matte, and process_dir end to end on given landmarks."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 32                      # kTileW, kTileH of csrc/fcp_matte.hip
SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (2, 7), (3, 3), (5, 4), (7, 7), (8, 9), (33, 65), (64, 64), (65, 127), (96, 80),
         (256, 256), (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1)]
SIZES = list(dict.fromkeys(SIZES))           # (33, 65) is tile + 1 already
PATTERNS = ("random", "checker", "corners")
ONE_17 = (1 << 1) | (1 << 17)
FILLS = ((0, 0, 0), (255, 255, 255), (12, 200, 99))


def _load():
    spec = importlib.util.spec_from_file_location("_matte_ref", os.path.join(os.path.dirname(__file__), "matte_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
BITS = (R.DEFAULT_BITS, ONE_17)
_CASES = {}


def _case(shape):
    """shape -> crops (3,h,w,3), {pattern: labels (3,h,w)}, {(pattern, bits, feather): reference alpha}, computed once."""
    if shape not in _CASES:
        h, w = shape
        rng = np.random.default_rng(1000 * h + w)
        labels = {"random": R.random_labels(rng, 3, h, w), "checker": R.checker_labels(3, h, w), "corners": R.corner_labels(3, h, w)}
        alphas = {(p, b, fe): np.stack([R.alpha_separable(R.mask(l, b), fe) for l in labels[p]])
                  for p in PATTERNS for b in BITS for fe in R.FEATHERS}
        _CASES[shape] = (R.random_crops(rng, 3, h, w), labels, alphas)
    return _CASES[shape]


def _call(crops, labels, bits, feather, fill, out, alpha):
    """The C entry point itself, on the pointers as given (views, in place, alpha NULL)."""
    from face_crop_plus_amd import _native as N
    f, h, w, _ = crops.shape
    N.check(N.lib().fcp_matte_u8(N.ptr(crops), N.ptr(labels), f, h, w, bits, feather, *fill, N.ptr(out), N.ptr(alpha),
                                 N.stream_ptr()), "fcp_matte_u8")


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_alpha_and_out_equal_reference(device, shape):
    from face_crop_plus_amd import matte as M
    crops, labels, alphas = _case(shape)
    crops_dev = torch.from_numpy(crops).to(device)
    checked = 0
    for p in PATTERNS:
        lab_dev = torch.from_numpy(labels[p]).to(device)
        for bits in BITS:
            for feather in R.FEATHERS:
                want_a = alphas[(p, bits, feather)]
                for fill in FILLS:
                    want = R.composite(crops, want_a, fill)
                    for f in (3, 1):
                        out, alpha = M.matte(crops_dev[:f], lab_dev[:f], bits, feather, fill, with_alpha=True)
                        assert out.dtype == torch.uint8 and tuple(out.shape) == (f, *shape, 3) and tuple(alpha.shape) == (f, *shape)
                        what = (shape, p, hex(bits), feather, fill, f)
                        assert np.array_equal(alpha.cpu().numpy(), want_a[:f]), what
                        assert np.array_equal(out.cpu().numpy(), want[:f]), what
                        checked += 1
    assert checked == len(PATTERNS) * len(BITS) * len(R.FEATHERS) * len(FILLS) * 2


def test_the_cases_are_not_trivial():
    """From the reference alone: the patterns give soft edges, both ends of alpha and differing class sets."""
    _, labels, alphas = _case((33, 65))
    hi, lo = alphas[("random", R.DEFAULT_BITS, 5)], alphas[("random", ONE_17, 5)]
    # 18 of 19 random classes are foreground under the default set, 2 of 19 under {1, 17}: both ends of the alpha range
    assert hi.mean() > 192 and lo.mean() < 64 and len(np.unique(hi)) > 16 and len(np.unique(lo)) > 16
    assert not np.array_equal(alphas[("random", R.DEFAULT_BITS, 5)], alphas[("random", ONE_17, 5)])
    assert not np.array_equal(alphas[("random", ONE_17, 3)], alphas[("random", ONE_17, 7)])
    c = alphas[("corners", R.DEFAULT_BITS, 7)][0]
    assert c[0, 0] > 0 and c[-1, -1] > 0 and c[16, 32] == 0
    assert set(np.unique(alphas[("checker", R.DEFAULT_BITS, 0)])) == {0, 255}


def test_labels_past_the_classes_are_background(device):
    from face_crop_plus_amd import matte as M
    rng = np.random.default_rng(5)
    h, w = 37, 70
    labels = rng.choice(np.array([0, 1, 17, 18, 19, 31, 32, 33, 63, 64, 128, 255], np.uint8), (2, h, w))
    crops = R.random_crops(rng, 2, h, w)
    for bits in (R.DEFAULT_BITS, ONE_17, 1, (1 << 19) - 1):
        hard = R.mask(labels, bits)
        assert not hard[labels >= 19].any() and hard.any()
        for feather in R.FEATHERS:
            want, want_a = R.matte(crops, labels, bits, feather, FILLS[2])
            out, alpha = M.matte(torch.from_numpy(crops).to(device), torch.from_numpy(labels).to(device), bits, feather, FILLS[2], True)
            assert np.array_equal(alpha.cpu().numpy(), want_a) and np.array_equal(out.cpu().numpy(), want), (hex(bits), feather)


@pytest.mark.parametrize("shape", [(7, 7), (33, 65), (5, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bytes_offset_views_and_null_alpha(device, shape):
    crops, labels, alphas = _case(shape)
    f, (h, w) = 3, shape
    G = 64
    for lead in (1, 2, 3):
        for feather in R.FEATHERS:
            want_a = alphas[("random", R.DEFAULT_BITS, feather)]
            want = R.composite(crops, want_a, FILLS[2])
            # inputs: views that start `lead` bytes into a buffer and end exactly where it ends
            cbuf = torch.zeros(lead + crops.size, dtype=torch.uint8, device=device)
            lbuf = torch.zeros(lead + labels["random"].size, dtype=torch.uint8, device=device)
            cbuf[lead:].copy_(torch.from_numpy(crops.reshape(-1)).to(device))
            lbuf[lead:].copy_(torch.from_numpy(labels["random"].reshape(-1)).to(device))
            cv, lv = cbuf[lead:].view(crops.shape), lbuf[lead:].view(f, h, w)
            assert cv.data_ptr() % 4 == lead and lv.data_ptr() % 4 == lead
            # outputs: between 64 guard bytes, at the same odd offsets
            obuf = torch.full((G + lead + crops.size + G,), 0xA5, dtype=torch.uint8, device=device)
            abuf = torch.full((G + lead + f * h * w + G,), 0x5A, dtype=torch.uint8, device=device)
            ov = obuf[G + lead:G + lead + crops.size].view(crops.shape)
            av = abuf[G + lead:G + lead + f * h * w].view(f, h, w)
            for with_alpha in (True, False):
                obuf.fill_(0xA5)
                abuf.fill_(0x5A)
                _call(cv, lv, R.DEFAULT_BITS, feather, FILLS[2], ov, av if with_alpha else None)
                o, a = obuf.cpu().numpy(), abuf.cpu().numpy()
                what = (shape, lead, feather, with_alpha)
                assert (o[:G + lead] == 0xA5).all() and (o[G + lead + crops.size:] == 0xA5).all(), what
                assert np.array_equal(o[G + lead:G + lead + crops.size].reshape(crops.shape), want), what
                if with_alpha:
                    assert (a[:G + lead] == 0x5A).all() and (a[G + lead + f * h * w:] == 0x5A).all(), what
                    assert np.array_equal(a[G + lead:G + lead + f * h * w].reshape(f, h, w), want_a), what
                else:
                    assert (a == 0x5A).all(), what
            assert np.array_equal(cbuf[lead:].cpu().numpy(), crops.reshape(-1))            # the inputs are untouched


@pytest.mark.parametrize("shape", [(33, 65), (96, 80), (5, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_in_place_equals_out_of_place_and_calls_repeat(device, shape):
    crops, labels, alphas = _case(shape)
    lab = torch.from_numpy(labels["checker"]).to(device)
    for feather in R.FEATHERS:
        want = R.composite(crops, alphas[("checker", R.DEFAULT_BITS, feather)], FILLS[2])
        src = torch.from_numpy(crops).to(device)
        outs = []
        for _ in range(2):
            out, alpha = torch.empty_like(src), torch.empty_like(lab)
            _call(src, lab, R.DEFAULT_BITS, feather, FILLS[2], out, alpha)
            outs.append((out.cpu().numpy(), alpha.cpu().numpy()))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        assert np.array_equal(outs[0][0], want)
        _call(src, lab, R.DEFAULT_BITS, feather, FILLS[2], src, None)                  # out is crops
        assert np.array_equal(src.cpu().numpy(), want), (shape, feather)


def test_boundaries_give_identical_tensors(device, monkeypatch):
    from face_crop_plus_amd import matte as M
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    for shape in ((33, 65), (96, 80)):
        crops, labels, alphas = _case(shape)
        cd, ld = torch.from_numpy(crops).to(device), torch.from_numpy(labels["random"]).to(device)
        for feather in R.FEATHERS:
            res = {}
            for enabled in (True, False):
                monkeypatch.setattr(T, "ENABLED", enabled)
                out, alpha = M.matte(cd, ld, ONE_17, feather, FILLS[2], with_alpha=True)
                out2, none = M.matte(cd, ld, ONE_17, feather, FILLS[2])
                assert none is None and torch.equal(out, out2)
                res[enabled] = (out, alpha)
            assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
            assert np.array_equal(res[True][1].cpu().numpy(), alphas[("random", ONE_17, feather)])
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        with pytest.raises(RuntimeError, match="feather"):
            M.matte(cd, ld, ONE_17, 4, FILLS[2])
        with pytest.raises(RuntimeError, match="class_bits"):
            M.matte(cd, ld, 1 << 19, 5, FILLS[2])
        empty, ea = M.matte(cd[:0], ld[:0], ONE_17, 5, FILLS[2], with_alpha=True)
        assert tuple(empty.shape) == (0, 96, 80, 3) and tuple(ea.shape) == (0, 96, 80)
    ops = T.load()
    with pytest.raises(RuntimeError, match="labels"):
        ops.matte(cd, ld[:, :-1].contiguous(), ONE_17, 5, 0, 0, 0, True)
    with pytest.raises(RuntimeError):
        ops.matte(cd.float(), ld, ONE_17, 5, 0, 0, 0, True)


def test_cropper_matte_equals_reference(device):
    from face_crop_plus_amd import Cropper
    crops, labels, alphas = _case((65, 127))
    c = Cropper(output_size=48, landmarks=(np.zeros((1, 5, 2), np.float32), np.array(["a"])), det_threshold=None, device="cuda:0",
                background=(12, 200, 99), foreground=[1, 17], feather=7, weights={"bisenet": "generated"})
    assert c.par_model is not None and c.par_model.attr_groups is None and c.par_model.mask_groups is None
    out, alpha = c.matte(crops, labels["random"])
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and alpha.dtype == np.uint8
    assert np.array_equal(alpha, alphas[("random", ONE_17, 7)])
    assert np.array_equal(out, R.composite(crops, alpha, (12, 200, 99)))
    out0, alpha0 = c.matte(crops[:0], labels["random"][:0])
    assert out0.shape == (0, 65, 127, 3) and alpha0.shape == (0, 65, 127)
    for bad in ((crops.astype(np.float32), labels["random"]), (crops, labels["random"].astype(np.int32)),
                (crops, labels["random"][:, :-1]), (crops[..., 0], labels["random"])):
        with pytest.raises(ValueError):
            c.matte(*bad)
    plain = Cropper(output_size=48, landmarks=(np.zeros((1, 5, 2), np.float32), np.array(["a"])), det_threshold=None, device="cuda:0")
    assert plain.par_model is None
    with pytest.raises(ValueError, match="background"):
        plain.matte(crops, labels["random"])


# ---- end to end: process_dir on given landmarks
FILL = (0, 177, 64)
SIZE = (64, 64)


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
    """Three files with a landmark set each, their plain crops, the label maps the Cropper's own parser gives them, and a
    foreground class set under which every crop has subject and background pixels.  The files are the faces of the BiSeNet
    golden fixture and the landmarks are the target points themselves, so the crops are (about) those faces, which the
    generated parser is known to split into two large classes: the composite is never the crop or the fill alone."""
    from PIL import Image
    d = tmp_path_factory.mktemp("matte_in")
    faces = np.load(os.path.join(os.path.dirname(__file__), "golden", "bisenet.npz"))["faces"]
    assert faces.shape == (3, *SIZE, 3)
    imgs = {f"{n}.png": face for n, face in zip("abc", faces)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name, compress_level=1)
    tgt = A.landmarks_target(SIZE, 0.65)
    landmarks = (np.stack([tgt, tgt, tgt]).astype(np.float32), np.array(sorted(imgs)))
    out = tmp_path_factory.mktemp("matte_plain")
    c = _cropper(landmarks)
    assert c.par_model is None
    c.process_dir(str(d), str(out), desc=None)
    plain = _tree(out)
    assert sorted(plain) == sorted(imgs)
    crops = np.stack([_pixels(plain[n]) for n in sorted(plain)])
    parser = _cropper(landmarks, background=FILL).par_model
    labels = parser.parse(torch.from_numpy(crops).to("cuda:0"))[0].cpu().numpy()
    present = [np.unique(l) for l in labels]
    print("classes per crop:", [p.tolist() for p in present])
    import itertools
    classes = sorted(set(np.concatenate(present).tolist()))
    foreground = None
    for n in (1, 2, 3):
        for cand in itertools.combinations(classes, n):
            hard = np.isin(labels, cand)
            if all(m.sum() > 10 and (~m).sum() > 10 for m in hard):      # more than BiSeNet.mask_threshold pixels each way
                foreground = list(cand)
                break
        if foreground is not None:
            break
    # not vacuous: without such a set the composite would be the crop or the fill everywhere
    assert foreground is not None, f"the generated parser gives no class set that splits every crop: {present}"
    return {"dir": d, "landmarks": landmarks, "plain": plain, "crops": crops, "labels": labels, "foreground": foreground}


def _expected(scene, feather=5):
    bits = sum(1 << c for c in scene["foreground"])
    want, alpha = R.matte(scene["crops"], scene["labels"], bits, feather, FILL)
    for a, l in zip(alpha, scene["labels"]):
        hard = np.isin(l, scene["foreground"])
        assert hard.any() and not hard.all() and a.min() < a.max()  # subject and background in every crop
    return want


def test_process_dir_writes_the_composite(device, scene, tmp_path):
    want = _expected(scene)
    c = _cropper(scene["landmarks"], background=FILL, foreground=scene["foreground"])
    assert c.feather == 5
    c.process_dir(str(scene["dir"]), str(tmp_path / "bg"), desc=None)
    got = _tree(tmp_path / "bg")
    assert sorted(got) == sorted(scene["plain"])
    for k, n in enumerate(sorted(got)):
        px = _pixels(got[n])
        assert np.array_equal(px, want[k]), n
        assert not np.array_equal(px, scene["crops"][k]) and not (px == np.array(FILL, np.uint8)).all()
    # feather 0 and a gray fill: the hard mask
    c = _cropper(scene["landmarks"], background=200, foreground=scene["foreground"], feather=0)
    c.process_dir(str(scene["dir"]), str(tmp_path / "hard"), desc=None)
    hard = np.isin(scene["labels"], scene["foreground"])[..., None]
    for k, (n, data) in enumerate(sorted(_tree(tmp_path / "hard").items())):
        assert np.array_equal(_pixels(data), np.where(hard[k], scene["crops"][k], np.uint8(200))), n


def test_masks_are_unchanged_and_the_batch_is_parsed_once(device, scene, tmp_path, monkeypatch):
    from face_crop_plus_amd import bise
    want = _expected(scene)
    groups = {"fg": scene["foreground"], "all": list(range(19))}
    calls = []
    real = bise.BiSeNet.parse
    monkeypatch.setattr(bise.BiSeNet, "parse", lambda self, faces: (calls.append(int(faces.shape[0])), real(self, faces))[1])
    c = _cropper(scene["landmarks"], mask_groups=groups)
    c.process_dir(str(scene["dir"]), str(tmp_path / "plain"), desc=None)
    assert sorted(calls) == [1, 2]                                   # three files in batches of two: one parse per batch
    del calls[:]
    c = _cropper(scene["landmarks"], mask_groups=groups, background=FILL, foreground=scene["foreground"])
    c.process_dir(str(scene["dir"]), str(tmp_path / "bg"), desc=None)
    assert sorted(calls) == [1, 2]
    plain, got = _tree(tmp_path / "plain"), _tree(tmp_path / "bg")
    assert sorted(plain) == sorted(got)
    masks = [n for n in plain if "_mask" + os.sep in n]
    assert len(masks) == 6
    for n in masks:
        assert got[n] == plain[n], n                                 # byte-identical files, hard 0 / 255
        assert set(np.unique(_pixels(plain[n]))) <= {0, 255}
    names = sorted(scene["plain"])
    for n in set(plain) - set(masks):
        k = names.index(os.path.basename(n))
        assert np.array_equal(_pixels(plain[n]), scene["crops"][k]) and np.array_equal(_pixels(got[n]), want[k]), n


def test_device_encoder_writes_the_jpeg_of_the_composite(device, scene, tmp_path):
    want = _expected(scene)
    c = _cropper(scene["landmarks"], background=FILL, foreground=scene["foreground"], encoder="device", output_format="jpg")
    c.process_dir(str(scene["dir"]), str(tmp_path / "dev"), desc=None)
    got = _tree(tmp_path / "dev")
    assert sorted(got) == ["a.jpg", "b.jpg", "c.jpg"]
    for data, ref in zip([got[n] for n in sorted(got)], c.encode_jpeg(want)):
        assert data == ref
    host = _cropper(scene["landmarks"], background=FILL, foreground=scene["foreground"], encoder="host", output_format="jpg")
    host.process_dir(str(scene["dir"]), str(tmp_path / "host"), desc=None)
    assert _tree(tmp_path / "host") == got


def test_min_sharpness_scores_the_unmatted_crop(device, scene, tmp_path):
    c = _cropper(scene["landmarks"])
    score = c.sharpness(scene["crops"])
    order = np.sort(score)
    assert order[0] < order[1]
    t = float(np.sqrt(max(order[0], 1e-9) * order[1])) if order[0] > 0 else float(order[1]) / 2
    kept_names = sorted(n for n, s in zip(sorted(scene["plain"]), score) if s >= t)
    assert 0 < len(kept_names) < 3
    # the matted crops would score differently: the filter must not see them
    matted = c.sharpness(_expected(scene))
    assert not np.array_equal(matted >= t, score >= t) or not np.array_equal(matted, score)
    res = {}
    for key, kw in (("plain", {}), ("bg", dict(background=FILL, foreground=scene["foreground"]))):
        c = _cropper(scene["landmarks"], min_sharpness=t, **kw)
        c.process_dir(str(scene["dir"]), str(tmp_path / key), desc=None)
        res[key] = sorted(_tree(tmp_path / key))
    assert res["plain"] == res["bg"] == kept_names
