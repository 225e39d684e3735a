"""Cropper(background_blur=...) on the GPU: the two blur launches against tests/matte_blur_ref.py byte for byte (sizes
below and around the 4 x 256 and 64 x 16 tiles, radii 3 and 48 and the tile width and one more, feathers, label patterns,
class sets), label bytes past the classes, guard bytes around offset views, repeated calls, in place, both boundaries,
Cropper.matte, and process_dir end to end on given landmarks."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu

ROW_W, ROW_H = 256, 4                        # kRowTileW, kRowTileH of csrc/fcp_masked_blur.h
TILE_W, TILE_H = 16, 64                      # kTileW, kTileH
SMALL = [(1, 1), (1, 2), (2, 1), (3, 3), (5, 4), (7, 7), (33, 65), (96, 80),
         (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1),
         (ROW_H - 1, ROW_W - 1), (ROW_H, ROW_W), (ROW_H + 1, ROW_W + 1)]
SIGMAS = (0.5, 5.33, 5.34, 16)               # r = 3, 16 (= kTileW), 17, 48
BIG, BIG_SIGMA = (256, 256), 4.0
ONE_17 = (1 << 1) | (1 << 17)


def _load():
    spec = importlib.util.spec_from_file_location("_matte_blur_ref", os.path.join(os.path.dirname(__file__), "matte_blur_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
MR = R.MR
_INPUTS, _BG = {}, {}


def _inputs(shape):
    """shape -> crops (3,h,w,3) and {pattern: labels (3,h,w)}, made once."""
    if shape not in _INPUTS:
        h, w = shape
        rng = np.random.default_rng(1000 * h + w)
        _INPUTS[shape] = (MR.random_crops(rng, 3, h, w), {p: R.labels_of(p, rng, 3, h, w) for p in R.PATTERNS})
    return _INPUTS[shape]


def _bg(shape, pattern, bits, sigma):
    """The reference background of a case, computed once and shared by every feather and test."""
    key = (shape, pattern, bits, sigma)
    if key not in _BG:
        crops, labels = _inputs(shape)
        _BG[key] = R.background(crops, labels[pattern], bits, R.blur_taps(sigma))[0]
    return _BG[key]


def _want(shape, pattern, bits, sigma, feather):
    crops, labels = _inputs(shape)
    return R.matte_blur(crops, labels[pattern], bits, feather, R.blur_taps(sigma), _bg(shape, pattern, bits, sigma))


def _combos(shape):
    if shape == BIG:
        return [("random", ONE_17)]
    if shape[0] * shape[1] > 3000:
        return [("random", ONE_17), ("one_bg", MR.DEFAULT_BITS)]        # the reference costs (2 r + 1)^2 passes over the crop
    return [(p, MR.DEFAULT_BITS) for p in R.PATTERNS] + [("random", ONE_17), ("checker", 1)]


def _call(crops, labels, bits, feather, taps, out, alpha):
    """The C entry point itself, on the pointers as given (views, in place, alpha NULL)."""
    import ctypes
    from face_crop_plus_amd import _native as N
    f, h, w, _ = crops.shape
    need = N.lib().fcp_matte_blur_workspace_bytes(f, h, w)
    assert need == 16 * f * h * w
    work = torch.empty((need,), dtype=torch.uint8, device=crops.device)
    t16 = (ctypes.c_uint16 * len(taps))(*taps)
    N.check(N.lib().fcp_matte_blur_u8(N.ptr(crops), N.ptr(labels), f, h, w, bits, feather, t16, len(taps) - 1, N.ptr(out),
                                      N.ptr(alpha), N.ptr(work), need, N.stream_ptr()), "fcp_matte_blur_u8")


@pytest.mark.parametrize("shape", SMALL + [BIG], ids=lambda s: f"{s[0]}x{s[1]}")
def test_out_and_alpha_equal_reference(device, shape):
    from face_crop_plus_amd import matte as M
    crops, labels = _inputs(shape)
    crops_dev = torch.from_numpy(crops).to(device)
    feathers = MR.FEATHERS if shape == (33, 65) else (0, 5)
    checked = 0
    for pattern, bits in _combos(shape):
        lab_dev = torch.from_numpy(labels[pattern]).to(device)
        for sigma in ((BIG_SIGMA,) if shape == BIG else SIGMAS):
            taps = M.blur_taps(sigma)
            assert taps == R.blur_taps(sigma)
            for feather in feathers:
                want, want_a = _want(shape, pattern, bits, sigma, feather)
                for f in (3, 1):
                    out, alpha = M.matte_blur(crops_dev[:f], lab_dev[:f], bits, feather, taps, with_alpha=True)
                    assert out.dtype == torch.uint8 and tuple(out.shape) == (f, *shape, 3) and tuple(alpha.shape) == (f, *shape)
                    what = (shape, pattern, hex(bits), sigma, feather, f)
                    assert np.array_equal(alpha.cpu().numpy(), want_a[:f]), what
                    got = out.cpu().numpy()
                    assert np.array_equal(got, want[:f]), (what, int((got != want[:f]).sum()))
                    checked += 1
    assert checked == len(_combos(shape)) * (1 if shape == BIG else len(SIGMAS)) * len(feathers) * 2


def test_the_cases_are_not_trivial():
    """From the reference alone: the blur changes the background, differs from a plain blur, and the radius matters."""
    shape = (33, 65)
    crops, labels = _inputs(shape)
    for sigma in SIGMAS:
        out, alpha = _want(shape, "random", ONE_17, sigma, 5)
        assert (out != crops).mean() > 0.5 and len(np.unique(alpha)) > 16
        assert not np.array_equal(_bg(shape, "random", ONE_17, sigma), R.plain_blur(crops, R.blur_taps(sigma)))
    assert not np.array_equal(_bg(shape, "random", ONE_17, 5.33), _bg(shape, "random", ONE_17, 5.34))
    out, alpha = _want(shape, "all_fg", MR.DEFAULT_BITS, 16, 5)
    assert np.array_equal(out, crops) and (alpha == 255).all()
    out, alpha = _want(shape, "one_bg", MR.DEFAULT_BITS, 16, 5)
    assert (alpha < 255).any() and not np.array_equal(out, crops)
    assert [len(R.blur_taps(s)) - 1 for s in SIGMAS] == [3, TILE_W, TILE_W + 1, 48]


def test_labels_past_the_classes_are_background(device):
    from face_crop_plus_amd import matte as M
    rng = np.random.default_rng(5)
    h, w = 37, 70
    labels = rng.choice(np.array([0, 1, 17, 18, 19, 31, 32, 33, 63, 64, 128, 255], np.uint8), (2, h, w))
    crops = MR.random_crops(rng, 2, h, w)
    taps = M.blur_taps(2.0)
    for bits in (MR.DEFAULT_BITS, ONE_17, 1, (1 << 19) - 1):
        hard = MR.mask(labels, bits)
        assert not hard[labels >= 19].any() and hard.any()
        bg = R.background(crops, labels, bits, taps)[0]
        for feather in MR.FEATHERS:
            want, want_a = R.matte_blur(crops, labels, bits, feather, taps, bg)
            out, alpha = M.matte_blur(torch.from_numpy(crops).to(device), torch.from_numpy(labels).to(device), bits, feather, taps, True)
            assert np.array_equal(alpha.cpu().numpy(), want_a) and np.array_equal(out.cpu().numpy(), want), (hex(bits), feather)


@pytest.mark.parametrize("shape", [(7, 7), (33, 65), (5, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bytes_offset_views_and_null_alpha(device, shape):
    crops, labels = _inputs(shape)
    lab = labels["random"]
    f, (h, w) = 3, shape
    G = 64
    for lead in (1, 2, 3):
        for sigma, feather in ((0.5, 0), (16, 5), (5.34, 7), (0.5, 3)):
            taps = R.blur_taps(sigma)
            want, want_a = _want(shape, "random", MR.DEFAULT_BITS, sigma, feather)
            # inputs: views that start `lead` bytes into a buffer and end exactly where it ends
            cbuf = torch.zeros(lead + crops.size, dtype=torch.uint8, device=device)
            lbuf = torch.zeros(lead + lab.size, dtype=torch.uint8, device=device)
            cbuf[lead:].copy_(torch.from_numpy(crops.reshape(-1)).to(device))
            lbuf[lead:].copy_(torch.from_numpy(lab.reshape(-1)).to(device))
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
                _call(cv, lv, MR.DEFAULT_BITS, feather, taps, ov, av if with_alpha else None)
                o, a = obuf.cpu().numpy(), abuf.cpu().numpy()
                what = (shape, lead, sigma, feather, with_alpha)
                assert (o[:G + lead] == 0xA5).all() and (o[G + lead + crops.size:] == 0xA5).all(), what
                assert np.array_equal(o[G + lead:G + lead + crops.size].reshape(crops.shape), want), what
                if with_alpha:
                    assert (a[:G + lead] == 0x5A).all() and (a[G + lead + f * h * w:] == 0x5A).all(), what
                    assert np.array_equal(a[G + lead:G + lead + f * h * w].reshape(f, h, w), want_a), what
                else:
                    assert (a == 0x5A).all(), what
            assert np.array_equal(cbuf[lead:].cpu().numpy(), crops.reshape(-1))            # the inputs are untouched
            assert np.array_equal(lbuf[lead:].cpu().numpy(), lab.reshape(-1))


@pytest.mark.parametrize("shape", [(33, 65), (96, 80), (5, 4), (65, 17)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_in_place_equals_out_of_place_and_calls_repeat(device, shape):
    crops, labels = _inputs(shape)
    lab = torch.from_numpy(labels["random"]).to(device)
    for sigma, feather in ((0.5, 0), (16, 5), (5.33, 7)):
        taps = R.blur_taps(sigma)
        want, want_a = _want(shape, "random", ONE_17, sigma, feather)
        src = torch.from_numpy(crops).to(device)
        outs = []
        for _ in range(2):
            out, alpha = torch.empty_like(src), torch.empty_like(lab)
            _call(src, lab, ONE_17, feather, taps, out, alpha)
            outs.append((out.cpu().numpy(), alpha.cpu().numpy()))
        assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        assert np.array_equal(outs[0][0], want) and np.array_equal(outs[0][1], want_a)
        _call(src, lab, ONE_17, feather, taps, src, None)                                  # out is crops
        assert np.array_equal(src.cpu().numpy(), want), (shape, sigma, feather)


def test_boundaries_give_identical_tensors(device, monkeypatch):
    from face_crop_plus_amd import matte as M
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    shape = (96, 80)
    crops, labels = _inputs(shape)
    cd, ld = torch.from_numpy(crops).to(device), torch.from_numpy(labels["random"]).to(device)
    for sigma, feather in ((0.5, 0), (16, 5), (5.34, 3), (5.33, 7)):
        taps = M.blur_taps(sigma)
        res = {}
        for enabled in (True, False):
            monkeypatch.setattr(T, "ENABLED", enabled)
            out, alpha = M.matte_blur(cd, ld, ONE_17, feather, taps, with_alpha=True)
            out2, none = M.matte_blur(cd, ld, ONE_17, feather, taps)
            assert none is None and torch.equal(out, out2)
            res[enabled] = (out, alpha)
        assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
        assert np.array_equal(res[True][0].cpu().numpy(), _want(shape, "random", ONE_17, sigma, feather)[0])
    taps = M.blur_taps(1.0)
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        with pytest.raises(RuntimeError, match="feather"):
            M.matte_blur(cd, ld, ONE_17, 4, taps)
        with pytest.raises(RuntimeError, match="class_bits"):
            M.matte_blur(cd, ld, 1 << 19, 5, taps)
        # the radius is the length of the taps less one: 2 and 49 are refused, and so is a list that lost a tap (its
        # length no longer goes with its radius, which shows in the sum)
        for bad in ([4094, 1, 1], [4096 - 2 * 49] + [1] * 49):
            with pytest.raises(RuntimeError, match="radius"):
                M.matte_blur(cd, ld, ONE_17, 5, bad)
        with pytest.raises(RuntimeError, match="sum to 4096"):
            M.matte_blur(cd, ld, ONE_17, 5, M.blur_taps(2.0)[:-1])
        empty, ea = M.matte_blur(cd[:0], ld[:0], ONE_17, 5, taps, with_alpha=True)
        assert tuple(empty.shape) == (0, 96, 80, 3) and tuple(ea.shape) == (0, 96, 80)
    ops = T.load()
    with pytest.raises(RuntimeError, match="labels"):
        ops.matte_blur(cd, ld[:, :-1].contiguous(), ONE_17, 5, taps, True)
    with pytest.raises(RuntimeError):
        ops.matte_blur(cd.float(), ld, ONE_17, 5, taps, True)
    # the C entry points themselves at 8 x 8: one tap of 0 in a window that still sums to 4096, and a window that sums to
    # 4095, are refused under the entry point's name before anything is launched
    import ctypes
    from face_crop_plus_amd import _native as N
    lib = N.lib()
    c8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=device)
    l8 = torch.zeros((1, 8, 8), dtype=torch.uint8, device=device)
    a8 = torch.full((1, 8, 8), 128, dtype=torch.uint8, device=device)
    o8 = torch.full((1, 8, 8, 3), 7, dtype=torch.uint8, device=device)
    need = lib.fcp_matte_blur_workspace_bytes(1, 8, 8)
    work = torch.empty((need,), dtype=torch.uint8, device=device)
    for bad, word in (([4090, 2, 0, 1], b"tap 2 is 0"), ([4089, 1, 1, 1], b"sum to 4096")):
        t16 = (ctypes.c_uint16 * 4)(*bad)
        assert lib.fcp_matte_blur_u8(N.ptr(c8), N.ptr(l8), 1, 8, 8, ONE_17, 5, t16, 3, N.ptr(o8), None, N.ptr(work), need,
                                     N.stream_ptr()) < 0, bad
        assert lib.fcp_last_error().startswith(b"matte_blur:") and word in lib.fcp_last_error(), (bad, lib.fcp_last_error())
        assert lib.fcp_matte_blur_alpha_u8(N.ptr(c8), N.ptr(l8), N.ptr(a8), 1, 8, 8, ONE_17, t16, 3, N.ptr(o8), N.ptr(work), need,
                                           N.stream_ptr()) < 0, bad
        assert lib.fcp_last_error().startswith(b"matte_blur_alpha:") and word in lib.fcp_last_error(), (bad, lib.fcp_last_error())
    torch.cuda.synchronize()
    assert (o8.cpu() == 7).all()                                     # nothing was launched


def test_cropper_matte_equals_reference(device):
    from face_crop_plus_amd import Cropper
    shape = (33, 65)
    crops, labels = _inputs(shape)
    c = Cropper(output_size=48, landmarks=(np.zeros((1, 5, 2), np.float32), np.array(["a"])), det_threshold=None, device="cuda:0",
                background_blur=5.34, foreground=[1, 17], feather=7, weights={"bisenet": "generated"})
    assert c.par_model is not None and c.par_model.attr_groups is None and c.par_model.mask_groups is None
    assert c.background is None and c.blur_taps == R.blur_taps(5.34)
    out, alpha = c.matte(crops, labels["random"])
    want, want_a = _want(shape, "random", ONE_17, 5.34, 7)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and alpha.dtype == np.uint8
    assert np.array_equal(alpha, want_a) and np.array_equal(out, want)
    out0, alpha0 = c.matte(crops[:0], labels["random"][:0])
    assert out0.shape == (0, 33, 65, 3) and alpha0.shape == (0, 33, 65)


# ---- end to end: process_dir on given landmarks
SIGMA = 3.0
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
    foreground class set under which every crop has subject and background pixels: the faces of the BiSeNet golden
    fixture, cropped at the target points themselves, which the generated parser splits into two large classes."""
    import itertools
    from PIL import Image
    d = tmp_path_factory.mktemp("blur_in")
    faces = np.load(os.path.join(os.path.dirname(__file__), "golden", "bisenet.npz"))["faces"]
    assert faces.shape == (3, *SIZE, 3)
    imgs = {f"{n}.png": face for n, face in zip("abc", faces)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name, compress_level=1)
    tgt = A.landmarks_target(SIZE, 0.65)
    landmarks = (np.stack([tgt, tgt, tgt]).astype(np.float32), np.array(sorted(imgs)))
    out = tmp_path_factory.mktemp("blur_plain")
    c = _cropper(landmarks)
    assert c.par_model is None
    c.process_dir(str(d), str(out), desc=None)
    plain = _tree(out)
    assert sorted(plain) == sorted(imgs)
    crops = np.stack([_pixels(plain[n]) for n in sorted(plain)])
    parser = _cropper(landmarks, background_blur=SIGMA).par_model
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


def _expected(scene, crops=None, feather=5):
    bits = sum(1 << c for c in scene["foreground"])
    crops = scene["crops"] if crops is None else crops
    want, alpha = R.matte_blur(crops, scene["labels"], bits, feather, R.blur_taps(SIGMA))
    for a in alpha:
        assert a.min() < a.max()                              # subject and background in every crop
    return want


def test_process_dir_writes_the_composite(device, scene, tmp_path):
    want = _expected(scene)
    c = _cropper(scene["landmarks"], background_blur=SIGMA, foreground=scene["foreground"])
    assert c.feather == 5 and c.background is None
    c.process_dir(str(scene["dir"]), str(tmp_path / "bb"), desc=None)
    got = _tree(tmp_path / "bb")
    assert sorted(got) == sorted(scene["plain"])
    for k, n in enumerate(sorted(got)):
        px = _pixels(got[n])
        assert np.array_equal(px, want[k]), n
        assert not np.array_equal(px, scene["crops"][k]) and len(np.unique(px.reshape(-1, 3), axis=0)) > 16   # no uniform fill


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
    c = _cropper(scene["landmarks"], mask_groups=groups, background_blur=SIGMA, foreground=scene["foreground"])
    c.process_dir(str(scene["dir"]), str(tmp_path / "bb"), desc=None)
    assert sorted(calls) == [1, 2]
    plain, got = _tree(tmp_path / "plain"), _tree(tmp_path / "bb")
    assert sorted(plain) == sorted(got)
    masks = [n for n in plain if "_mask" + os.sep in n]
    assert len(masks) == 6
    for n in masks:
        assert got[n] == plain[n], n                                 # byte-identical files
    names = sorted(scene["plain"])
    for n in set(plain) - set(masks):
        k = names.index(os.path.basename(n))
        assert np.array_equal(_pixels(plain[n]), scene["crops"][k]) and np.array_equal(_pixels(got[n]), want[k]), n


def test_device_encoder_writes_the_jpeg_of_the_composite(device, scene, tmp_path):
    want = _expected(scene)
    kw = dict(background_blur=SIGMA, foreground=scene["foreground"], output_format="jpg")
    c = _cropper(scene["landmarks"], encoder="device", **kw)
    c.process_dir(str(scene["dir"]), str(tmp_path / "dev"), desc=None)
    got = _tree(tmp_path / "dev")
    assert sorted(got) == ["a.jpg", "b.jpg", "c.jpg"]
    for data, ref in zip([got[n] for n in sorted(got)], c.encode_jpeg(want)):
        assert data == ref
    host = _cropper(scene["landmarks"], encoder="host", **kw)
    host.process_dir(str(scene["dir"]), str(tmp_path / "host"), desc=None)
    assert _tree(tmp_path / "host") == got


def test_min_sharpness_scores_the_unblurred_crop(device, scene, tmp_path):
    c = _cropper(scene["landmarks"])
    score = c.sharpness(scene["crops"])
    order = np.sort(score)
    assert order[0] < order[1]
    t = float(np.sqrt(max(order[0], 1e-9) * order[1])) if order[0] > 0 else float(order[1]) / 2
    kept_names = sorted(n for n, s in zip(sorted(scene["plain"]), score) if s >= t)
    assert 0 < len(kept_names) < 3
    assert not np.array_equal(c.sharpness(_expected(scene)), score)      # the filter must not see the blurred crops
    res = {}
    for key, kw in (("plain", {}), ("bb", dict(background_blur=SIGMA, foreground=scene["foreground"]))):
        c = _cropper(scene["landmarks"], min_sharpness=t, **kw)
        c.process_dir(str(scene["dir"]), str(tmp_path / key), desc=None)
        res[key] = sorted(_tree(tmp_path / key))
    assert res["plain"] == res["bb"] == kept_names


def test_clahe_runs_before_the_blur(device, scene, tmp_path):
    c = _cropper(scene["landmarks"], clahe=2.0, background_blur=SIGMA, foreground=scene["foreground"])
    equalised = c.equalize(scene["crops"])
    assert not np.array_equal(equalised, scene["crops"])
    want = _expected(scene, crops=equalised)                  # the labels are those of the original crop
    c.process_dir(str(scene["dir"]), str(tmp_path / "cl"), desc=None)
    got = _tree(tmp_path / "cl")
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), want[k]), n
