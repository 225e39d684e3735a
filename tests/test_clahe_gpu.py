"""Cropper(clahe=...) on the GPU: the two CLAHE kernels against tests/clahe_ref.py byte for byte, through ctypes and
through the torch op, on the inputs of clahe_ref.gpu_cases (tests/test_clahe_cpu.py shows which branches they reach), the
LUT workspace itself, offset views with guard bytes, in place, F = 0, Cropper.equalize, and process_dir end to end."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu


def _load():
    spec = importlib.util.spec_from_file_location("_clahe_ref", os.path.join(os.path.dirname(__file__), "clahe_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
CASES = R.gpu_cases()
_WANT = {}


def _want(name):
    """name -> (reference RGB (F,h,w,3), reference LUTs (F,g,g,256)), computed once."""
    if name not in _WANT:
        crops, g, c = CASES[name]
        full = [R.clahe_full(crop, c, g) for crop in crops]
        _WANT[name] = (np.stack([d["rgb"] for d in full]), np.stack([d["luts"] for d in full]))
    return _WANT[name]


def _call(crops, grid, clip, luts, out):
    """The C entry point itself, on the pointers as given (views, in place)."""
    from face_crop_plus_amd import _native as N
    f, h, w, _ = crops.shape
    N.check(N.lib().fcp_clahe_u8(N.ptr(crops), f, h, w, grid, clip, N.ptr(luts), N.ptr(out), N.stream_ptr()), "fcp_clahe_u8")


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_equal_reference(device, name):
    from face_crop_plus_amd import torch_ops as T
    crops, g, c = CASES[name]
    want, want_luts = _want(name)
    src = torch.from_numpy(crops).to(device)
    luts = torch.full((len(crops), g, g, 256), 0x5A, dtype=torch.uint8, device=device)
    out = torch.empty_like(src)
    _call(src, g, c, luts, out)                                                    # ctypes
    assert np.array_equal(luts.cpu().numpy(), want_luts), name
    assert np.array_equal(out.cpu().numpy(), want), name
    assert np.array_equal(src.cpu().numpy(), crops)                                # the input is untouched
    got = T.load().clahe(src, g, c)                                                # the torch op
    assert got.dtype == torch.uint8 and tuple(got.shape) == crops.shape
    assert np.array_equal(got.cpu().numpy(), want), name
    again = torch.empty_like(src)                                                  # the same bytes from run to run
    _call(src, g, c, luts, again)
    assert torch.equal(again, out)
    _call(src, g, c, luts, src)                                                    # out is crops
    assert np.array_equal(src.cpu().numpy(), want), name


def test_offset_view_with_guard_bytes(device):
    """The 48 x 37 case on the view crops[1:]: 37 * 3 = 111 bytes a row, the view starts 48 * 111 = 5328 + lead bytes in,
    at every residue of the base address; out sits between guard bytes at the same residues."""
    crops, g, c = CASES["48x37_g8_view"]
    want, want_luts = _want("48x37_g8_view")
    G = 64
    n = crops[1:].size
    for lead in (0, 1, 2, 3):
        buf = torch.zeros(lead + crops.size, dtype=torch.uint8, device=device)
        buf[lead:].copy_(torch.from_numpy(crops.reshape(-1)).to(device))
        view = buf[lead:].view(crops.shape)[1:]
        assert view.data_ptr() % 4 == (lead + 48 * 37 * 3) % 4 and view.is_contiguous()
        obuf = torch.full((G + lead + n + G,), 0xA5, dtype=torch.uint8, device=device)
        ov = obuf[G + lead:G + lead + n].view(view.shape)
        luts = torch.empty((2, g, g, 256), dtype=torch.uint8, device=device)
        _call(view, g, c, luts, ov)
        o = obuf.cpu().numpy()
        assert (o[:G + lead] == 0xA5).all() and (o[G + lead + n:] == 0xA5).all(), lead
        assert np.array_equal(o[G + lead:G + lead + n].reshape(view.shape), want[1:]), lead
        assert np.array_equal(luts.cpu().numpy(), want_luts[1:]), lead
        assert np.array_equal(buf[lead:].cpu().numpy(), crops.reshape(-1))          # the inputs are untouched
        _call(view, g, c, luts, view)                                                # in place, on the view
        assert np.array_equal(buf[lead:].cpu().numpy().reshape(crops.shape)[1:], want[1:]), lead
        assert np.array_equal(buf[lead:].cpu().numpy().reshape(crops.shape)[0], crops[0]), lead


def test_boundaries_give_identical_tensors(device, monkeypatch):
    from face_crop_plus_amd import clahe as C
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    for name in ("64x64_g8_c2", "50x37_g8_c40", "primaries_g4"):
        crops, g, c = CASES[name]
        src = torch.from_numpy(crops).to(device)
        res = {}
        for enabled in (True, False):
            monkeypatch.setattr(T, "ENABLED", enabled)
            res[enabled] = C.clahe(src, c, g)
        assert torch.equal(res[True], res[False])
        assert np.array_equal(res[True].cpu().numpy(), _want(name)[0])
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        with pytest.raises(RuntimeError, match="grid"):
            C.clahe(src, 2.0, 17)
        with pytest.raises(RuntimeError, match="clip_limit"):
            C.clahe(src, 0.0, 4)
        with pytest.raises(RuntimeError, match="2 \\* grid"):
            C.clahe(src[:, :20].contiguous(), 2.0, 16)
        empty = C.clahe(src[:0], 2.0, 4)                                             # F = 0
        assert tuple(empty.shape) == (0, 40, 48, 3) and empty.dtype == torch.uint8
    with pytest.raises(RuntimeError):
        T.load().clahe(src.float(), 4, 2.0)
    with pytest.raises(RuntimeError):
        T.load().clahe(src[..., 0], 4, 2.0)


def test_cropper_equalize_equals_reference(device):
    from face_crop_plus_amd import Cropper
    given = dict(landmarks=(np.zeros((1, 5, 2), np.float32), np.array(["a"])), det_threshold=None, device="cuda:0")
    crops, g, c = CASES["50x37_g8_c40"]
    cr = Cropper(output_size=48, clahe=c, **given)
    assert cr.clahe_grid == 8 and cr.par_model is None
    out = cr.equalize(crops)
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8
    assert np.array_equal(out, _want("50x37_g8_c40")[0])
    assert cr.equalize(crops[:0]).shape == (0, 50, 37, 3)
    crops4, g4, c4 = CASES["primaries_g4"]
    assert np.array_equal(Cropper(output_size=48, clahe=c4, clahe_grid=g4, **given).equalize(crops4), _want("primaries_g4")[0])
    for bad in (crops.astype(np.float32), crops[..., 0], crops[..., :2]):
        with pytest.raises(ValueError):
            cr.equalize(bad)
    with pytest.raises(ValueError, match="clahe"):
        Cropper(output_size=48, **given).equalize(crops)


# ---- end to end: process_dir on given landmarks
FILL = (0, 177, 64)
SIZE = (64, 64)
CLIP = 2.0


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
    """Three files with a landmark set each (the faces of the BiSeNet golden fixture, the landmarks the target points), the
    crops a Cropper without ``clahe`` writes for them, and the reference applied to those crops."""
    from PIL import Image
    d = tmp_path_factory.mktemp("clahe_in")
    faces = np.load(os.path.join(os.path.dirname(__file__), "golden", "bisenet.npz"))["faces"]
    assert faces.shape == (3, *SIZE, 3)
    imgs = {f"{n}.png": face for n, face in zip("abc", faces)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name, compress_level=1)
    tgt = A.landmarks_target(SIZE, 0.65)
    landmarks = (np.stack([tgt, tgt, tgt]).astype(np.float32), np.array(sorted(imgs)))
    out = tmp_path_factory.mktemp("clahe_plain")
    _cropper(landmarks).process_dir(str(d), str(out), desc=None)
    plain = _tree(out)
    assert sorted(plain) == sorted(imgs)
    crops = np.stack([_pixels(plain[n]) for n in sorted(plain)])
    want = R.clahe(crops, CLIP, 8)
    assert all(not np.array_equal(a, b) for a, b in zip(want, crops))
    return {"dir": d, "landmarks": landmarks, "plain": plain, "crops": crops, "want": want}


def test_process_dir_writes_the_equalised_crops(device, scene, tmp_path):
    c = _cropper(scene["landmarks"], clahe=CLIP)
    assert c.clahe_grid == 8 and c.par_model is None
    c.process_dir(str(scene["dir"]), str(tmp_path / "eq"), desc=None)
    got = _tree(tmp_path / "eq")
    assert sorted(got) == sorted(scene["plain"])
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), scene["want"][k]), n
    # another grid and clip limit
    c = _cropper(scene["landmarks"], clahe=4.0, clahe_grid=4)
    c.process_dir(str(scene["dir"]), str(tmp_path / "g4"), desc=None)
    want4 = R.clahe(scene["crops"], 4.0, 4)
    for k, (n, data) in enumerate(sorted(_tree(tmp_path / "g4").items())):
        assert np.array_equal(_pixels(data), want4[k]), n


def test_background_composites_the_equalised_crop_and_masks_are_unchanged(device, scene, tmp_path):
    """matte(reference-CLAHE(crop)): the parser sees the original crop, the fill colour stays exact."""
    spec = importlib.util.spec_from_file_location("_matte_ref", os.path.join(os.path.dirname(__file__), "matte_ref.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    groups = {"all": list(range(19))}
    parser = _cropper(scene["landmarks"], background=FILL).par_model
    labels = parser.parse(torch.from_numpy(scene["crops"]).to("cuda:0"))[0].cpu().numpy()
    fg = [int(np.bincount(labels.reshape(-1), minlength=19).argmax())]               # the most common class: some of each side
    hard = np.isin(labels, fg)
    assert all(m.any() and not m.all() for m in hard), "the generated parser does not split the crops"
    want, alpha = M.matte(scene["want"], labels, 1 << fg[0], 5, FILL)
    plainc = _cropper(scene["landmarks"], mask_groups=groups, background=FILL, foreground=fg)
    plainc.process_dir(str(scene["dir"]), str(tmp_path / "bg"), desc=None)
    c = _cropper(scene["landmarks"], mask_groups=groups, background=FILL, foreground=fg, clahe=CLIP)
    c.process_dir(str(scene["dir"]), str(tmp_path / "eqbg"), desc=None)
    base, got = _tree(tmp_path / "bg"), _tree(tmp_path / "eqbg")
    assert sorted(base) == sorted(got)
    masks = [n for n in got if "_mask" + os.sep in n]
    assert len(masks) == 3
    names = sorted(scene["plain"])
    for n in got:
        if n in masks:
            assert got[n] == base[n], n                                              # mask files are unchanged
            continue
        k = names.index(os.path.basename(n))
        px = _pixels(got[n])
        assert np.array_equal(px, want[k]), n
        assert (px[alpha[k] == 0] == np.array(FILL, np.uint8)).all()                 # the fill is exact
        assert not np.array_equal(px, _pixels(base[n]))
    assert (alpha == 0).any() and (alpha == 255).any()


def test_device_encoder_writes_the_jpeg_of_the_equalised_crop(device, scene, tmp_path):
    c = _cropper(scene["landmarks"], clahe=CLIP, encoder="device", output_format="jpg")
    c.process_dir(str(scene["dir"]), str(tmp_path / "dev"), desc=None)
    got = _tree(tmp_path / "dev")
    assert sorted(got) == ["a.jpg", "b.jpg", "c.jpg"]
    for data, ref in zip([got[n] for n in sorted(got)], c.encode_jpeg(scene["want"])):
        assert data == ref
    host = _cropper(scene["landmarks"], clahe=CLIP, encoder="host", output_format="jpg")
    host.process_dir(str(scene["dir"]), str(tmp_path / "host"), desc=None)
    assert _tree(tmp_path / "host") == got


def test_min_sharpness_scores_the_original_crop(device, scene, tmp_path):
    c = _cropper(scene["landmarks"])
    score = c.sharpness(scene["crops"])
    order = np.sort(score)
    assert order[0] < order[1]
    t = float(np.sqrt(max(order[0], 1e-9) * order[1])) if order[0] > 0 else float(order[1]) / 2
    kept = sorted(n for n, s in zip(sorted(scene["plain"]), score) if s >= t)
    assert 0 < len(kept) < 3
    assert not np.array_equal(c.sharpness(scene["want"]), score)                      # the equalised crops score differently
    c = _cropper(scene["landmarks"], min_sharpness=t, clahe=CLIP)
    c.process_dir(str(scene["dir"]), str(tmp_path / "eq"), desc=None)
    got = _tree(tmp_path / "eq")
    assert sorted(got) == kept
    names = sorted(scene["plain"])
    for n in got:
        assert np.array_equal(_pixels(got[n]), scene["want"][names.index(n)]), n
