"""Cropper(background_image=...) without a GPU: the signature and the argument checks, the fit of the pictures against
the Pillow call INTEGRATION.md section 2r states, ``pick_pictures``, the properties of the reference
tests/matte_image_ref.py, the C exports, the ops, the documents and the CLI flags.

Every test fails without the feature: the keywords, ``matte.pick_pictures``, the reference file, the exports, the ops and
the flags do not exist there."""
import importlib.util
import inspect
import json
import os
import re
import warnings
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(os.path.dirname(__file__), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def R():
    return _load("matte_image_ref")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    return N


@pytest.fixture
def no_device(monkeypatch):
    """Any device work raises: what is refused was refused by the argument checks, what passes reaches the models."""
    from face_crop_plus_amd import cropper as CR

    def fail(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", fail)
    monkeypatch.setattr(torch.cuda, "set_device", fail)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)


@pytest.fixture
def no_models(monkeypatch):
    from face_crop_plus_amd import cropper as CR
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)


def _picture(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- signature
def test_signature_places_the_options_after_background_blur():
    from face_crop_plus_amd import Cropper
    params = inspect.signature(Cropper).parameters
    names = list(params)
    at = names.index("background_blur")
    assert names[at + 1:at + 3] == ["background_image", "background_fit"]
    assert params["background_image"].default is None and params["background_fit"].default is None
    matte = inspect.signature(Cropper.matte).parameters
    assert list(matte) == ["self", "crops", "labels", "picks"] and matte["picks"].default is None
    device = inspect.signature(Cropper._matte_device).parameters
    assert device["picks"].default is None and device["with_alpha"].default is False


# ---- argument checks
def test_cropper_checks_the_new_arguments_without_a_device(no_device, tmp_path):
    from PIL import Image
    from face_crop_plus_amd import Cropper
    pic = _picture(8, 8)
    with pytest.raises(ValueError, match="background_fit needs background_image"):
        Cropper(background_fit="cover")
    for fit in ("Cover", "fill", "contain", 1, b"cover", ("cover",)):
        with pytest.raises(ValueError, match="background_fit"):
            Cropper(background_image=pic, background_fit=fit)
    # one background mode at a time
    for other in ({"background": 0}, {"background": (1, 2, 3)}, {"background": "transparent", "output_format": "png"},
                  {"background_blur": 4}):
        with pytest.raises(ValueError, match="background_image excludes"):
            Cropper(background_image=pic, **other)
    with pytest.raises(ValueError, match="background_image needs aligned crops.*no alignment"):
        Cropper(background_image=pic, det_threshold=None, landmarks=None)
    # what applies with a colour fill applies here, with the same refusals
    with pytest.raises(ValueError, match="foreground"):
        Cropper(background_image=pic, foreground=[])
    with pytest.raises(ValueError, match="feather"):
        Cropper(background_image=pic, feather=4)
    with pytest.raises(ValueError, match="refine and feather"):
        Cropper(background_image=pic, refine=4, feather=5)
    with pytest.raises(ValueError, match="refine_eps needs refine"):
        Cropper(background_image=pic, refine_eps=64)
    for kw, word in (({"refine": 17}, "refine"), ({"subject": "all"}, "subject"), ({"fill_holes": 0}, "fill_holes"),
                     ({"edge_shift": 0}, "edge_shift"), ({"decontaminate": 17}, "decontaminate")):
        with pytest.raises(ValueError, match=word):
            Cropper(background_image=pic, **kw)
    # the checks that need a background mode keep their messages without one
    for kw, message in (({"foreground": [1]}, "foreground / feather need background or background_blur"),
                        ({"feather": 3}, "foreground / feather need background or background_blur"),
                        ({"refine": 4}, "refine needs background or background_blur"),
                        ({"subject": "largest"}, "subject / fill_holes need background or background_blur"),
                        ({"fill_holes": 9}, "subject / fill_holes need background or background_blur"),
                        ({"edge_shift": -2}, "edge_shift needs background or background_blur"),
                        ({"decontaminate": 4}, "decontaminate needs background")):
        with pytest.raises(ValueError, match=message):
            Cropper(**kw)
    # the pictures themselves
    empty = tmp_path / "empty"
    empty.mkdir()
    (tmp_path / "notes.txt").write_text("not a picture")
    for bad in ([], (), str(empty), str(tmp_path / "missing.png"), str(tmp_path / "notes.txt"), np.zeros((8, 8), np.uint8),
                np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 3), np.float32), np.zeros((0, 8, 3), np.uint8),
                np.zeros((8, 0, 3), np.uint8), np.zeros((2, 8, 8, 3), np.uint8), [pic, np.zeros((8, 8), np.uint8)], [[pic]], 7,
                {"a": pic}):
        with pytest.raises(ValueError, match="background_image"), warnings.catch_warnings():
            warnings.simplefilter("ignore")                  # the decoder's own warning for the file it cannot read
            Cropper(background_image=bad)
    # the bank's bounds, with the size in the message: 1 GiB and 4096 pictures
    with pytest.raises(ValueError, match=r"1100 pictures of 1024 x 512 px needs 1730150400 bytes"):
        Cropper(background_image=[_picture(2, 2)] * 1100, output_size=(1024, 512))
    with pytest.raises(ValueError, match=r"at most 4096 pictures \(got 4097\)"):
        Cropper(background_image=[_picture(2, 2)] * 4097, output_size=4)
    # valid values get past the argument checks (and only then reach the models)
    Image.fromarray(pic).save(tmp_path / "one.png")
    full = tmp_path / "full"
    full.mkdir()
    Image.fromarray(pic).save(full / "p.png")
    for kw in ({"background_image": pic}, {"background_image": [pic, pic], "background_fit": "stretch"},
               {"background_image": (pic,), "background_fit": "cover", "output_size": (48, 32)},
               {"background_image": str(tmp_path / "one.png")}, {"background_image": str(full)},
               {"background_image": [str(full), pic, tmp_path / "one.png"]},
               {"background_image": pic, "foreground": [1, 17], "feather": 7, "decontaminate": 4},
               {"background_image": pic, "refine": 4, "refine_eps": 16, "subject": "largest", "fill_holes": 50, "edge_shift": -2,
                "decontaminate": 0.5, "output_format": "jpg"},
               {"background_image": [_picture(2, 2)] * 4096, "output_size": 4}):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(**kw)


def test_cropper_resolves_the_new_defaults(no_models):
    from face_crop_plus_amd import Cropper
    c = Cropper()
    assert (c.background_image, c.background_fit) == (None, None) and not c._has_background()
    assert Cropper(background=0)._has_background() and Cropper(background_blur=2)._has_background()
    pic = _picture(24, 32)
    c = Cropper(background_image=pic, output_size=(32, 24))
    assert c.background_fit == "cover" and c.background is None and c.background_blur is None and c._has_background()
    assert c.background_image.shape == (1, 24, 32, 3) and np.array_equal(c.background_image[0], pic)
    assert c.feather == 5 and c.foreground == tuple(range(1, 19)) and c.decontaminate_taps is None
    c = Cropper(background_image=[pic, pic[::-1]], background_fit="stretch", output_size=16, refine=3, decontaminate=4)
    assert c.background_fit == "stretch" and c.background_image.shape == (2, 16, 16, 3) and c.background_image.dtype == np.uint8
    assert c.feather == 0 and c.refine == 3 and len(c.decontaminate_taps) == 13
    # Cropper.matte refuses on the host what it can
    crops, labels = np.zeros((2, 16, 16, 3), np.uint8), np.zeros((2, 16, 16), np.uint8)
    for picks in ([0], [0, 1, 0], [0, 2], [-1, 0], [0.5, 1], "01"):
        with pytest.raises(ValueError, match="picks"):
            c.matte(crops, labels, picks)
    with pytest.raises(ValueError, match="output size"):
        c.matte(np.zeros((2, 16, 8, 3), np.uint8), np.zeros((2, 16, 8), np.uint8))
    with pytest.raises(ValueError, match="picks need a Cropper with background_image"):
        Cropper(background=0).matte(crops, labels, [0, 0])
    with pytest.raises(ValueError, match="background_image"):
        Cropper().matte(crops, labels)
    # a Cropper made without __init__ has no background mode
    bare = Cropper.__new__(Cropper)
    bare.background = None
    assert not bare._has_background()


def test_background_image_alone_creates_the_parser(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import bise
    made, uploads = [], []

    class Parser:
        def __init__(self, attr_groups, mask_groups, batch_size):
            made.append((attr_groups, mask_groups))

        def load(self, device, weights, precision):
            made.append(weights)

    class Bank:
        def to(self, device):
            uploads.append(device)
            return "the bank on the device"
    monkeypatch.setattr(bise, "BiSeNet", Parser)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: None)
    monkeypatch.setattr(torch, "from_numpy", lambda a: Bank())
    c = Cropper(background_image=_picture(8, 8), output_size=8, device="cuda:0", weights={"bisenet": "generated"},
                det_threshold=None, landmarks=(np.zeros((1, 5, 2), np.float32), np.array(["a"])))
    assert isinstance(c.par_model, Parser) and made == [(None, None), "generated"]
    assert uploads == [torch.device("cuda:0")] and c._pictures_dev == "the bank on the device"      # once, at construction


# ---- the fit
def _cover_box(W, H, ow, oh):
    s = max(ow / W, oh / H)
    bw, bh = ow / s, oh / s
    box = ((W - bw) / 2, (H - bh) / 2, (W + bw) / 2, (H + bh) / 2)
    return (min(max(box[0], 0), W), min(max(box[1], 0), H), min(max(box[2], 0), W), min(max(box[3], 0), H))


def test_fit_is_the_stated_pillow_call(monkeypatch):
    from PIL import Image
    from face_crop_plus_amd import matte as M
    ow, oh = 48, 32
    same = _picture(oh, ow, 3)
    calls = []
    real = Image.Image.resize
    monkeypatch.setattr(Image.Image, "resize", lambda self, *a, **k: calls.append(a) or real(self, *a, **k))
    for fit in M.FITS:
        got = M.fit_picture(same, (ow, oh), fit)
        assert got.tobytes() == same.tobytes() and got.shape == (oh, ow, 3)
    assert calls == []                                             # byte for byte, no resample call
    monkeypatch.undo()
    assert _cover_box(100, 40, ow, oh) == (20.0, 0.0, 80.0, 40.0) and _cover_box(40, 100, ow, oh)[0::2] == (0.0, 40.0)
    for H, W in ((40, 100), (100, 40)):
        p = _picture(H, W, H)
        for fit, box in (("stretch", (0, 0, W, H)), ("cover", _cover_box(W, H, ow, oh))):
            want = np.asarray(Image.fromarray(p).resize((ow, oh), Image.Resampling.LANCZOS, box=box))
            got = M.fit_picture(p, (ow, oh), fit)
            assert got.shape == (oh, ow, 3) and got.dtype == np.uint8 and np.array_equal(got, want), (H, W, fit)
        assert not np.array_equal(M.fit_picture(p, (ow, oh), "cover"), M.fit_picture(p, (ow, oh), "stretch"))
        bank = M.picture_bank([p, same], (ow, oh), "cover")
        assert bank.shape == (2, oh, ow, 3) and np.array_equal(bank[0], M.fit_picture(p, (ow, oh))) and np.array_equal(bank[1], same)
    assert M.check_fit(None) == "cover" and M.check_fit("stretch") == "stretch"


def test_pictures_come_from_files_directories_arrays_and_lists(tmp_path):
    from PIL import Image
    from face_crop_plus_amd import matte as M
    d = tmp_path / "bank"
    d.mkdir()
    rgb = {name: _picture(6, 5, i) for i, name in enumerate(("b.png", "a.png", "c.bmp"))}
    for name, p in rgb.items():
        Image.fromarray(p).save(d / name)
    (d / "readme.txt").write_text("the decoder does not read this")
    with pytest.warns(UserWarning, match="readme.txt"):
        got = M.load_pictures(str(d))
    assert len(got) == 3 and all(np.array_equal(g, rgb[n]) for g, n in zip(got, ("a.png", "b.png", "c.bmp")))   # sorted names
    gray = np.arange(30, dtype=np.uint8).reshape(6, 5)
    Image.fromarray(gray).save(tmp_path / "gray.png")
    rgba = np.random.default_rng(5).integers(0, 256, (6, 5, 4), dtype=np.uint8)
    Image.fromarray(rgba).save(tmp_path / "rgba.png")
    (g,), (a,) = M.load_pictures(str(tmp_path / "gray.png")), M.load_pictures(tmp_path / "rgba.png")
    assert g.shape == a.shape == (6, 5, 3) and g.dtype == a.dtype == np.uint8
    assert np.array_equal(g, np.repeat(gray[..., None], 3, -1)) and np.array_equal(a, rgba[..., :3])
    array = _picture(3, 4, 9)
    with pytest.warns(UserWarning, match="readme.txt"):
        mixed = M.load_pictures([str(tmp_path / "gray.png"), array, str(d)])
    assert len(mixed) == 5 and np.array_equal(mixed[0], g) and np.array_equal(mixed[1], array) and np.array_equal(mixed[2], rgb["a.png"])
    assert np.array_equal(M.load_pictures(array[:, ::-1])[0], array[:, ::-1])             # a view is taken as it is
    with pytest.warns(UserWarning, match="readme.txt"):
        bank = M.picture_bank(str(d), (5, 6))
    assert bank.shape == (3, 6, 5, 3) and np.array_equal(bank[2], rgb["c.bmp"])


# ---- pick_pictures
def test_pick_pictures_is_crc32_of_the_stem():
    from face_crop_plus_amd import matte as M
    names = ["a.png", "b.jpg", "a_0.png", "a_1.png", "out/dir/photo 12.jpeg", "señor_ñandú.png", "no_extension", "x.tar.gz"]
    stems = ["a", "b", "a_0", "a_1", "photo 12", "señor_ñandú", "no_extension", "x.tar"]
    assert M.pick_pictures(names, 1) == [0] * len(names)
    for k in (2, 3, 7, 64, 4096):
        want = [zlib.crc32(s.encode("utf-8")) % k for s in stems]
        assert M.pick_pictures(names, k) == want, k
        assert M.pick_pictures(np.array(names), k) == want
        # a face's pick does not depend on the other names, their order or how they are split into batches
        order = np.random.default_rng(k).permutation(len(names))
        assert M.pick_pictures([names[i] for i in order], k) == [want[i] for i in order]
        assert M.pick_pictures(names[:3], k) + M.pick_pictures(names[3:], k) == want
        assert [M.pick_pictures([n], k)[0] for n in names] == want
    assert zlib.crc32("a_0".encode("utf-8")) % 7 != zlib.crc32("a_1".encode("utf-8")) % 7      # the faces of one photo differ
    assert M.pick_pictures(["a.png"], 5) == M.pick_pictures(["somewhere/else/a.jpg"], 5)
    assert M.pick_pictures([], 3) == []


def test_process_passes_picks_of_the_written_names(no_models):
    """strategy "all": the stem of a face is "<source stem>_<k>", as its file in the main output directory is named."""
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import matte as M
    c = Cropper(background_image=[_picture(4, 4, i) for i in range(5)], output_size=4, strategy="all", output_format="png")
    paths = c._target_paths(np.array(["p.jpg", "q.jpg", "p.jpg"]), "out")
    assert [os.path.basename(p) for p in paths] == ["p_0.png", "q_0.png", "p_1.png"]
    assert M.pick_pictures(paths, 5) == [zlib.crc32(s.encode()) % 5 for s in ("p_0", "q_0", "p_1")]


# ---- the reference
def test_reference_with_a_constant_picture_is_the_colour_fill(R):
    rng = np.random.default_rng(21)
    colour = (0, 177, 64)
    for h, w in ((1, 1), (5, 3), (13, 17)):
        crops, labels = R.MR.random_crops(rng, 3, h, w), R.MR.random_labels(rng, 3, h, w)
        bank = np.concatenate([R.random_bank(rng, 1, h, w), R.constant_bank(colour, h, w)])
        for feather in (0, 3, 5, 7):
            want, want_a = R.MR.matte(crops, labels, R.MR.DEFAULT_BITS, feather, colour)
            got, alpha = R.matte_image(crops, labels, R.MR.DEFAULT_BITS, feather, bank, [1, 1, 1])
            assert np.array_equal(got, want) and np.array_equal(alpha, want_a), (h, w, feather)
            assert got.dtype == np.uint8 and got.shape == crops.shape


def test_reference_shows_the_picture_behind_and_the_crop_in_front(R):
    rng = np.random.default_rng(22)
    h, w = 9, 11
    crops, bank = R.MR.random_crops(rng, 3, h, w), R.random_bank(rng, R.K, h, w)
    zeros, ones = np.zeros((3, h, w), np.uint8), np.full((3, h, w), 255, np.uint8)
    assert np.array_equal(R.behind(bank, R.PICKS), np.stack([bank[1], bank[0], bank[1]]))
    assert np.array_equal(R.composite(crops, zeros, bank, R.PICKS), R.behind(bank, R.PICKS))
    assert np.array_equal(R.composite(crops, ones, bank, R.PICKS), crops)
    alpha = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    alpha[0, 0, :3] = (0, 255, 128)
    out = R.composite(crops, alpha, bank, R.PICKS)
    assert np.array_equal(out[alpha == 0], R.behind(bank, R.PICKS)[alpha == 0]) and np.array_equal(out[alpha == 255], crops[alpha == 255])
    c, p, a = int(crops[0, 0, 2, 1]), int(bank[1, 0, 2, 1]), 128
    assert out[0, 0, 2, 1] == (c * a + p * (255 - a) + 127) // 255
    # every face on its own
    for i, pick in enumerate(R.PICKS):
        assert np.array_equal(R.composite(crops[i:i + 1], alpha[i:i + 1], bank, [pick]), out[i:i + 1])
    assert R.composite(crops[:0], alpha[:0], bank, []).shape == (0, h, w, 3)


def test_reference_with_taps_and_a_constant_picture_is_cutout_fill(R):
    from face_crop_plus_amd import matte as M
    rng = np.random.default_rng(23)
    h, w = 17, 9
    colour = (12, 34, 56)
    crops = R.MR.random_crops(rng, 3, h, w)
    bank = R.constant_bank(colour, h, w, 2)
    for kind in ("disc5", "random", "zeros", "ones"):
        alpha = R.CR.alpha_of(kind, rng, 3, h, w)
        for sigma in (0.5, 4):
            taps = M.blur_taps(sigma)
            assert np.array_equal(R.composite(crops, alpha, bank, R.PICKS, taps), R.CR.fill(crops, alpha, taps, colour)), (kind, sigma)
    # where the alpha is 0 the result is the picture, whatever F is
    alpha = R.CR.alpha_of("random", rng, 3, h, w)
    rbank = R.random_bank(rng, 2, h, w)
    out = R.composite(crops, alpha, rbank, R.PICKS, M.blur_taps(4))
    assert (alpha == 0).any() and np.array_equal(out[alpha == 0], R.behind(rbank, R.PICKS)[alpha == 0])


def test_shape_list_crosses_the_kernel_s_tiles(R):
    src = open(os.path.join(ROOT, "face-crop-plus_amd", "csrc", "fcp_matte.hip")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    tw, th = const("kTileW"), const("kTileH")
    assert R.SHAPES == [(1, 1), (1, 7), (5, 3), (33, 47), (64, 64), (70, 130)] and (R.F, R.K, R.PICKS) == (3, 2, (1, 0, 1))
    assert (tw, th) == (64, 32) and (64, 64) in R.SHAPES                          # whole tiles
    assert any(h > 2 * th and w > 2 * tw and h % th and w % tw for h, w in R.SHAPES)   # several tiles both ways, ragged
    assert any(w < 4 for _, w in R.SHAPES) and any(w % 4 and (3 * w) % 4 for _, w in R.SHAPES)


# ---- the library and the ops
def test_header_signatures_and_exports_agree(native):
    import ctypes
    N = native
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    params = lambda name: [p.strip() for p in norm(re.search(r"int %s\(([^)]*)\)" % name, hdr).group(1)).split(",")]
    assert params("fcp_matte_image_u8") == ["const uint8_t* crops", "const uint8_t* labels", "int f", "int h", "int w",
                                            "uint32_t class_bits", "int feather", "const uint8_t* pictures", "int k",
                                            "const int32_t* picks", "uint8_t* out", "uint8_t* alpha", "fcp_stream_t stream"]
    assert params("fcp_matte_image_alpha_u8") == ["const uint8_t* crops", "const uint8_t* alpha", "int f", "int h", "int w",
                                                  "const uint8_t* pictures", "int k", "const int32_t* picks", "uint8_t* out",
                                                  "fcp_stream_t stream"]
    assert params("fcp_cutout_image_u8") == ["const uint8_t* crops", "const uint8_t* alpha", "int f", "int h", "int w",
                                             "const uint8_t* pictures", "int k", "const int32_t* picks", "const uint16_t* taps",
                                             "int radius", "uint8_t* out", "void* workspace", "int64_t workspace_bytes",
                                             "fcp_stream_t stream"]
    Pt, I, U, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_int64
    assert N.SIGNATURES["fcp_matte_image_u8"] == [Pt, Pt, I, I, I, U, I, Pt, I, Pt, Pt, Pt, Pt]
    assert N.SIGNATURES["fcp_matte_image_alpha_u8"] == [Pt, Pt, I, I, I, Pt, I, Pt, Pt, Pt]
    assert N.SIGNATURES["fcp_cutout_image_u8"] == [Pt, Pt, I, I, I, Pt, I, Pt, Pt, I, Pt, Pt, L, Pt]
    lib = N.lib()
    for name in ("fcp_matte_image_u8", "fcp_matte_image_alpha_u8", "fcp_cutout_image_u8"):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert "#define FCP_ABI_VERSION 15" in hdr and N.ABI_VERSION == 15 and lib.fcp_abi_version() == 15
    from face_crop_plus_amd import matte as M
    fill = open(os.path.join(ROOT, "face-crop-plus_amd", "csrc", "fcp_fill.h")).read()
    assert M.MAX_PICTURES == 4096 == int(re.search(r"constexpr int kMaxPictures = (\d+);", fill).group(1))
    assert M.MAX_BANK_BYTES == 1 << 30


def test_entry_points_refuse_before_any_device_work(native):
    """Null pointers everywhere: a call that got past its checks would fault, a refused one returns with its message."""
    import ctypes
    from face_crop_plus_amd import matte as M
    lib = native.lib()
    bits = sum(1 << c for c in range(1, 19))
    ok = dict(f=1, h=4, w=4, bits=bits, feather=5, k=2)
    sizes = (({"f": -1}, b"bad sizes"), ({"h": 0}, b"bad sizes"), ({"w": 0}, b"bad sizes"), ({"h": 8193}, b"8192"),
             ({"w": 8193}, b"8192"), ({"f": 65536}, b"65535"))
    banks = (({"k": 0}, b"1..4096 pictures"), ({"k": -1}, b"1..4096 pictures"), ({"k": 4097}, b"1..4096 pictures"))
    for change, word in sizes + banks + (({"feather": 4}, b"feather"), ({"feather": 9}, b"feather"), ({"bits": 1 << 19}, b"class_bits"),
                                         ({}, b"null pointer"), ({"k": 4096}, b"null pointer")):
        a = dict(ok, **change)
        assert lib.fcp_matte_image_u8(None, None, a["f"], a["h"], a["w"], a["bits"], a["feather"], None, a["k"], None, None, None,
                                      None) < 0, change
        assert word in lib.fcp_last_error() and lib.fcp_last_error().startswith(b"matte_image:"), (change, lib.fcp_last_error())
    assert lib.fcp_matte_image_u8(None, None, 0, 4, 4, bits, 5, None, 2, None, None, None, None) == 0          # f == 0: a no-op
    for change, word in sizes + banks + (({}, b"null pointer"),):
        a = dict(ok, **change)
        assert lib.fcp_matte_image_alpha_u8(None, None, a["f"], a["h"], a["w"], None, a["k"], None, None, None) < 0, change
        assert word in lib.fcp_last_error() and lib.fcp_last_error().startswith(b"matte_image_alpha:"), (change, lib.fcp_last_error())
    assert lib.fcp_matte_image_alpha_u8(None, None, 0, 4, 4, None, 2, None, None, None) == 0
    taps = M.blur_taps(4)
    t16 = (ctypes.c_uint16 * 49)(*taps)
    short = (ctypes.c_uint16 * 49)(*([taps[0] - 2] + taps[1:]))
    zero = (ctypes.c_uint16 * 49)(*([taps[0] + 2 * taps[-1]] + taps[1:-1] + [0]))
    ok = dict(f=1, h=4, w=4, k=2, taps=t16, radius=len(taps) - 1)
    for change, word in sizes + banks + (({"radius": 0}, b"fcp_matte_image_alpha_u8"), ({"radius": 1}, b"radius"),
                                         ({"radius": 2}, b"radius"), ({"radius": 49}, b"radius"), ({"radius": -3}, b"radius"),
                                         ({"taps": None}, b"null taps"), ({"taps": short}, b"sum to 4096"),
                                         ({"taps": zero}, b"at least 1"), ({"radius": 11}, b"sum to 4096"), ({}, b"null pointer")):
        a = dict(ok, **change)
        assert lib.fcp_cutout_image_u8(None, None, a["f"], a["h"], a["w"], None, a["k"], None, a["taps"], a["radius"], None, None, 0,
                                       None) < 0, change
        assert word in lib.fcp_last_error() and lib.fcp_last_error().startswith(b"cutout_image:"), (change, lib.fcp_last_error())
    assert lib.fcp_cutout_image_u8(None, None, 0, 4, 4, None, 2, None, t16, len(taps) - 1, None, None, 0, None) == 0


def test_ops_are_registered_and_refuse_cpu_tensors(native):
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    names = ("matte_image", "matte_image_alpha", "cutout_image")
    for name in names:
        assert name in T.OPS and hasattr(ops, name)
        assert torch._C._dispatch_has_kernel_for_dispatch_key("fcp::" + name, "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcp::" + name, "CPU")
    assert str(torch.ops.fcp.matte_image.default._schema) == (
        "fcp::matte_image(Tensor crops, Tensor labels, int class_bits, int feather, Tensor pictures, Tensor picks, bool with_alpha) "
        "-> (Tensor, Tensor)")
    assert str(torch.ops.fcp.matte_image_alpha.default._schema) == (
        "fcp::matte_image_alpha(Tensor crops, Tensor alpha, Tensor pictures, Tensor picks) -> Tensor")
    assert str(torch.ops.fcp.cutout_image.default._schema) == (
        "fcp::cutout_image(Tensor crops, Tensor alpha, Tensor pictures, Tensor picks, int[] taps) -> Tensor")
    crops, plane = torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    bank, picks = torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.matte_image(crops, plane, 2, 5, bank, picks, False)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.matte_image_alpha(crops, plane, bank, picks)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.cutout_image(crops, plane, bank, picks, [4090, 1, 1, 1])


def test_wrappers_check_the_bank_and_the_picks_on_the_host():
    """Before anything is uploaded or launched: host tensors stand in for device ones."""
    from face_crop_plus_amd import matte as M
    crops, labels = torch.zeros(2, 8, 6, 3, dtype=torch.uint8), torch.zeros(2, 8, 6, dtype=torch.uint8)
    bank = torch.zeros(3, 8, 6, 3, dtype=torch.uint8)
    for picks in ([0], [0, 1, 2], [0, 3], [-1, 0], [0, 1.5], [True, 0]):
        with pytest.raises(ValueError, match="picks"):
            M.matte_image(crops, labels, 2, 5, bank, picks)
        with pytest.raises(ValueError, match="picks"):
            M.cutout_image(crops, labels, bank, picks, M.blur_taps(4))
    for bad in (bank[:, :, :5], bank[:, :7], bank.float(), bank[:0], bank[..., :2], bank.numpy(), bank.permute(0, 2, 1, 3), bank[0]):
        with pytest.raises(ValueError, match="pictures"):
            M.matte_image(crops, labels, 2, 5, bad, [0, 1])
        with pytest.raises(ValueError, match="pictures"):
            M.cutout_image(crops, labels, bad, [0, 1], M.blur_taps(4))


# ---- documents, CLI
def test_docs_mention_the_options():
    readme = open(os.path.join(ROOT, "README.md")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    tools = open(os.path.join(ROOT, "tools", "README.md")).read()
    assert "background_image" in readme and "background_fit" in readme and "--background-image" in readme
    section = re.sub(r"\s+", " ", integration[integration.index("## 2r."):integration.index("## 3.")])     # line breaks aside
    for phrase in ("background_image", "background_fit", '"cover"', '"stretch"', "pick_pictures", "crc32", "fcp_matte_image_u8",
                   "fcp_matte_image_alpha_u8", "fcp_cutout_image_u8", "Image.Resampling.LANCZOS", "tests/matte_image_ref.py",
                   "tools/bench_matte_image.py", "--background-image", "--background-fit"):
        assert phrase in section, phrase
    assert "bench_matte_image.py" in tools and os.path.isfile(os.path.join(ROOT, "tools", "bench_matte_image.py"))


def test_cli_flags(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    plain = parse_args(base)
    assert not {"background_image", "background_fit"} & set(plain)
    assert parse_args(base + ["-bi", "a.png"])["background_image"] == ["a.png"]
    got = parse_args(base + ["--background-image", "a.png", "dir", "b.jpg", "--background-fit", "stretch"])
    assert got["background_image"] == ["a.png", "dir", "b.jpg"] and got["background_fit"] == "stretch"
    assert parse_args(base + ["-bi", "dir", "-bf", "cover"])["background_fit"] == "cover"
    got = parse_args(base + ["-bi", "dir", "-bf", "cover"])
    assert {k: v for k, v in got.items() if k not in ("background_image", "background_fit")} == plain     # nothing else moves
    for bad in (["-bi"], ["-bf", "contain"], ["-bf"], ["-bi", "a.png", "-bf", "Cover"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"background_image": "bank", "background-fit": "stretch", "decontaminate": 2}))
    got = parse_args(base + ["-c", str(cfg)])
    assert got["background_image"] == "bank" and got["background_fit"] == "stretch" and got["decontaminate"] == 2
