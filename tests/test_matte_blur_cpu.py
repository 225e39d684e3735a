"""Cropper(background_blur=...) without a GPU: the taps, the properties of the reference tests/matte_blur_ref.py, the
argument checks, the resolved defaults and the CLI flags."""
import importlib.util
import inspect
import json
import math
import os

import numpy as np
import pytest
import torch


def _load():
    spec = importlib.util.spec_from_file_location("_matte_blur_ref", os.path.join(os.path.dirname(__file__), "matte_blur_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
MR = R.MR
SIZES = [(1, 1), (1, 2), (2, 1), (3, 3), (5, 4), (7, 7), (13, 17)]


# ---- the taps
@pytest.mark.parametrize("sigma, radius", [(0.5, 3), (1, 3), (1.01, 4), (5.33, 16), (5.34, 17), (16, 48)])
def test_taps(sigma, radius):
    from face_crop_plus_amd import matte as M
    t = M.blur_taps(sigma)
    assert len(t) == radius + 1 == min(48, max(3, math.ceil(3 * sigma))) + 1
    assert all(isinstance(v, int) for v in t)
    assert t[0] + 2 * sum(t[1:]) == 4096 == M.TAP_SUM
    assert all(t[k] >= t[k + 1] for k in range(radius)) and t[radius] >= 1
    assert t == R.blur_taps(sigma)
    # the 32-bit bounds of the kernel follow from the sum
    assert 255 * 4096 < 2 ** 20 and 255 * 4096 ** 2 + 4096 ** 2 // 2 == 4286578688 < 2 ** 32


def test_taps_over_the_whole_range_of_sigma():
    from face_crop_plus_amd import matte as M
    for sigma in np.linspace(0.5, 16, 311):
        t = M.blur_taps(float(sigma))
        assert t[0] + 2 * sum(t[1:]) == 4096 and min(t) >= 1 and 3 <= len(t) - 1 <= 48


@pytest.mark.parametrize("bad", [0.49, 16.01, float("nan"), float("inf"), -float("inf"), True, False, "2", [2.0], 0, -1])
def test_sigma_is_checked(bad):
    from face_crop_plus_amd import matte as M
    with pytest.raises(ValueError, match="background_blur"):
        M.check_blur(bad)
    with pytest.raises(ValueError, match="background_blur"):
        M.blur_taps(bad)


def test_sigma_accepts_numbers():
    from face_crop_plus_amd import matte as M
    assert M.check_blur(None) is None
    assert M.check_blur(2) == 2.0 and M.check_blur(np.float32(0.5)) == 0.5 and M.check_blur(16) == 16.0
    with pytest.raises(ValueError):
        M.blur_taps(None)


# ---- the reference's own properties
def _cases():
    for h, w in SIZES:
        for pattern in R.PATTERNS:
            yield h, w, pattern


@pytest.mark.parametrize("sigma", [0.5, 16])
def test_alpha_below_255_implies_a_weight(sigma):
    taps = R.blur_taps(sigma)
    for h, w, pattern in _cases():
        rng = np.random.default_rng(100 * h + w)
        labels = R.labels_of(pattern, rng, 3, h, w)
        crops = MR.random_crops(rng, 3, h, w)
        for bits in (MR.DEFAULT_BITS, (1 << 1) | (1 << 5)):
            bg, d = R.background(crops, labels, bits, taps)
            for feather in MR.FEATHERS:
                alpha = R.alpha_of(labels, bits, feather)
                assert (d[alpha < 255] > 0).all(), (h, w, pattern, feather)
            # where nothing was seen the crop stands in
            assert (bg[d == 0] == crops[d == 0]).all()


def test_window_sums_against_python_integers():
    rng = np.random.default_rng(5)
    taps = R.blur_taps(1.3)
    r = len(taps) - 1
    planes = rng.integers(0, 256, (5, 6, 2)).astype(np.int64)
    got = R.window_sums(planes, taps)
    for y in range(5):
        for x in range(6):
            for p in range(2):
                want = sum(taps[abs(j)] * taps[abs(i)] * int(planes[y + j, x + i, p]) for j in range(-r, r + 1) for i in range(-r, r + 1)
                           if 0 <= y + j < 5 and 0 <= x + i < 6)
                assert got[y, x, p] == want


@pytest.mark.parametrize("feather", MR.FEATHERS)
def test_all_foreground_and_all_background(feather):
    rng = np.random.default_rng(11)
    taps = R.blur_taps(2.0)
    for h, w in SIZES:
        crops = MR.random_crops(rng, 2, h, w)
        out, alpha = R.matte_blur(crops, R.labels_of("all_fg", rng, 2, h, w), MR.DEFAULT_BITS, feather, taps)
        assert (alpha == 255).all() and (out == crops).all()
        labels = R.labels_of("all_bg", rng, 2, h, w)
        out, alpha = R.matte_blur(crops, labels, MR.DEFAULT_BITS, feather, taps)
        assert (alpha == 0).all() and (out == R.background(crops, labels, MR.DEFAULT_BITS, taps)[0]).all()


def test_a_uniform_background_stays_that_colour():
    rng = np.random.default_rng(12)
    for sigma in (0.5, 3.0, 16):
        taps = R.blur_taps(sigma)
        for h, w in SIZES[3:]:
            labels = MR.random_labels(rng, 2, h, w)
            labels[:, 0, 0] = 0
            crops = MR.random_crops(rng, 2, h, w)
            crops[MR.mask(labels, MR.DEFAULT_BITS) == 0] = (201, 3, 77)
            bg, d = R.background(crops, labels, MR.DEFAULT_BITS, taps)
            assert (d > 0).any() and (bg[d > 0] == np.array([201, 3, 77], np.uint8)).all()
            assert (bg[d == 0] == crops[d == 0]).all()


def test_no_halo_and_a_plain_blur_has_one():
    rng = np.random.default_rng(13)
    taps = R.blur_taps(2.0)
    h, w = 13, 17
    labels = np.zeros((2, h, w), np.uint8)
    labels[:, 4:9, 5:12] = 1
    subject = MR.mask(labels, MR.DEFAULT_BITS) == 255
    crops = MR.random_crops(rng, 2, h, w)
    other = crops.copy()
    other[subject] = 255 - other[subject]
    bg_a, _ = R.background(crops, labels, MR.DEFAULT_BITS, taps)
    bg_b, _ = R.background(other, labels, MR.DEFAULT_BITS, taps)
    assert (bg_a == bg_b).all()
    for feather in MR.FEATHERS:
        out_a, alpha = R.matte_blur(crops, labels, MR.DEFAULT_BITS, feather, taps)
        out_b, _ = R.matte_blur(other, labels, MR.DEFAULT_BITS, feather, taps)
        assert (alpha == 0).any() and (out_a[alpha == 0] == out_b[alpha == 0]).all()
    # the plain Gaussian of the crop is what leaks the subject into the background
    assert (R.plain_blur(crops, taps)[~subject] != R.plain_blur(other, taps)[~subject]).any()


# ---- constructor, defaults, CLI
def test_constructor_checks(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    assert inspect.signature(Cropper).parameters["background_blur"].default is None
    for bad in (0.49, 16.01, float("nan"), float("inf"), True, "3", (3,)):
        with pytest.raises(ValueError, match="background_blur"):
            Cropper(background_blur=bad)
    with pytest.raises(ValueError, match="exclude each other"):
        Cropper(background=0, background_blur=3.0)
    with pytest.raises(ValueError, match="need background"):
        Cropper(foreground=[1])
    with pytest.raises(ValueError, match="need background"):
        Cropper(feather=3)
    with pytest.raises(ValueError, match="no alignment"):
        Cropper(background_blur=3.0, det_threshold=None, landmarks=None)
    for bad in ([], [19], "face"):
        with pytest.raises(ValueError, match="foreground"):
            Cropper(background_blur=3.0, foreground=bad)
    with pytest.raises(ValueError, match="feather"):
        Cropper(background_blur=3.0, feather=4)
    for kw in ({"background_blur": 0.5}, {"background_blur": 16}, {"background_blur": 3.0, "foreground": [1, 17], "feather": 0},
               {"background_blur": np.float64(2.5), "feather": 7}):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(**kw)


def test_cropper_resolves_the_defaults(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    from face_crop_plus_amd import matte as M
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    c = Cropper(background_blur=4)
    assert (c.background, c.background_blur, c.foreground, c.foreground_bits, c.feather) == \
        (None, 4.0, tuple(range(1, 19)), MR.DEFAULT_BITS, 5)
    assert c.blur_taps == M.blur_taps(4.0) and len(c.blur_taps) == 13
    c = Cropper(background_blur=0.5, foreground=[17, 1], feather=0)
    assert (c.background, c.foreground, c.foreground_bits, c.feather, len(c.blur_taps)) == (None, (1, 17), (1 << 1) | (1 << 17), 0, 4)
    c = Cropper(background=9)
    assert (c.background, c.background_blur, c.blur_taps) == ((9, 9, 9), None, None)
    c = Cropper()
    assert (c.background, c.background_blur, c.blur_taps, c.foreground, c.feather) == (None, None, None, None, None)
    with pytest.raises(ValueError, match="background"):
        c.matte(np.zeros((1, 4, 4, 3), np.uint8), np.zeros((1, 4, 4), np.uint8))


def test_background_blur_alone_creates_the_parser(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import bise
    made = []

    class Parser:
        def __init__(self, attr_groups, mask_groups, batch_size):
            made.append((attr_groups, mask_groups))

        def load(self, device, weights, precision):
            made.append(weights)
    monkeypatch.setattr(bise, "BiSeNet", Parser)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: None)
    c = Cropper.__new__(Cropper)
    c.device, c.det_threshold, c.landmarks, c.enh_threshold = torch.device("cuda:0"), None, (None, None), None
    c.attr_groups, c.mask_groups, c.batch_size, c.weights, c.precision, c.encoder = None, None, 8, {"bisenet": "generated"}, None, "host"
    c.background, c.background_blur = None, None
    c._init_models()
    assert c.par_model is None and made == []
    c.background_blur = 3.0
    c._init_models()
    assert isinstance(c.par_model, Parser) and made == [(None, None), "generated"]


def test_cli_flags(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    plain = parse_args(base)
    assert "background_blur" not in plain
    assert parse_args(base + ["-bb", "3.5"])["background_blur"] == 3.5
    assert parse_args(base + ["--background-blur", "8"])["background_blur"] == 8.0
    got = parse_args(base + ["-bb", "2", "-fg", "[1,17]", "-fe", "3"])
    assert (got["background_blur"], got["foreground"], got["feather"]) == (2.0, [1, 17], 3)
    got = parse_args(base + ["-bb", "2"])
    assert {k: v for k, v in got.items() if k != "background_blur"} == plain          # nothing else moves
    for bad in (["-bb", "soft"], ["-bb"], ["-bg", "red"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"background-blur": 6.5, "feather": 7}))
    got = parse_args(base + ["-c", str(cfg)])
    assert got["background_blur"] == 6.5 and got["feather"] == 7


def test_c_export_refuses_bad_arguments_before_any_device_call():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    lib = N.lib()
    taps = R.blur_taps(2.0)
    t16 = (ctypes.c_uint16 * 49)(*taps)
    one = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its checks first

    def call(f=1, h=4, w=4, bits=2, feather=5, t=t16, radius=len(taps) - 1, ws=one, ws_bytes=1 << 20):
        return lib.fcp_matte_blur_u8(one, one, f, h, w, bits, feather, t, radius, one, None, ws, ws_bytes, None)
    assert lib.fcp_matte_blur_workspace_bytes(3, 5, 7) == 3 * 5 * 7 * 16
    assert lib.fcp_matte_blur_workspace_bytes(1, 8193, 1) == -1 and lib.fcp_matte_blur_workspace_bytes(1, 0, 1) == -1
    for kw, text in (({"feather": 4}, "feather"), ({"radius": 2}, "radius"), ({"radius": 49}, "radius"), ({"bits": 1 << 19}, "class_bits"),
                     ({"h": 8193}, "8192"), ({"w": 0}, "bad sizes"), ({"f": -1}, "bad sizes"), ({"t": None}, "taps"),
                     ({"radius": len(taps) - 2}, "sum to 4096"), ({"ws": None}, "workspace"), ({"ws_bytes": 255}, "workspace"),
                     ({"ws": ctypes.c_void_p(8)}, "aligned")):
        assert call(**kw) == -1, kw
        assert text in lib.fcp_last_error().decode(), (kw, lib.fcp_last_error())
    zero = (ctypes.c_uint16 * 49)(*([4094, 1, 0, 0]))
    assert call(t=zero, radius=3) == -1 and "tap 2 is 0" in lib.fcp_last_error().decode()
    assert call(f=0, ws=None, ws_bytes=0) == 0      # a no-op
