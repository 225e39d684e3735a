"""Cropper(background=...) without a GPU: arithmetic of the reference tests/matte_ref.py, the C export and the op of the
matte kernel, the argument checks and the CLI flags."""
import importlib.util
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("_matte_ref", os.path.join(os.path.dirname(__file__), "matte_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    return N


# ---- the reference
@pytest.mark.parametrize("feather", R.FEATHERS)
@pytest.mark.parametrize("shape", R.PIN_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_direct_separable_and_scipy_agree(shape, feather):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + feather)
    for _ in range(2 if shape[0] * shape[1] > 1000 else 4):
        m = R.random_mask(rng, *shape)
        direct, sep = R.alpha_direct(m, feather), R.alpha_separable(m, feather)
        assert direct.dtype == np.uint8 and sep.dtype == np.uint8
        assert np.array_equal(direct, sep)
        if feather == 0:
            assert np.array_equal(direct, m)
            continue
        k = np.array(R.TAPS[feather], np.int64)
        want = (ndimage.correlate(m.astype(np.int64), np.outer(k, k), mode="mirror") + 32768) >> 16
        assert np.array_equal(direct, want)


def test_reflect101_is_iterated():
    assert [R.reflect101(p, 1) for p in (-3, 0, 5)] == [0, 0, 0]
    assert [R.reflect101(p, 2) for p in range(-3, 5)] == [1, 0, 1, 0, 1, 0, 1, 0]
    assert [R.reflect101(p, 3) for p in range(-3, 6)] == [1, 2, 1, 0, 1, 2, 1, 0, 1]
    assert [R.reflect101(p, 5) for p in (-1, -2, 5, 6)] == [1, 2, 3, 2]


@pytest.mark.parametrize("feather", R.FEATHERS)
def test_uniform_masks_are_unchanged(feather):
    if feather:
        assert sum(R.TAPS[feather]) == 256 and R.TAPS[feather] == R.TAPS[feather][::-1]
    for shape in ((1, 1), (2, 7), (13, 17)):
        for v in (0, 255):
            m = np.full(shape, v, np.uint8)
            assert (R.alpha_direct(m, feather) == v).all() and (R.alpha_separable(m, feather) == v).all()


def test_division_shortcut_equals_rounded_division():
    t = np.arange(0, 65026, dtype=np.int64)
    u = t + 128
    assert np.array_equal((u + (u >> 8)) >> 8, (t + 127) // 255)
    # round to nearest, and no ties: 255 is odd
    assert np.array_equal((t + 127) // 255, np.rint(t / 255.0).astype(np.int64))
    assert not ((2 * t) % 255 == 0)[t % 255 != 0].any()


def test_composite_ends_and_mask():
    rng = np.random.default_rng(3)
    crop = R.random_crops(rng, 1, 5, 6)[0]
    assert np.array_equal(R.composite(crop, np.full((5, 6), 255, np.uint8), (1, 2, 3)), crop)
    assert (R.composite(crop, np.zeros((5, 6), np.uint8), (1, 2, 3)) == np.array([1, 2, 3], np.uint8)).all()
    labels = np.array([[0, 1, 17, 18, 19, 31, 32, 255]], np.uint8)
    assert R.mask(labels, R.DEFAULT_BITS).tolist() == [[0, 255, 255, 255, 0, 0, 0, 0]]
    assert R.mask(labels, (1 << 1) | (1 << 17)).tolist() == [[0, 255, 255, 0, 0, 0, 0, 0]]
    assert R.mask(labels, 1).tolist() == [[255, 0, 0, 0, 0, 0, 0, 0]]


# ---- the library and the op
def test_header_signatures_and_exports_agree(native):
    import ctypes
    N = native
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    params = [p.strip() for p in norm(re.search(r"int fcp_matte_u8\(([^)]*)\)", hdr).group(1)).split(",")]
    assert params == ["const uint8_t* crops", "const uint8_t* labels", "int f", "int h", "int w", "uint32_t class_bits",
                      "int feather", "int bg_r", "int bg_g", "int bg_b", "uint8_t* out", "uint8_t* alpha", "fcp_stream_t stream"]
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "fcp_matte_u8")
    P, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    assert N.SIGNATURES["fcp_matte_u8"] == [P, P, I, I, I, U, I, I, I, I, P, P, P]
    assert "fcp_matte_u8" in N.EXPORTS
    assert "#define FCP_ABI_VERSION 15" in hdr and N.ABI_VERSION == 15
    # the contract: in place is allowed and said so
    doc = norm(hdr[hdr.index("Background replacement of crops"):hdr.index("int fcp_matte_u8(")])
    assert "out MAY BE crops" in doc and "alpha may be NULL" in doc


def test_entry_point_refuses_before_any_device_work(native):
    lib = native.lib()
    bits = R.DEFAULT_BITS
    ok = dict(f=1, h=4, w=4, bits=bits, feather=5, r=0, g=0, b=0)
    for change, word in (({"f": -1}, b"bad sizes"), ({"h": 0}, b"bad sizes"), ({"w": 0}, b"bad sizes"), ({"h": 8193}, b"8192"),
                         ({"w": 8193}, b"8192"), ({"f": 65536}, b"65535"), ({"feather": 1}, b"feather"),
                         ({"feather": 4}, b"feather"), ({"feather": 9}, b"feather"), ({"feather": -3}, b"feather"),
                         ({"r": 256}, b"fill"), ({"g": -1}, b"fill"), ({"b": 1000}, b"fill"), ({"bits": 1 << 19}, b"class_bits"),
                         ({"bits": 1 << 31}, b"class_bits"), ({}, b"null pointer")):
        a = dict(ok, **change)
        rc = lib.fcp_matte_u8(None, None, a["f"], a["h"], a["w"], a["bits"], a["feather"], a["r"], a["g"], a["b"], None, None, None)
        assert rc < 0, change
        assert word in lib.fcp_last_error(), (change, lib.fcp_last_error())
    for feather in R.FEATHERS:                                                     # f == 0: a no-op
        assert lib.fcp_matte_u8(None, None, 0, 4, 4, bits, feather, 1, 2, 3, None, None, None) == 0


def test_op_is_registered_and_refuses_cpu_tensors(native):
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    assert "matte" in T.OPS
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcp::matte", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcp::matte", "CPU")
    assert str(torch.ops.fcp.matte.default._schema) == ("fcp::matte(Tensor crops, Tensor labels, int class_bits, int feather, "
                                                        "int bg_r, int bg_g, int bg_b, bool with_alpha) -> (Tensor, Tensor)")
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.matte(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8), 2, 5, 0, 0, 0, True)


# ---- Cropper arguments, CLI
def test_cropper_checks_background_without_a_device(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import bise
    from face_crop_plus_amd import cropper as CR
    from face_crop_plus_amd import matte as M

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    params = inspect.signature(Cropper).parameters
    assert [params[k].default for k in ("background", "foreground", "feather")] == [None, None, None]
    assert M.NUM_CLASSES == bise.NUM_CLASSES == 19
    for bad in (True, False, 1.5, -1, 256, "12", "1,2,3", (1, 2), (1, 2, 3, 4), (1, 2, 256), (0, -1, 0), (1, 2.5, 3), [1, 2, True],
                (), {}, float("nan")):
        with pytest.raises(ValueError, match="background"):
            Cropper(background=bad)
    for bad in ([], (), [19], [-1], [1, 2.5], [1, True], 5, "face"):
        with pytest.raises(ValueError, match="foreground"):
            Cropper(background=0, foreground=bad)
    for bad in (1, 2, 4, 6, 9, -3, 3.5, True, "5", (5,)):
        with pytest.raises(ValueError, match="feather"):
            Cropper(background=0, feather=bad)
    with pytest.raises(ValueError, match="need background"):
        Cropper(foreground=[1])
    with pytest.raises(ValueError, match="need background"):
        Cropper(feather=3)
    with pytest.raises(ValueError, match="need background"):
        Cropper(feather=0)
    with pytest.raises(ValueError, match="no alignment"):
        Cropper(background=0, det_threshold=None, landmarks=None)
    # valid values get past the argument checks (and only then reach the models)
    given = {"det_threshold": None, "landmarks": (np.zeros((1, 5, 2)), np.array(["a"]))}
    for kw in ({"background": 0}, {"background": 255}, {"background": 128.0}, {"background": (12, 200, 99)},
               {"background": [0, 0, 0], "foreground": [1, 17], "feather": 0}, {"background": np.array([1, 2, 3]), "feather": 7},
               {"background": 7, "foreground": range(1, 14), "feather": 3, **given}):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(**kw)
    # what the defaults resolve to
    assert M.check_background(None) is None and M.check_background(7) == (7, 7, 7) and M.check_background([1, 2, 3]) == (1, 2, 3)
    assert M.check_feather(None) == 5 and [M.check_feather(v) for v in R.FEATHERS] == list(R.FEATHERS)
    assert M.check_foreground(None) == sum(1 << c for c in range(1, 19)) == R.DEFAULT_BITS
    assert M.check_foreground([17, 1, 1]) == (1 << 1) | (1 << 17) and M.check_foreground([0]) == 1


def test_cropper_resolves_the_defaults(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    c = Cropper(background=9)
    assert (c.background, c.foreground, c.foreground_bits, c.feather) == ((9, 9, 9), tuple(range(1, 19)), R.DEFAULT_BITS, 5)
    c = Cropper(background=(1, 2, 3), foreground=[17, 1], feather=0)
    assert (c.background, c.foreground, c.foreground_bits, c.feather) == ((1, 2, 3), (1, 17), (1 << 1) | (1 << 17), 0)
    c = Cropper()
    assert (c.background, c.foreground, c.feather) == (None, None, None)
    with pytest.raises(ValueError, match="background"):
        c.matte(np.zeros((1, 4, 4, 3), np.uint8), np.zeros((1, 4, 4), np.uint8))


def test_background_alone_creates_the_parser(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import bise
    made, real = [], bise.BiSeNet

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
    c.background = None
    c._init_models()
    assert c.par_model is None and made == []
    c.background = (0, 0, 0)
    c._init_models()
    assert isinstance(c.par_model, Parser) and made == [(None, None), "generated"]
    # the real parser accepts having neither group
    neither = real()
    assert neither.attr_groups is None and neither.mask_groups is None
    assert inspect.signature(real.predict).parameters["return_labels"].default is False


def test_cli_flags(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    plain = parse_args(base)
    assert not {"background", "foreground", "feather"} & set(plain)
    assert parse_args(base + ["-bg", "12,34,56"])["background"] == [12, 34, 56]
    assert parse_args(base + ["--background", "7"])["background"] == 7
    assert parse_args(base + ["-bg", "0", "-fg", "[1,17]"])["foreground"] == [1, 17]
    assert parse_args(base + ["-bg", "0", "--foreground", "[2]", "-fe", "3"])["feather"] == 3
    assert parse_args(base + ["-bg", "0", "--feather", "0"])["feather"] == 0
    got = parse_args(base + ["-bg", "1,2,3"])
    assert {k: v for k, v in got.items() if k != "background"} == plain          # nothing else moves
    for bad in (["-bg", "red"], ["-bg", "1;2;3"], ["-fe", "soft"], ["-fg", "[1,"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"background": [0, 177, 64], "feather": 7}))
    got = parse_args(base + ["-c", str(cfg)])
    assert got["background"] == [0, 177, 64] and got["feather"] == 7
    assert parse_args(base + ["-c", str(cfg), "-bg", "5"])["background"] == 5
