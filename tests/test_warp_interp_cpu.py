"""Cropper(interpolation=...) without a GPU: the C exports and ops of the cubic / Lanczos-4 warps, the library's weight
table against tests/warp_interp_ref.py, properties of that reference, the argument checks and the CLI flag."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import align_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BORDERS = (0, 1, 2, 3, 4)


def _load():
    spec = importlib.util.spec_from_file_location("_warp_interp_ref", os.path.join(os.path.dirname(__file__),
                                                                                   "warp_interp_ref.py"))
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


def test_header_declares_and_library_exports_the_interp_warps(native):
    import ctypes
    N = native
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    params = lambda name: [p.strip() for p in norm(re.search(rf"int {name}\(([^)]*)\)", hdr).group(1)).split(",")]
    for linear, interp in (("fcp_warp_affine_u8", "fcp_warp_affine_u8_interp"),
                           ("fcp_warp_affine_u8_ragged", "fcp_warp_affine_u8_interp_ragged")):
        lp, ip = params(linear), params(interp)
        at = lp.index("int border") + 1
        assert ip == lp[:at] + ["int interp"] + lp[at:], interp          # the linear list with `int interp` after border
        assert hasattr(ctypes.CDLL(N.LIB_PATH), interp)
        want = list(N.SIGNATURES[linear])
        want.insert(at, ctypes.c_int)
        assert N.SIGNATURES[interp] == want
    assert params("fcp_warp_interp_weights") == ["int interp", "int16_t* out"]
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "fcp_warp_interp_weights")
    assert N.SIGNATURES["fcp_warp_interp_weights"] == [ctypes.c_int, ctypes.c_void_p]
    assert "#define FCP_ABI_VERSION 15" in hdr


def test_interp_ops_are_registered_and_refuse_cpu_tensors(native):
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    for name in ("warp_affine_u8_interp", "warp_affine_u8_interp_ragged"):
        assert name in T.OPS
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"fcp::{name}", "CUDA")
    schema = lambda n: str(getattr(torch.ops.fcp, n).default._schema).split("(", 1)[1]
    assert schema("warp_affine_u8_interp") == schema("warp_affine_u8").replace("int border)", "int border, int interp)")
    assert schema("warp_affine_u8_interp_ragged") == schema("warp_affine_u8_ragged").replace("int family)", "int interp)")
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.warp_affine_u8_interp(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32),
                                  torch.zeros(1, 2, 3, dtype=torch.float64), None, None, 4, 4, 0, 2)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.warp_affine_u8_interp_ragged(torch.zeros(192, dtype=torch.uint8), torch.tensor([[0, (8 << 32) | 8]]),
                                         torch.zeros(1, 2, 3, dtype=torch.float64), None, 4, 4, 0, 4)


@pytest.mark.parametrize("interp", [2, 4])
def test_library_weight_table_equals_reference(native, interp):
    K = R.TAPS[interp]
    out = np.zeros(1024 * K * K, np.int16)
    assert native.lib().fcp_warp_interp_weights(interp, out.ctypes.data) == 0
    out = out.reshape(1024, K, K)
    ref = R.weights_2d(interp)
    assert np.array_equal(out, ref)
    assert (out.reshape(1024, -1).astype(np.int64).sum(1) == 32768).all()
    # (0, 0): the centre tap saturates to 32767, the first entry of the correction block gets the missing 1
    h = K // 2
    assert out[0, h - 1, h - 1] == 32767 and out[0, h, h] == 1


def test_weight_export_refuses_other_methods(native):
    out = np.zeros(64 * 1024, np.int16)
    for bad in (0, 1, 3, 5, -2):
        assert native.lib().fcp_warp_interp_weights(bad, out.ctypes.data) < 0
        assert b"interpolation" in native.lib().fcp_last_error()
    assert not out.any()


def test_tables_follow_the_published_formulas():
    cub = R.tab1d(2)
    assert cub.dtype == np.float32 and cub.shape == (32, 4)
    assert np.array_equal(cub[0], np.float32([0, 1, 0, 0]))
    lan = R.tab1d(4)
    assert lan.shape == (32, 8) and abs(float(lan[0, 3]) - 1) < 1e-6 and np.abs(np.delete(lan[0], 3)).max() < 1e-20
    x = np.arange(32) / 32.0
    for t, interp in ((cub, 2), (lan, 4)):
        K = t.shape[1]
        d = x[:, None] - (np.arange(K) - (K // 2 - 1))[None, :]
        w = R.kernel_f64(interp, d)
        w = w / w.sum(1, keepdims=True)
        assert np.abs(t - w).max() < 1e-5, interp


def _rand_image(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("interp", [2, 4])
@pytest.mark.parametrize("border", BORDERS)
def test_identity_and_integer_shifts_reproduce_the_source(interp, border):
    rng = np.random.default_rng(7)
    img = _rand_image(rng, 23, 31)
    for tx, ty in ((0, 0), (3, -2), (-5, 4)):
        M = np.array([[1.0, 0.0, tx], [0.0, 1.0, ty]])
        out = R.warp_affine_interp(img, M, (31, 23), border, interp)
        ys, xs = np.mgrid[0:23, 0:31]
        sy, sx = ys - ty, xs - tx
        inside = (sx >= 0) & (sx < 31) & (sy >= 0) & (sy < 23)
        assert np.array_equal(out[inside], img[sy[inside], sx[inside]]), (tx, ty)
        if border == 0:
            assert not out[~inside].any()


@pytest.mark.parametrize("interp", [2, 4])
def test_interior_is_within_one_level_of_float64(interp):
    rng = np.random.default_rng(8)
    K = R.TAPS[interp]
    img = _rand_image(rng, 48, 64)
    for trial in range(6):
        s, th = rng.uniform(0.4, 5.0), rng.uniform(-np.pi, np.pi)
        M = np.array([[s * np.cos(th), -s * np.sin(th), 0], [s * np.sin(th), s * np.cos(th), 0]])
        c = M[:, :2] @ np.array([31.5, 23.5])
        M[:, 2] = np.array([20.0, 20.0]) - c + rng.uniform(-3, 3, 2)
        out = R.warp_affine_interp(img, M, (40, 40), 0, interp).astype(np.int64)
        X, Y = R.source_coords(M, (40, 40))
        sx, sy = (X >> 5) - (K // 2 - 1), (Y >> 5) - (K // 2 - 1)
        inner = (sx >= 0) & (sx <= 64 - K) & (sy >= 0) & (sy <= 48 - K)
        assert inner.sum() > 100
        fx, fy = (X & 31) / 32.0, (Y & 31) / 32.0
        taps = np.arange(K) - (K // 2 - 1)
        wx = R.kernel_f64(interp, fx[..., None] - taps)
        wy = R.kernel_f64(interp, fy[..., None] - taps)
        wx /= wx.sum(-1, keepdims=True)
        wy /= wy.sum(-1, keepdims=True)
        acc = np.zeros(X.shape + (3,))
        for r in range(K):
            for k in range(K):
                v = img[np.clip(sy + r, 0, 47), np.clip(sx + k, 0, 63)].astype(np.float64)
                acc += v * (wy[..., r] * wx[..., k])[..., None]
        want = np.clip(np.rint(acc), 0, 255)
        assert np.abs(out[inner] - want[inner]).max() <= 1, trial


@pytest.mark.parametrize("interp", [2, 4])
def test_constant_border_all_outside_is_zero(interp):
    K = R.TAPS[interp]
    img = np.full((9, 7, 3), 200, np.uint8)
    M = np.array([[1.0, 0.0, 20.0], [0.0, 1.0, 15.0]])
    out = R.warp_affine_interp(img, M, (40, 30), 0, interp)
    X, Y = R.source_coords(M, (40, 30))
    sx, sy = (X >> 5) - (K // 2 - 1), (Y >> 5) - (K // 2 - 1)
    outside = (sx >= 7) | (sx + K <= 0) | (sy >= 9) | (sy + K <= 0)
    assert outside.any() and not out[outside].any()
    assert out[~outside].any()


def test_batch_reference_unpads_and_zeroes_dropped_faces():
    rng = np.random.default_rng(9)
    imgs = rng.integers(0, 256, (2, 20, 24, 3), dtype=np.uint8)
    pads = np.array([[0, 0, 0, 0], [2, 3, 4, 5]], np.int32)
    M = np.array([[1.5, 0.2, -1.0], [-0.2, 1.5, 0.5]])
    out = R.warp_batch(imgs, [1, 0, 1], [M, M, M], [1, 1, 0], pads, (16, 12), 4, 4)
    assert np.array_equal(out[0], R.warp_affine_interp(imgs[1, 2:17, 4:19], M, (16, 12), 4, 4))
    assert np.array_equal(out[1], R.warp_affine_interp(imgs[0], M, (16, 12), 4, 4))
    assert not out[2].any()


def test_cropper_rejects_bad_interpolation_without_a_device(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    assert inspect.signature(Cropper).parameters["interpolation"].default == "linear"
    with pytest.raises(ValueError, match="interpolation"):
        Cropper(interpolation="bogus")
    with pytest.raises(ValueError, match="float32"):
        Cropper(interpolation="cubic", warp_family="float32")
    monkeypatch.setenv("FCP_WARP_FAMILY", "float32")
    with pytest.raises(ValueError, match="float32"):
        Cropper(interpolation="lanczos4")


def test_align_rejects_float32_with_cubic_or_lanczos():
    from face_crop_plus_amd import align
    assert align.INTERPOLATIONS == ("linear", "cubic", "lanczos4")
    for fn in (lambda: align.warp_affine(None, None, None, None, None, (4, 4), 0, "float32", "cubic"),
               lambda: align.crop_align(None, None, None, None, (4, 4), family="float32", interpolation="lanczos4"),
               lambda: align.warp_affine_ragged(None, None, None, None, (4, 4), 0, "float32", "cubic"),
               lambda: align.crop_align_sources(None, None, None, None, None, (4, 4), family="float32",
                                                interpolation="cubic")):
        with pytest.raises(ValueError, match="float32"):
            fn()
    with pytest.raises(ValueError, match="interpolation"):
        align.warp_affine(None, None, None, None, None, (4, 4), 0, interpolation="area")


def test_cli_interpolation_flag(tmp_path):
    import json
    from face_crop_plus_amd.__main__ import parse_args
    assert parse_args(["-i", str(tmp_path), "-ip", "cubic"])["interpolation"] == "cubic"
    assert parse_args(["-i", str(tmp_path), "--interpolation", "lanczos4"])["interpolation"] == "lanczos4"
    assert "interpolation" not in parse_args(["-i", str(tmp_path)])
    with pytest.raises(SystemExit):
        parse_args(["-i", str(tmp_path), "-ip", "area"])
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"interpolation": "lanczos4"}))
    assert parse_args(["-i", str(tmp_path), "-c", str(cfg)])["interpolation"] == "lanczos4"
