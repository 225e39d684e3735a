"""Cropper(min_sharpness=...) without a GPU: properties of the reference tests/sharpness_ref.py, the C export and the op of
the sharpness kernel, the host score formula, the argument checks and the CLI flag."""
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
    spec = importlib.util.spec_from_file_location("_sharpness_ref", os.path.join(os.path.dirname(__file__), "sharpness_ref.py"))
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
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 1), (2, 2), (17, 23)])
def test_laplacian_equals_scipy_mirror(shape):
    from scipy import ndimage
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for _ in range(4):
        g = rng.integers(0, 256, shape, dtype=np.uint8)
        want = ndimage.laplace(g.astype(np.int64), mode="mirror")
        got = R.laplacian(g)
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert np.abs(got).max() <= 1020


def test_constant_image_has_zero_sums():
    for v in (0, 77, 255):
        img = np.full((9, 13, 3), v, np.uint8)
        assert R.sums(img) == (0, 0) and R.score(img) == 0.0


def test_checkerboard_is_the_extreme():
    for h, w in ((2, 2), (6, 10), (64, 64)):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
        lap = R.laplacian(R.gray(img))
        assert (np.abs(lap) == 1020).all()
        s1, s2 = R.sums(img)
        assert s1 == 0 and s2 == h * w * 1040400
        assert R.score(img) == 1040400.0


def test_ramp_has_zero_interior():
    yy, xx = np.mgrid[0:12, 0:15]
    g = (3 * xx + 5 * yy).astype(np.uint8)
    lap = R.laplacian(g)
    assert not lap[1:-1, 1:-1].any()
    assert lap[0].any() and lap[:, 0].any()            # the reflected border is not a ramp


def test_score_is_the_variance_of_the_laplacian():
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (3, 5), (17, 23), (64, 48)):
        img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
        var = R.laplacian(R.gray(img)).astype(np.float64).var()
        assert abs(R.score(img) - var) <= 1e-9 * max(var, 1e-300), shape


def test_gray_is_the_bt601_luma():
    assert R.gray(np.full((1, 1, 3), 255, np.uint8))[0, 0] == 255
    assert R.gray(np.zeros((1, 1, 3), np.uint8))[0, 0] == 0
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    corners = np.array([[[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)]], np.uint8)
    for a in (img, corners):
        got = R.gray(a)
        assert got.dtype == np.uint8
        luma = 0.299 * a[..., 0] + 0.587 * a[..., 1] + 0.114 * a[..., 2]
        assert np.abs(got.astype(np.float64) - luma).max() <= 1.0


# ---- the library and the op
def test_header_declares_and_library_exports_the_sharpness_kernel(native):
    import ctypes
    N = native
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    params = [p.strip() for p in norm(re.search(r"int fcp_crop_sharpness_u8\(([^)]*)\)", hdr).group(1)).split(",")]
    # the stream is the header's `fcp_stream_t` (`typedef void* fcp_stream_t; /* hipStream_t */`), as in every entry point
    assert params == ["const uint8_t* crops", "int f", "int h", "int w", "const int32_t* ok", "int64_t* sums",
                      "fcp_stream_t stream"]
    assert re.search(r"typedef void\* fcp_stream_t; /\* hipStream_t \*/", hdr)
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "fcp_crop_sharpness_u8")
    P, I = ctypes.c_void_p, ctypes.c_int
    assert N.SIGNATURES["fcp_crop_sharpness_u8"] == [P, I, I, I, P, P, P]
    assert "fcp_crop_sharpness_u8" in N.EXPORTS
    assert "#define FCP_ABI_VERSION 15" in hdr and N.ABI_VERSION == 15


def test_entry_point_checks_sizes_before_any_device_work(native):
    lib = native.lib()
    for f, h, w, word in ((1, 0, 4, b"bad sizes"), (1, 4, 0, b"bad sizes"), (-1, 4, 4, b"bad sizes"), (1, 4, 8193, b"8192"),
                          (1, (1 << 20) + 1, 4, b"1048576"), (65536, 4, 4, b"65535")):
        assert lib.fcp_crop_sharpness_u8(None, f, h, w, None, None, None) < 0, (f, h, w)
        assert word in lib.fcp_last_error(), (f, h, w, lib.fcp_last_error())
    assert lib.fcp_crop_sharpness_u8(None, 0, 4, 4, None, None, None) == 0          # f == 0: a no-op


def test_op_is_registered_and_refuses_cpu_tensors(native):
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    assert "crop_sharpness" in T.OPS
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcp::crop_sharpness", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcp::crop_sharpness", "CPU")
    assert str(torch.ops.fcp.crop_sharpness.default._schema) == "fcp::crop_sharpness(Tensor crops, Tensor? ok) -> Tensor"
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.crop_sharpness(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), None)


# ---- the host formula
def test_sharpness_score_is_exact_in_python_integers():
    from face_crop_plus_amd import align
    # 2048^2 checkerboard: N*S2 = 2^44 * 1040400 > 2^63 — int64 arithmetic would wrap
    n = 2048 * 2048
    sums = np.array([[0, n * 1040400], [12345, 987654321], [-7, 49], [0, 0]], np.int64)
    got = align.sharpness_score(sums, n)
    assert got.dtype == np.float64 and got.shape == (4,)
    assert got[0] == 1040400.0 and got[3] == 0.0
    for k in (1, 2):
        s1, s2 = int(sums[k, 0]), int(sums[k, 1])
        assert got[k] == (n * s2 - s1 * s1) / (n * n)
    assert align.sharpness_score(torch.from_numpy(sums), n).tolist() == got.tolist()       # a tensor is read back
    assert align.sharpness_score(np.zeros((0, 2), np.int64), 16).shape == (0,)
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (17, 23, 3), dtype=np.uint8)
    assert align.sharpness_score(np.array([R.sums(img)], np.int64), 17 * 23)[0] == R.score(img)


# ---- Cropper arguments, CLI
def test_cropper_checks_min_sharpness_without_a_device(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    params = inspect.signature(Cropper).parameters
    assert params["min_sharpness"].default is None
    assert list(params)[-2:] == ["interpolation", "min_sharpness"]
    for bad in (-1.0, -1e-9, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="min_sharpness"):
            Cropper(min_sharpness=bad)
    with pytest.raises(ValueError, match="min_sharpness"):
        Cropper(min_sharpness="12")
    with pytest.raises(ValueError, match="no alignment"):
        Cropper(min_sharpness=10.0, det_threshold=None, landmarks=None)
    # valid values get past the argument checks (and only then reach the models)
    for good, kw in ((0.0, {}), (150, {}), (3.5, {"det_threshold": None, "landmarks": (np.zeros((1, 5, 2)), np.array(["a"]))})):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(min_sharpness=good, **kw)


def test_cli_min_sharpness_flag(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    assert parse_args(["-i", str(tmp_path), "-ms", "120.5"])["min_sharpness"] == 120.5
    assert parse_args(["-i", str(tmp_path), "--min_sharpness", "40"])["min_sharpness"] == 40.0
    assert "min_sharpness" not in parse_args(["-i", str(tmp_path)])
    with pytest.raises(SystemExit):
        parse_args(["-i", str(tmp_path), "-ms", "sharp"])
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"min_sharpness": 75.0}))
    assert parse_args(["-i", str(tmp_path), "-c", str(cfg)])["min_sharpness"] == 75.0
    assert parse_args(["-i", str(tmp_path), "-c", str(cfg), "-ms", "5"])["min_sharpness"] == 5.0
