"""Cropper(clahe=...) without a GPU: hand-computable cases and invariants of the reference tests/clahe_ref.py, the
branches the GPU test's inputs reach, the C export and the op of the CLAHE kernels, the argument checks and the CLI flags."""
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("_clahe_ref", os.path.join(os.path.dirname(__file__), "clahe_ref.py"))
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


# ---- the reference: cases one can compute by hand
@pytest.mark.parametrize("v", [0, 93, 255])
@pytest.mark.parametrize("shape,c", [((8, 8), 2.0), ((16, 24), 5.0), ((40, 40), 40.0), ((7, 5), 0.5), ((512, 512), 0.5),
                                     ((512, 512), 1000.0)], ids=str)
def test_constant_tile(shape, c, v):
    """One bin holds the whole tile: everything above clip is spread, a batch to every bin and the residual one by one."""
    area = shape[0] * shape[1]
    lut, d = R.tile_lut(np.full(shape, v, np.int64), c)
    clip = max(int(c * area / 256), 1)
    clip = min(clip, area)
    assert d["clip"] == clip and d["clipped"] == area - clip
    batch, residual = divmod(area - clip, 256)
    assert d["residual"] == residual
    step = max(256 // residual, 1) if residual else 0
    assert d["step"] == step
    for i in (0, 1, v - 1, v, v + 1, 100, 254, 255):
        if not 0 <= i <= 255:
            continue
        marks = sum(1 for k in range(residual) if k * step <= i) if residual else 0         # residual bins at or below i
        s = (i + 1) * batch + (clip if i >= v else 0) + marks
        want = int(np.clip(np.rint(np.float32(s) * (np.float32(255) / np.float32(area))), 0, 255))
        assert lut[i] == want, (i, s)
    assert lut[255] == 255


def test_nothing_clipped_is_plain_equalisation():
    rng = np.random.default_rng(1)
    y = rng.integers(0, 256, (33, 31))
    out, luts, diag = R.clahe_plane(y, 1000.0, 1)
    d = diag[0][0]
    assert d["clipped"] == 0 and d["residual"] == 0 and d["clip"] == 33 * 31          # capped at the area
    cdf = np.cumsum(np.bincount(y.reshape(-1), minlength=256))
    want = np.rint(cdf.astype(np.float32) * (np.float32(255) / np.float32(33 * 31))).astype(np.uint8)
    assert np.array_equal(luts[0, 0], want)
    # a single tile: the four LUTs of every pixel are the same one, the weights sum to one
    assert np.array_equal(out, want[y])


def test_ties_round_to_even():
    """A prefix sum of exactly area / 2 gives 127.5, which rounds to 128; 126.5 would round to 126."""
    tile = np.zeros((16, 16), np.int64)
    tile.reshape(-1)[128:] = 200                      # 128 zeros, 128 at 200: s[0..199] = 128 = area / 2
    lut, d = R.tile_lut(tile, 1000.0)
    assert d["clipped"] == 0
    assert np.float32(128) * (np.float32(255) / np.float32(256)) == np.float32(127.5)
    assert lut[0] == 128 and lut[199] == 128 and lut[200] == 255
    assert np.rint(np.float32(126.5)) == 126 and np.rint(np.float32(127.5)) == 128


def test_colour_round_trip_and_clamps():
    g = np.arange(256, dtype=np.uint8)
    gray = np.stack([g, g, g], -1)
    y, cr, cb = R.rgb_to_ycrcb(gray)
    assert np.array_equal(y, g) and (cr == 128).all() and (cb == 128).all()
    assert np.array_equal(R.ycrcb_to_rgb(y, cr, cb), gray)
    y, cr, cb = R.rgb_to_ycrcb(np.array([[255, 0, 0], [0, 0, 255], [0, 255, 0]], np.uint8))
    assert y.tolist() == [76, 29, 150] and cr.tolist() == [255, 107, 21] and cb.tolist() == [85, 255, 43]   # Cr, Cb of pure R, B: clamped
    assert R.ycrcb_to_rgb(np.array([250]), np.array([255]), np.array([128])).tolist() == [[255, 159, 250]]
    assert R.ycrcb_to_rgb(np.array([5]), np.array([0]), np.array([128])).tolist() == [[0, 96, 5]]


def test_extension_rule():
    p = np.arange(48 * 37).reshape(48, 37)
    assert R.extend(p[:, :32], 8) is not None and R.extend(p[:, :32], 8).shape == (48, 32)           # both divisible: as is
    e = R.extend(p, 8)                                                                                 # 48 is divisible: it grows by 8
    assert e.shape == (56, 40)
    assert np.array_equal(e[:48, :37], p)
    assert np.array_equal(e[48:, :37], p[[46, 45, 44, 43, 42, 41, 40, 39]]) and np.array_equal(e[:48, 37:], p[:, [35, 34, 33]])
    assert R.extend(p[:33, :31], 1).shape == (33, 31)                                                  # g = 1 divides everything


@pytest.mark.parametrize("g,c", [(8, 2.0), (4, 40.0), (3, 1.0), (1, 3.0)])
def test_luts_are_monotonic_and_end_in_255(g, c):
    for seed, (h, w) in enumerate(((64, 64), (50, 37), (48, 37), (33, 31))):
        for crop in (R.smooth_crops(100 + seed, 1, h, w)[0], np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)):
            d = R.clahe_full(crop, c, g)
            luts = d["luts"].astype(np.int64)
            assert luts.shape == (g, g, 256)
            assert (np.diff(luts, axis=-1) >= 0).all()
            assert (luts[..., 255] == 255).all()
            assert d["rgb"].shape == crop.shape and d["rgb"].dtype == np.uint8


def test_gpu_inputs_reach_every_branch():
    """A condition on the inputs of tests/test_clahe_gpu.py (clahe_ref.gpu_cases), shown with the reference's diagnostics."""
    seen = set()
    for name, (crops, g, c) in R.gpu_cases().items():
        for crop in crops:
            d = R.clahe_full(crop, c, g)
            e = R.extend(d["y"].astype(np.int64), g)
            area = (e.shape[0] // g) * (e.shape[1] // g)
            for row in d["diag"]:
                for t in row:
                    if t["residual"] == 0:
                        seen.add("residual == 0")
                    elif t["step"] > 1:
                        seen.add("step > 1")
                    else:
                        assert t["step"] == 1 and t["residual"] > 128
                        seen.add("step == 1")
                    if int(c * area / 256) < 1:
                        assert t["clip"] == 1
                        seen.add("clip == 1 through the max")
                    if t["clipped"] > 65535:
                        seen.add("counts past 16 bits")
            if (d["unsaturated"] > 255).any():
                seen.add("saturates above")
            if (d["unsaturated"] < 0).any():
                seen.add("saturates below")
            assert not np.array_equal(d["rgb"], crop), name                         # the step does something everywhere
    assert seen == {"residual == 0", "step > 1", "step == 1", "clip == 1 through the max", "counts past 16 bits",
                    "saturates above", "saturates below"}
    cases = R.gpu_cases()
    assert cases["48x37_g8_view"][0].shape == (3, 48, 37, 3) and 48 % 8 == 0 and 37 % 8 != 0      # the full-g padding quirk
    d = R.clahe_full(cases["primaries_g4"][0][0], *cases["primaries_g4"][2:0:-1])
    assert (d["unsaturated"] > 255).any() and (d["unsaturated"] < 0).any()


# ---- the library and the op
def test_header_signatures_and_exports_agree(native):
    import ctypes
    N = native
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    params = [p.strip() for p in norm(re.search(r"int fcp_clahe_u8\(([^)]*)\)", hdr).group(1)).split(",")]
    assert params == ["const uint8_t* crops", "int f", "int h", "int w", "int grid", "double clip_limit", "uint8_t* luts",
                      "uint8_t* out", "fcp_stream_t stream"]
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "fcp_clahe_u8")
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    assert N.SIGNATURES["fcp_clahe_u8"] == [P, I, I, I, I, D, P, P, P]
    assert "fcp_clahe_u8" in N.EXPORTS
    assert "#define FCP_ABI_VERSION 15" in hdr and N.ABI_VERSION == 15
    doc = norm(hdr[hdr.index("Contrast-limited adaptive histogram equalisation"):hdr.index("int fcp_clahe_u8(")])
    assert "out MAY BE crops" in doc and "the same bytes from run to run" in doc


def test_entry_point_refuses_before_any_device_work(native):
    lib = native.lib()
    ok = dict(f=1, h=64, w=64, grid=8, clip=2.0)
    for change, word in (({"grid": 0}, b"grid"), ({"grid": 17}, b"grid"), ({"grid": -1}, b"grid"), ({"f": -1}, b"bad sizes"),
                         ({"h": 15}, b"2 * grid"), ({"w": 15}, b"2 * grid"), ({"h": 4097}, b"4096"), ({"w": 4097}, b"4096"),
                         ({"f": 65536}, b"65535"), ({"clip": 0.0}, b"clip_limit"), ({"clip": -2.0}, b"clip_limit"),
                         ({"clip": float("nan")}, b"clip_limit"), ({"clip": float("inf")}, b"clip_limit"), ({}, b"null pointer")):
        a = dict(ok, **change)
        rc = lib.fcp_clahe_u8(None, a["f"], a["h"], a["w"], a["grid"], a["clip"], None, None, None)
        assert rc != 0, change
        assert word in lib.fcp_last_error(), (change, lib.fcp_last_error())
    assert lib.fcp_clahe_u8(None, 0, 64, 64, 8, 2.0, None, None, None) == 0               # f == 0: a no-op
    assert lib.fcp_clahe_u8(None, 0, 2, 2, 1, 0.5, None, None, None) == 0


def test_op_is_registered_and_refuses_cpu_tensors(native):
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    assert "clahe" in T.OPS
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcp::clahe", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcp::clahe", "CPU")
    assert str(torch.ops.fcp.clahe.default._schema) == "fcp::clahe(Tensor crops, int grid, float clip_limit) -> Tensor"
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.clahe(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), 8, 2.0)


# ---- Cropper arguments, CLI
def test_checks():
    from face_crop_plus_amd import clahe as C
    assert C.check_clahe(None) is None and C.check_clahe(2) == 2.0 and C.check_clahe(np.float32(0.5)) == 0.5
    assert isinstance(C.check_clahe(2), float)
    for bad in (0, 0.0, -1, float("nan"), float("inf"), -float("inf"), True, "2", (2,), [2.0]):
        with pytest.raises(ValueError, match="clahe"):
            C.check_clahe(bad)
    assert C.check_grid(None) == 8 and C.check_grid(1) == 1 and C.check_grid(16) == 16 and C.check_grid(4.0) == 4
    for bad in (0, 17, -8, 2.5, True, "8", (8,), float("nan")):
        with pytest.raises(ValueError, match="clahe_grid"):
            C.check_grid(bad)
    assert C.check_grid(8, (16, 16)) == 8 and C.check_grid(None, (256, 16)) == 8 and C.check_grid(1, (2, 2)) == 1
    for grid, size in ((8, (15, 64)), (8, (64, 15)), (None, (15, 15)), (16, (31, 31)), (1, (1, 5))):
        with pytest.raises(ValueError, match="output_size"):
            C.check_grid(grid, size)


def test_cropper_checks_clahe_without_a_device(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    params = inspect.signature(Cropper).parameters
    assert [params[k].default for k in ("clahe", "clahe_grid")] == [None, None]
    for bad in (0, -2.0, float("nan"), float("inf"), True, "2"):
        with pytest.raises(ValueError, match="clahe"):
            Cropper(clahe=bad)
    for bad in (0, 17, 2.5, "8"):
        with pytest.raises(ValueError, match="clahe_grid"):
            Cropper(clahe=2.0, clahe_grid=bad)
    with pytest.raises(ValueError, match="needs clahe"):
        Cropper(clahe_grid=8)
    with pytest.raises(ValueError, match="output_size"):
        Cropper(clahe=2.0, output_size=15)
    with pytest.raises(ValueError, match="output_size"):
        Cropper(clahe=2.0, clahe_grid=16, output_size=(64, 31))
    with pytest.raises(ValueError, match="no alignment"):
        Cropper(clahe=2.0, det_threshold=None, landmarks=None)
    given = {"det_threshold": None, "landmarks": (np.zeros((1, 5, 2)), np.array(["a"]))}
    for kw in ({"clahe": 2.0}, {"clahe": 2, "clahe_grid": 4}, {"clahe": 0.01, "clahe_grid": 16, "output_size": 32},
               {"clahe": 40.0, "clahe_grid": 1, "output_size": (2, 2), **given}):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(**kw)


def test_cropper_resolves_the_defaults(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    c = Cropper(clahe=2)
    assert (c.clahe, c.clahe_grid) == (2.0, 8)
    c = Cropper(clahe=3.5, clahe_grid=4)
    assert (c.clahe, c.clahe_grid) == (3.5, 4)
    c = Cropper()
    assert (c.clahe, c.clahe_grid) == (None, None)
    with pytest.raises(ValueError, match="clahe"):
        c.equalize(np.zeros((1, 16, 16, 3), np.uint8))


def test_cli_flags(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    plain = parse_args(base)
    assert not {"clahe", "clahe_grid"} & set(plain)
    got = parse_args(base + ["-cl", "2", "-cg", "4"])
    assert got["clahe"] == 2.0 and got["clahe_grid"] == 4
    assert {k: v for k, v in got.items() if k not in ("clahe", "clahe_grid")} == plain           # nothing else moves
    got = parse_args(base + ["--clahe", "0.5"])
    assert got["clahe"] == 0.5 and "clahe_grid" not in got
    assert parse_args(base + ["--clahe", "3", "--clahe-grid", "16"])["clahe_grid"] == 16
    for bad in (["-cl", "strong"], ["-cg", "2.5"], ["-cg", "many"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
