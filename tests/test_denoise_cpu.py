"""Cropper(denoise=H) without a GPU: the reference tests/denoise_ref.py against the plain loops of its definition, the
host's weight table against the reference's own, the table's properties, the argument checks of denoise.py and of the
Cropper, the CLI flag, the header, exports and op schema, the C export's refusals, and what the filter is for: the noise it
removes from a synthetic scene."""
import ctypes
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(os.path.dirname(__file__), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("denoise_ref")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    return N


# ---- the reference
def test_reference_equals_the_plain_loops():
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:14, 0:15]
    crop = np.clip(np.stack([8 * x + 20, 9 * y + 30, 100 + 3 * x - 2 * y], -1) + rng.integers(-6, 7, (14, 15, 3)), 0, 255).astype(np.uint8)
    mixed = rng.integers(0, 65536, 300).astype(np.uint16)               # any table: not monotone, entries above ONE, zeros
    mixed[::7] = 0
    for lut, shift in (R.weight_lut(4), (mixed, 2)):
        want = R.nlm_loops(crop, lut, shift)
        got = R.nlm_one(crop, lut, shift)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        assert not np.array_equal(got, crop)
    assert np.array_equal(R.nlm(crop[None], *R.weight_lut(4))[0], R.nlm_one(crop, *R.weight_lut(4)))
    assert R.nlm(crop[None][:0], mixed, 0).shape == (0, 14, 15, 3)
    assert np.array_equal(R.nlm_one(crop, np.zeros(5, np.uint16), 0), crop)          # W == 0: the pixel is copied


# ---- the table
def test_weight_lut_equals_the_reference_table():
    from face_crop_plus_amd import denoise as D
    assert (D.PATCH_RADIUS, D.SEARCH_RADIUS, D.ONE, D.MIN_SIDE, D.MAX_LUT) == (R.P, R.S, R.ONE, R.MIN_SIDE, R.MAX_LUT) == (3, 10, 4096, 14, 4096)
    for strength in np.arange(1, 32.25, 0.25):
        lut, shift = D.weight_lut(float(strength))
        want, want_shift = R.weight_lut(float(strength))
        assert lut.dtype == np.uint16 and shift == want_shift and np.array_equal(lut, want), strength


def test_table_properties():
    from face_crop_plus_amd import denoise as D
    for strength in list(np.arange(1, 32.25, 0.25)) + [1, 32, np.float32(7.5), np.int64(3)]:
        lut, shift = D.weight_lut(strength)
        cut = int(np.floor(np.log(2.0 * 4096) * 49.0 * float(strength) ** 2))
        assert 0 <= shift <= 10 and 1 <= len(lut) <= 4096 and len(lut) == (cut >> shift) + 1
        assert shift == 0 or (cut >> (shift - 1)) >= 4096                       # the smallest shift
        assert lut[0] == 4096 and lut.min() >= 1 and (np.diff(lut.astype(np.int64)) <= 0).all(), strength
    for strength, (n, shift) in R.TABLE.items():
        lut, s = D.weight_lut(strength)
        assert (len(lut), s) == (n, shift), strength


# ---- argument checks
def test_check_denoise():
    from face_crop_plus_amd import denoise as D
    assert D.check_denoise(None) is None
    for good, want in ((1, 1.0), (32, 32.0), (8.5, 8.5), (np.float32(2.5), 2.5), (np.int64(12), 12.0)):
        got = D.check_denoise(good)
        assert got == want and type(got) is float, good
    for bad in (True, False, np.bool_(True), "8", "strong", 0.99, 32.5, 0, -8, float("nan"), float("inf"), -float("inf"), (8,), [8.0]):
        with pytest.raises(ValueError, match="denoise must be"):
            D.check_denoise(bad)
    D.check_size((14, 14))
    D.check_size((256,))
    for size in ((13,), (13, 64), (64, 13), (1, 1)):
        with pytest.raises(ValueError, match="output_size of at least 14 x 14"):
            D.check_size(size)
    assert list(inspect.signature(D.nlm).parameters) == ["crops_dev", "lut_dev", "shift"]
    assert list(inspect.signature(D.denoise).parameters) == ["crops_dev", "strength"]
    for text in ("denoise=H", "fcp_nlm_denoise_u8", "torch.ops.fcp.nlm_denoise", "chroma noise is reduced less", "section 2p"):
        assert text in D.__doc__, text


def test_cropper_checks_denoise_without_a_device(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    params = inspect.signature(Cropper).parameters
    names = list(params)
    assert params["denoise"].default is None
    assert names[names.index("edge_shift") + 1] == "denoise" and names[names.index("denoise") + 1] == "clahe"
    assert names[names.index("decontaminate") + 1] == "edge_shift" and names[-2:] == ["interpolation", "min_sharpness"]
    for bad in (True, "8", 0.99, 32.5, 0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="denoise must be"):
            Cropper(denoise=bad)
    with pytest.raises(ValueError, match="denoise needs aligned crops.*no alignment"):
        Cropper(denoise=8, det_threshold=None, landmarks=None)
    for size in (13, (13, 64), (64, 13)):
        with pytest.raises(ValueError, match="denoise needs an output_size of at least 14 x 14"):
            Cropper(denoise=8, output_size=size)
    given = {"det_threshold": None, "landmarks": (np.zeros((1, 5, 2)), np.array(["a"]))}
    for kw in ({"denoise": 8}, {"denoise": 1, "output_size": 14}, {"denoise": 32.0, "output_size": (14, 40), **given},
               {"denoise": np.float32(2.5), "clahe": 2.0, "background": 0, "refine": 4, "min_sharpness": 5.0}):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(**kw)


def test_cropper_resolves_the_default_and_remove_noise_needs_denoise(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    c = Cropper(denoise=8)
    assert c.denoise == 8.0 and type(c.denoise) is float and c.clahe is None
    c = Cropper()
    assert c.denoise is None
    with pytest.raises(ValueError, match="Cropper.remove_noise needs a Cropper with denoise"):
        c.remove_noise(np.zeros((1, 16, 16, 3), np.uint8))
    for bad in (np.zeros((1, 16, 16, 3), np.float32), np.zeros((16, 16, 3), np.uint8), np.zeros((1, 16, 16, 4), np.uint8)):
        with pytest.raises(ValueError, match="crops must be"):
            Cropper(denoise=8).remove_noise(bad)
    assert Cropper(denoise=8).remove_noise(np.zeros((0, 16, 16, 3), np.uint8)).shape == (0, 16, 16, 3)
    doc = Cropper.__init__.__doc__
    assert "``denoise``" in doc and "denoise.denoise" in doc and "section 2p" in doc and "chroma noise is reduced less" in doc


def test_cli_flag(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    plain = parse_args(base)
    assert "denoise" not in plain
    got = parse_args(base + ["-dn", "8"])
    assert got["denoise"] == 8.0 and type(got["denoise"]) is float
    assert {k: v for k, v in got.items() if k != "denoise"} == plain                     # nothing else moves
    assert parse_args(base + ["--denoise", "2.5"])["denoise"] == 2.5
    got = parse_args(base + ["-dn", "12", "-cl", "2"])
    assert (got["denoise"], got["clahe"]) == (12.0, 2.0)
    for bad in (["-dn", "strong"], ["-dn"], ["--denoise", "8px"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)


# ---- the library and the op
def test_header_signatures_and_exports_agree(native):
    N = native
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    norm = lambda s: re.sub(r"[\s*]+", " ", s).strip()
    params = [re.sub(r"\s+", " ", p).strip() for p in re.search(r"int fcp_nlm_denoise_u8\(([^)]*)\)", hdr).group(1).split(",")]
    assert params == ["const uint8_t* crops", "int f", "int h", "int w", "const uint16_t* lut", "int lut_len", "int shift",
                      "uint8_t* out", "fcp_stream_t stream"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert N.SIGNATURES["fcp_nlm_denoise_u8"] == [P, I, I, I, P, I, I, P, P]
    assert "fcp_nlm_denoise_u8" in N.EXPORTS and hasattr(N.lib(), "fcp_nlm_denoise_u8")
    assert "#define FCP_ABI_VERSION 15" in hdr and N.ABI_VERSION == 15 and N.lib().fcp_abi_version() == 15
    doc = norm(hdr[hdr.index("Non-local-means noise removal"):hdr.index("int fcp_nlm_denoise_u8(")])
    for phrase in ("min(lut[k], ONE)", "W == 0 copies the pixel", "no workspace, no float and no atomics", "must not overlap",
                   "out == crops included", 'a "nlm_denoise:" message'):
        assert phrase in doc, phrase
    src = open(os.path.join(ROOT, "face-crop-plus_amd", "csrc", "fcp_nlm.hip")).read()
    assert '#include "fcp_gray.h"' in src and "9798u" not in src                    # the gray is shared, not copied
    assert "9798u * r + 19235u * g + 3735u * b + 16384u) >> 15" in open(os.path.join(ROOT, "face-crop-plus_amd", "csrc", "fcp_gray.h")).read()


def test_entry_point_refuses_before_any_device_work(native):
    """Null pointers everywhere: a call that got past its checks would fault, a refused one returns with its message."""
    lib = native.lib()
    ok = dict(f=1, h=64, w=64, n=100, shift=0)

    def call(crops=None, lut=None, out=None, **change):
        a = dict(ok, **change)
        return lib.fcp_nlm_denoise_u8(crops, a["f"], a["h"], a["w"], lut, a["n"], a["shift"], out, None)
    for change, word in (({"f": -1}, b"bad sizes"), ({"h": 0}, b"bad sizes"), ({"w": -3}, b"bad sizes"), ({"h": 8193}, b"8192"),
                         ({"w": 8193}, b"8192"), ({"f": 65536}, b"65535"), ({"h": 13}, b"at least 14 x 14"),
                         ({"w": 13}, b"at least 14 x 14"), ({"n": 0}, b"lut_len must be 1..4096"), ({"n": 4097}, b"lut_len must be 1..4096"),
                         ({"n": -1}, b"lut_len"), ({"shift": -1}, b"shift must be 0..10"), ({"shift": 11}, b"shift must be 0..10"),
                         ({}, b"null pointer"), ({"h": 14, "w": 14, "n": 1, "shift": 10}, b"null pointer"),
                         ({"n": 4096}, b"null pointer")):
        assert call(**change) == -1, change
        assert word in lib.fcp_last_error() and lib.fcp_last_error().startswith(b"nlm_denoise:"), (change, lib.fcp_last_error())
    one, two, far = ctypes.c_void_p(4096), ctypes.c_void_p(4098), ctypes.c_void_p(1 << 20)      # never dereferenced
    for kw in ({"crops": one}, {"lut": one}, {"out": one}, {"crops": one, "lut": two}, {"lut": two, "out": one}, {"crops": one, "out": far}):
        assert call(**kw) == -1 and b"null pointer" in lib.fcp_last_error(), kw
    for kw in ({"crops": one, "out": one}, {"crops": one, "out": two}, {"crops": two, "out": one},
               {"crops": one, "out": ctypes.c_void_p(4096 + 64 * 64 * 3 - 1)}):
        assert call(lut=far, **kw) == -1, kw
        assert b"must not overlap" in lib.fcp_last_error() and lib.fcp_last_error().startswith(b"nlm_denoise:"), lib.fcp_last_error()
    assert call(crops=one, out=far, lut=ctypes.c_void_p(4097)) == -1 and b"2-byte aligned" in lib.fcp_last_error()
    assert call(f=0) == 0 and call(f=0, h=14, w=8192, n=4096, shift=10) == 0           # f == 0: a no-op
    assert call(f=0, h=13) == -1 and call(f=0, n=0) == -1 and call(f=0, shift=11) == -1   # the checks come before the no-op


def test_op_is_registered_and_refuses_cpu_tensors(native):
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    assert "nlm_denoise" in T.OPS and hasattr(ops, "nlm_denoise")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcp::nlm_denoise", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcp::nlm_denoise", "CPU")
    assert str(ops.nlm_denoise.default._schema) == "fcp::nlm_denoise(Tensor crops, Tensor lut, int shift) -> Tensor"
    with pytest.raises((NotImplementedError, RuntimeError)):                # no CPU kernel: a missing device is an error
        ops.nlm_denoise(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint16), 0)


# ---- what it is for
def test_the_reference_removes_the_noise_of_a_synthetic_scene():
    """Gaussian noise of sigma 10 on a 96 x 80 scene of gradients, an ellipse and a checkered band, H = 8: the mean
    squared error against the clean scene must at least halve (3.01 dB).  Measured: 28.2 dB before, 33.9 dB after, a factor of 3.7."""
    clean = R.scene()
    assert clean.shape == (96, 80, 3)
    noisy = R.noisy(clean, 10.0, 0)
    out = R.denoise(noisy[None], 8)[0]
    before, after = R.psnr(noisy, clean), R.psnr(out, clean)
    print(f"PSNR against the clean scene: {before:.1f} dB noisy, {after:.1f} dB denoised")
    mse = lambda a: np.mean((a.astype(np.float64) - clean.astype(np.float64)) ** 2)
    assert mse(out) <= mse(noisy) / 2
    sentence = f"from {before:.1f} dB to {after:.1f} dB"
    readme = re.sub(r"\s+", " ", open(os.path.join(ROOT, "README.md")).read())
    assert sentence in readme, sentence


def test_docs_say_what_it_is():
    readme = re.sub(r"\s+", " ", open(os.path.join(ROOT, "README.md")).read())
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`Cropper(denoise=H)` / `-dn H`" in readme and "INTEGRATION.md section 2p" in readme
    assert integration.index("## 2o.") < integration.index("## 2p.") < integration.index("## 3.")
    section = re.sub(r"\s+", " ", integration[integration.index("## 2p."):integration.index("## 3.")])
    for phrase in ("`-dn H` / `--denoise H`", "BORDER_REFLECT_101", "min(lut[k], ONE)", "floor(ln(2 ONE) 49 H^2)", "fcp_nlm_denoise_u8",
                   "torch.ops.fcp.nlm_denoise", "denoise.weight_lut", "tests/denoise_ref.py", "One launch", "no workspace",
                   "chroma noise is reduced less", "The ABI version stays 15", "tools/bench_denoise.py", "64 crops of 256 x 256"):
        assert phrase in section, phrase
    assert "bench_denoise.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
