"""Cropper(background="transparent") / Cropper(decontaminate=...) without a GPU: the properties of the reference
tests/cutout_ref.py and its quality on a synthetic scene, the argument checks, the CLI flags, the C exports, the ops and
the RGBA side of the PNG encoder's host code.

The reference's own tests (its taps, window sums, properties, 32-bit bounds and the quality condition) are pinned to
tests/cutout_ref.py alone and need nothing of the package but ``blur_taps``; every other test fails without the feature:
the keywords, the CLI flags, the exports, the ops and ``png_file_rgba`` do not exist there."""
import importlib.util
import inspect
import io
import json
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


R = _load("cutout_ref")
P = _load("png_ref")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    return N


def _taps(sigma):
    from face_crop_plus_amd import matte as M
    return M.blur_taps(sigma)


# ---- the reference
def test_reference_taps_are_the_package_s():
    for sigma in (0.5, 1, 2, 4, 8, 16):
        assert _taps(sigma) == R.BR.blur_taps(sigma)
    assert [len(_taps(s)) - 1 for s in R.SIGMAS] == [3, 12, 48]


def test_shape_list_crosses_the_kernel_s_tiles():
    """The shapes of the GPU tests come from the tile constants of csrc/fcp_cutout.hip and, for the rows pass it shares
    with the background blur, of csrc/fcp_masked_blur.h: more than one tile each way."""
    csrc = os.path.join(ROOT, "face-crop-plus_amd", "csrc")
    src = open(os.path.join(csrc, "fcp_masked_blur.h")).read() + open(os.path.join(csrc, "fcp_cutout.hip")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert (R.ROW_W, R.ROW_H, R.COL_W, R.COL_H) == (const("kRowTileW"), const("kRowTileH"), const("kTileW"), const("kTileH"))
    assert any(w > R.ROW_W for _, w in R.SHAPES) and any(h > R.ROW_H for h, _ in R.SHAPES)
    tall = [(h, w) for h, w in R.SHAPES if h > R.COL_H]
    assert len(tall) >= 3 and any(h > 2 * R.COL_H for h, _ in tall) and any(h % R.COL_H == 2 for h, _ in tall)
    assert any(h > R.COL_H + 48 for h, _ in tall)               # a full margin of r = 48 from the tile above
    assert (R.COL_H, R.COL_W) in R.SHAPES and all(s in R.SHAPES for s in [(8, 300), (70, 20), (96, 80), (1, 1)])


def test_window_sums_equal_the_two_dimensional_definition():
    rng = np.random.default_rng(2)
    for (h, w), sigma in (((1, 1), 0.5), ((5, 6), 4), ((17, 9), 16), ((9, 30), 2)):
        planes = rng.integers(0, 256, (2, h, w, 4))
        assert np.array_equal(R.window_sums(planes, _taps(sigma)), R.BR.window_sums(planes, _taps(sigma))), (h, w, sigma)


def test_opaque_alpha_keeps_the_crop_and_empty_alpha_ships_nothing():
    rng = np.random.default_rng(5)
    crops = R.MR.random_crops(rng, 2, 13, 17)
    ones, zeros = np.full((2, 13, 17), 255, np.uint8), np.zeros((2, 13, 17), np.uint8)
    for taps in (None, _taps(0.5), _taps(4)):
        assert np.array_equal(R.foreground(crops, ones, taps), crops)
        out = R.rgba(crops, ones, taps)
        assert out.shape == (2, 13, 17, 4) and np.array_equal(out[..., :3], crops) and (out[..., 3] == 255).all()
        assert not R.rgba(crops, zeros, taps).any()
    assert np.array_equal(R.fill(crops, ones, _taps(4), (1, 2, 3)), crops)
    assert (R.fill(crops, zeros, _taps(4), (1, 2, 3)) == np.array([1, 2, 3], np.uint8)).all()
    # hidden colours are zeroed pixel by pixel, shown ones keep theirs
    alpha = rng.integers(0, 3, (2, 13, 17)).astype(np.uint8) * 127         # 0, 127, 254
    out = R.rgba(crops, alpha)
    assert not out[alpha == 0].any() and np.array_equal(out[alpha > 0][:, :3], crops[alpha > 0])
    assert np.array_equal(out[..., 3], alpha)
    # the estimate without a certain pixel of either kind in reach: the crop's colour stands
    assert np.array_equal(R.foreground(crops, np.full((2, 13, 17), 128, np.uint8), _taps(4)), crops)


def test_exact_composite_of_constant_colours_is_recovered_within_one_level():
    h, w = 40, 36
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    al = np.clip((1 - np.sqrt((yy - 20) ** 2 / 12.0 ** 2 + (xx - 18) ** 2 / 10.0 ** 2)) * 3 + 0.5, 0, 1)
    a = np.round(255 * al).astype(np.int64)
    fg, bg = np.array([200, 60, 50], np.int64), np.array([20, 210, 130], np.int64)
    # composed exactly, in the integers of the definition: 255 c = a F + (255 - a) B up to the rounding of c
    c = ((a[..., None] * fg + (255 - a[..., None]) * bg + 127) // 255).astype(np.uint8)
    a = a.astype(np.uint8)
    for sigma in (2, 4):
        taps = _taps(sigma)
        fh, bh, df, db = R.estimates(c[None], a[None], taps)
        e = R.corrected(c[None], a[None], fh, bh)[0]
        both = (df[0] > 0) & (db[0] > 0) & (a > 0) & (a < 255)
        assert both.sum() > 100
        assert np.abs(e[both] - fg).max() <= 1, sigma
        assert np.array_equal(R.foreground(c[None], a[None], taps)[0][both], e[both].astype(np.uint8))


@pytest.mark.parametrize("sigma", [0.5, 4, 16])
def test_sums_stay_below_32_bits(sigma):
    taps = _taps(sigma)
    r = len(taps) - 1
    white = np.full((1, 2 * r + 3, 2 * r + 5, 3), 255, np.uint8)
    for s in (np.ones(white.shape[:3], bool), np.zeros(white.shape[:3], bool)):
        est, d, peak = R.side_estimate(white, s, taps)
        assert peak < 2 ** 32 and d.max() <= 4096 ** 2
    est, d, peak = R.side_estimate(white, np.ones(white.shape[:3], bool), taps)
    assert peak == 255 * 4096 ** 2 + 4096 ** 2 // 2 == 4286578688 and (est == 255).all()


def test_reference_quality_on_the_synthetic_scene():
    """The estimate's own condition, on the reference alone: at sigma 4 its mean absolute error against the true subject
    colour over the soft pixels is at most a quarter of the crop's own (measured: 4.30 against 60.56)."""
    c, a, true = R.scene()
    assert c.shape == (96, 80, 3) and a.shape == (96, 80)
    soft = (a > 0) & (a < 255)
    assert soft.sum() == 744
    own = np.abs(c.astype(np.float64) - true)[soft].mean()
    est = np.abs(R.foreground(c[None], a[None], _taps(4))[0].astype(np.float64) - true)[soft].mean()
    print("crop's own", own, "estimate", est, "ratio", est / own)
    assert est <= own / 4


# ---- the host side of the RGBA PNG
def test_png_file_rgba_decodes_to_the_array_the_stream_was_made_from():
    from PIL import Image
    from face_crop_plus_amd import pngenc
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (17, 9, 4), dtype=np.uint8)
    img[rng.integers(0, 2, (17, 9)) == 0] = 0                     # cut-out like: runs of zero pixels
    file = pngenc.png_file_rgba(17, 9, P.encode_stream(img))
    assert file[:8] == b"\x89PNG\r\n\x1a\n" and file[25] == 6     # IHDR colour type
    got = Image.open(io.BytesIO(file))
    assert got.mode == "RGBA" and np.array_equal(np.asarray(got), img)
    with pytest.raises(ValueError, match="px"):
        pngenc.png_file_rgba(0, 9, b"")
    # the three-channel functions answer as before
    with pytest.raises(ValueError, match="channels"):
        pngenc.png_file(17, 9, 4, b"")
    assert not pngenc.supported(8, 8, 4)
    # the host fallback writes RGBA too
    host = Image.open(io.BytesIO(pngenc._host_png(img)))
    assert host.mode == "RGBA" and np.array_equal(np.asarray(host), img)


def test_supported_rgba_at_its_bound():
    from face_crop_plus_amd import pngenc
    assert pngenc.supported_rgba(1500, 1500) and not pngenc.supported_rgba(1520, 1520)
    assert pngenc.supported_rgba(1, 1) and pngenc.supported_rgba(8192, 281) and not pngenc.supported_rgba(8192, 282)
    assert not pngenc.supported_rgba(8193, 1) and not pngenc.supported_rgba(1, 8193) and not pngenc.supported_rgba(0, 8)
    # the bound itself: h * (4 w + 1) + 1 < 9227464
    assert 8192 * (4 * 281 + 1) + 1 < pngenc.MAX_SYMBOLS <= 8192 * (4 * 282 + 1) + 1


# ---- the library and the ops
def test_header_signatures_and_exports_agree(native):
    import ctypes
    N = native
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    params = lambda name: [p.strip() for p in norm(re.search(r"int(?:64_t)? %s\(([^)]*)\)" % name, hdr).group(1)).split(",")]
    assert params("fcp_feather_alpha_u8") == ["const uint8_t* labels", "int f", "int h", "int w", "uint32_t class_bits", "int feather",
                                              "uint8_t* alpha_out", "fcp_stream_t stream"]
    assert params("fcp_cutout_u8") == ["const uint8_t* crops", "const uint8_t* alpha", "int f", "int h", "int w", "int mode",
                                       "int bg_r", "int bg_g", "int bg_b", "const uint16_t* taps", "int radius", "uint8_t* out",
                                       "void* workspace", "int64_t workspace_bytes", "fcp_stream_t stream"]
    assert params("fcp_cutout_workspace_bytes") == ["int f", "int h", "int w"]
    Pt, I, U, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_int64
    assert N.SIGNATURES["fcp_feather_alpha_u8"] == [Pt, I, I, I, U, I, Pt, Pt]
    assert N.SIGNATURES["fcp_cutout_u8"] == [Pt, Pt, I, I, I, I, I, I, I, Pt, I, Pt, Pt, L, Pt]
    lib = N.lib()
    for name in ("fcp_feather_alpha_u8", "fcp_cutout_u8", "fcp_cutout_workspace_bytes"):
        assert name in N.EXPORTS and hasattr(lib, name)
    assert "#define FCP_ABI_VERSION 15" in hdr and N.ABI_VERSION == 15 and lib.fcp_abi_version() == 15
    assert "#define FCP_CUTOUT_RGBA 0" in hdr and "#define FCP_CUTOUT_FILL 1" in hdr
    from face_crop_plus_amd import matte as M
    assert (M.CUTOUT_RGBA, M.CUTOUT_FILL) == (0, 1) == (R.RGBA, R.FILL)
    assert lib.fcp_cutout_workspace_bytes(3, 5, 7) == 32 * 3 * 5 * 7 and lib.fcp_cutout_workspace_bytes(0, 5, 7) == 0
    for bad in ((-1, 4, 4), (1, 0, 4), (1, 4, 8193), (65536, 4, 4)):
        assert lib.fcp_cutout_workspace_bytes(*bad) == -1
    # four channels for the PNG encoder, two still refused
    assert lib.fcp_png_workspace_bytes(1, 8, 8, 4) > lib.fcp_png_workspace_bytes(1, 8, 8, 3) > 0
    assert lib.fcp_png_workspace_bytes(1, 8, 8, 2) == -1 and b"channels" in lib.fcp_last_error()
    assert lib.fcp_png_workspace_bytes(1, 1500, 1500, 4) > 0 and lib.fcp_png_workspace_bytes(1, 1520, 1520, 4) == -1


def test_entry_points_refuse_before_any_device_work(native):
    """Null pointers everywhere: a call that got past its checks would fault, a refused one returns with its message."""
    import ctypes
    lib = native.lib()
    taps = _taps(4)
    t16 = (ctypes.c_uint16 * 49)(*taps)
    ok = dict(f=1, h=4, w=4, mode=0, r=0, g=0, b=0, taps=t16, radius=len(taps) - 1, ws=None, wsb=0)

    def call(**change):
        a = dict(ok, **change)
        return lib.fcp_cutout_u8(None, None, a["f"], a["h"], a["w"], a["mode"], a["r"], a["g"], a["b"], a["taps"], a["radius"], None,
                                 a["ws"], a["wsb"], None)
    short = (ctypes.c_uint16 * 49)(*([taps[0] - 2] + taps[1:]))
    zero = (ctypes.c_uint16 * 49)(*([taps[0] + 2 * taps[-1]] + taps[1:-1] + [0]))
    for change, word in (({"f": -1}, b"bad sizes"), ({"h": 0}, b"bad sizes"), ({"w": 0}, b"bad sizes"), ({"h": 8193}, b"8192"),
                         ({"w": 8193}, b"8192"), ({"f": 65536}, b"65535"), ({"mode": 2}, b"mode"), ({"mode": -1}, b"mode"),
                         ({"radius": 1}, b"radius"), ({"radius": 2}, b"radius"), ({"radius": 49}, b"radius"),
                         ({"radius": -3}, b"radius"), ({"mode": 1, "radius": 0}, b"fcp_matte_alpha_u8"),
                         ({"r": 256}, b"fill"), ({"g": -1}, b"fill"), ({"taps": None}, b"null taps"),
                         ({"taps": short}, b"sum to 4096"), ({"taps": zero}, b"at least 1"),
                         ({"radius": 11}, b"sum to 4096"), ({}, b"null pointer"), ({"radius": 0}, b"null pointer")):
        assert call(**change) < 0, change
        assert word in lib.fcp_last_error(), (change, lib.fcp_last_error())
    assert call(f=0) == 0 and call(f=0, radius=0, taps=None) == 0                  # f == 0: a no-op
    bits = R.MR.DEFAULT_BITS
    ok = dict(f=1, h=4, w=4, bits=bits, feather=5)
    for change, word in (({"f": -1}, b"bad sizes"), ({"h": 0}, b"bad sizes"), ({"w": 8193}, b"8192"), ({"f": 65536}, b"65535"),
                         ({"feather": 4}, b"feather"), ({"feather": 9}, b"feather"), ({"bits": 1 << 19}, b"class_bits"),
                         ({}, b"null pointer")):
        a = dict(ok, **change)
        assert lib.fcp_feather_alpha_u8(None, a["f"], a["h"], a["w"], a["bits"], a["feather"], None, None) < 0, change
        assert word in lib.fcp_last_error() and b"feather_alpha" in lib.fcp_last_error(), (change, lib.fcp_last_error())
    assert lib.fcp_feather_alpha_u8(None, 0, 4, 4, bits, 5, None, None) == 0


def test_ops_are_registered_and_refuse_cpu_tensors(native):
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    assert "feather_alpha" in T.OPS and "cutout" in T.OPS
    for name in ("fcp::feather_alpha", "fcp::cutout"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(name, "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(name, "CPU")
    assert str(torch.ops.fcp.feather_alpha.default._schema) == "fcp::feather_alpha(Tensor labels, int class_bits, int feather) -> Tensor"
    assert str(torch.ops.fcp.cutout.default._schema) == ("fcp::cutout(Tensor crops, Tensor alpha, int mode, int bg_r, int bg_g, "
                                                         "int bg_b, int[] taps) -> Tensor")
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.feather_alpha(torch.zeros(1, 8, 8, dtype=torch.uint8), 2, 5)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.cutout(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8), 0, 0, 0, 0, [])


# ---- Cropper arguments, CLI
def test_cropper_checks_the_new_arguments_without_a_device(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    from face_crop_plus_amd import matte as M

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    params = inspect.signature(Cropper).parameters
    assert [params[k].default for k in ("background", "decontaminate")] == [None, None]
    assert M.TRANSPARENT == "transparent" and M.check_background("transparent") is M.TRANSPARENT
    assert M.check_decontaminate(None) is None and M.check_decontaminate(4) == 4.0 and isinstance(M.check_decontaminate(4), float)
    # "transparent" needs PNG, named in the message, at construction
    for fmt in (None, "jpg", "bmp", "webp", "tiff", "PNG8", 5):
        with pytest.raises(ValueError, match="png"):
            Cropper(background="transparent", output_format=fmt)
    for other in ("Transparent", "clear", "none", b"transparent"):
        with pytest.raises(ValueError, match="background"):
            Cropper(background=other, output_format="png")
    with pytest.raises(ValueError, match="background_blur"):
        Cropper(background="transparent", output_format="png", background_blur=4)
    with pytest.raises(ValueError, match="no alignment"):
        Cropper(background="transparent", output_format="png", det_threshold=None, landmarks=None)
    # decontaminate: the range of background_blur, no bool
    for bad in (True, False, 0, 0.49, 16.5, -1, float("nan"), float("inf"), "4", (4,), [4]):
        with pytest.raises(ValueError, match="decontaminate"):
            Cropper(background=0, decontaminate=bad)
    with pytest.raises(ValueError, match="decontaminate needs background"):
        Cropper(decontaminate=4)
    with pytest.raises(ValueError, match="decontaminate and background_blur"):
        Cropper(background_blur=4, decontaminate=4)
    # valid values get past the argument checks (and only then reach the models)
    for kw in ({"background": "transparent", "output_format": "png"}, {"background": "transparent", "output_format": "PNG"},
               {"background": "transparent", "output_format": "Png", "decontaminate": 4, "refine": 4, "subject": "largest",
                "fill_holes": 50, "foreground": [1, 17]},
               {"background": "transparent", "output_format": "png", "feather": 7, "decontaminate": 0.5},
               {"background": (0, 177, 64), "decontaminate": 16}, {"background": 7, "decontaminate": np.float32(2.5), "feather": 0},
               {"background": 0, "decontaminate": 3, "output_format": "jpg"}):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(**kw)


def test_cropper_resolves_the_new_defaults(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    from face_crop_plus_amd import matte as M
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    c = Cropper()
    assert (c.background, c.decontaminate, c.decontaminate_taps) == (None, None, None)
    c = Cropper(background=9)
    assert (c.background, c.decontaminate, c.decontaminate_taps, c.feather) == ((9, 9, 9), None, None, 5)
    c = Cropper(background="transparent", output_format="png")
    assert c.background is M.TRANSPARENT and c.decontaminate is None and c.feather == 5
    assert c.foreground == tuple(range(1, 19))
    c = Cropper(background="transparent", output_format="PNG", decontaminate=4, refine=3)
    assert c.decontaminate == 4.0 and c.decontaminate_taps == M.blur_taps(4) and c.feather == 0 and c.refine == 3
    assert c._is_png_target(np.array(["a.jpg", "b.bmp"])).all()
    c = Cropper(background=(1, 2, 3), decontaminate=0.5)
    assert c.decontaminate_taps == M.blur_taps(0.5) and len(c.decontaminate_taps) == 4
    with pytest.raises(ValueError, match=r"\(F,H,W,4\)"):
        c.encode_png(np.zeros((1, 4, 4, 2), np.uint8))


def test_transparent_alone_creates_the_parser(monkeypatch):
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
    c = Cropper(background="transparent", output_format="png", device="cuda:0", weights={"bisenet": "generated"},
                det_threshold=None, landmarks=(np.zeros((1, 5, 2), np.float32), np.array(["a"])))
    assert isinstance(c.par_model, Parser) and made == [(None, None), "generated"]


def test_cli_flags(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    plain = parse_args(base)
    assert not {"background", "decontaminate"} & set(plain)
    got = parse_args(base + ["-bg", "transparent", "-f", "png"])
    assert got["background"] == "transparent" and got["output_format"] == "png"
    assert parse_args(base + ["--background", "transparent"])["background"] == "transparent"
    assert parse_args(base + ["-bg", "0", "-dc", "4"])["decontaminate"] == 4.0
    assert parse_args(base + ["-bg", "1,2,3", "--decontaminate", "0.5"])["decontaminate"] == 0.5
    got = parse_args(base + ["-dc", "2"])
    assert {k: v for k, v in got.items() if k != "decontaminate"} == plain          # nothing else moves
    assert parse_args(base + ["-bg", "12,34,56"])["background"] == [12, 34, 56]
    for bad in (["-bg", "red"], ["-bg", "Transparent"], ["-dc", "wide"], ["-dc"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"background": "transparent", "output_format": "png", "decontaminate": 8}))
    got = parse_args(base + ["-c", str(cfg)])
    assert got["background"] == "transparent" and got["decontaminate"] == 8 and got["output_format"] == "png"


def test_docs_say_what_the_estimate_weighs():
    readme = open(os.path.join(ROOT, "README.md")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert 'background="transparent"' in readme and "decontaminate" in readme
    section = re.sub(r"\s+", " ", integration[integration.index("## 2n."):integration.index("## 3.")])   # line breaks aside
    for phrase in ("exactly 255", "exactly 0", "the crop's colour stands", "width of the soft edge", "fcp_cutout_u8",
                   "fcp_feather_alpha_u8"):
        assert phrase in section, phrase
