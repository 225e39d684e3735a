"""Cropper(refine=...) without a GPU: the reference tests/matte_refine_ref.py against its own pixel-by-pixel form, the
properties of the definition (constant mask, locality, constant guide, the edge it follows), the inputs that need the
wide accumulators, the argument checks, the resolved defaults, the CLI flags and the C exports' refusals."""
import importlib.util
import inspect
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("_matte_refine_ref", os.path.join(os.path.dirname(__file__), "matte_refine_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
MR = R.MR
SIZES = [(1, 1), (1, 5), (2, 2), (3, 2), (2, 7), (13, 17)]
RADII = (1, 2, 16)
EPS = (1, 64, 4096)


def test_bounds_arithmetic():
    """The figures the kernel's widths rest on, from r = 16 and 8-bit inputs alone."""
    n = R.MAX_N
    assert n == 33 * 33 == 1089
    assert R.BOUND_S1 == 277695 and R.BOUND_S2 == 70812225 < 2 ** 32
    assert n * R.BOUND_S2 < R.BOUND_COV and R.BOUND_S1 * R.BOUND_S1 < R.BOUND_COV          # |cov|, var < 7.8e10
    assert R.BOUND_COV + R.MAX_EPS * n * n < R.BOUND_DEN                                    # den < 1.6e11
    assert R.BOUND_COV * 4096 < 32 * 10 ** 13 < 2 ** 63
    # |a| <= 127.5 / (2 sqrt(eps)): |cov| <= sd_I * 127.5 n^2 (Cauchy-Schwarz; sd_p <= 127.5), sd_I / (var_I + eps) <= 1 / (2 sqrt(eps))
    assert R.BOUND_A == 4096 * 255 // 4 + 1                                                  # ... and the rounding of rdiv
    assert 255 * 4096 + R.BOUND_A * 255 + 1 < R.BOUND_B < 2 ** 31                           # |B| <= (4096 S_p + |A| S_I) / n + 1
    assert n * R.BOUND_A < R.BOUND_BOX_A < 2 ** 31 and n * R.BOUND_B < R.BOUND_BOX_B
    assert 33 * R.BOUND_B > 2 ** 31                                                         # a row sum of B is past 31 bits
    assert 33 * R.BOUND_A < 2 ** 25 and 33 * R.BOUND_B < 2 ** 33                            # ... and the two pack into 64
    assert R.BOUND_BOX_A * 255 + R.BOUND_BOX_B + 2048 * n < 2 ** 63
    assert (R.BOUND_BOX_A * 255 + R.BOUND_BOX_B + 2048 * n) >> 12 < 2 ** 31                 # 32 bits after the shift


@pytest.mark.parametrize("shape", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_vectorised_reference_equals_the_python_int_form(shape):
    h, w = shape
    rng = np.random.default_rng(100 * h + w)
    checked = 0
    for r in RADII:
        for eps in EPS:
            for guide, p in ((rng.integers(0, 256, (h, w)), MR.random_mask(rng, h, w)),
                             (MR.random_mask(rng, h, w), MR.random_mask(rng, h, w))):
                assert np.array_equal(R.refine(guide, p, r, eps), R.refine_direct(guide, p, r, eps)), (shape, r, eps)
                checked += 1
    assert checked == 18


def test_gray_is_the_gray_of_min_sharpness():
    rng = np.random.default_rng(1)
    c = rng.integers(0, 256, (50, 3), dtype=np.uint8)
    want = [(9798 * int(r) + 19235 * int(g) + 3735 * int(b) + 16384) >> 15 for r, g, b in c]
    assert R.gray(c).tolist() == want
    assert R.gray(np.array([[255, 255, 255], [0, 0, 0]], np.uint8)).tolist() == [255, 0]
    src = open(os.path.join(ROOT, "face-crop-plus_amd", "csrc", "fcp_sharpness.hip")).read()
    assert "(9798u * r + 19235u * g + 3735u * b + 16384u) >> 15" in src


@pytest.mark.parametrize("r", RADII)
def test_a_constant_mask_stays_constant(r):
    rng = np.random.default_rng(2)
    for h, w in SIZES + [(33, 40)]:
        crops = MR.random_crops(rng, 2, h, w)
        for eps in EPS:
            for labels, value in ((np.full((2, h, w), 1, np.uint8), 255), (np.zeros((2, h, w), np.uint8), 0)):
                alpha = R.alpha_of(crops, labels, MR.DEFAULT_BITS, r, eps)
                assert (alpha == value).all(), (h, w, r, eps, value)
                out, _ = R.matte(crops, labels, MR.DEFAULT_BITS, r, eps, (1, 2, 3))
                assert (out == (crops if value else np.array([1, 2, 3], np.uint8))).all()


@pytest.mark.parametrize("r", (1, 2, 5))
def test_locality(r):
    """A pixel more than 2 r (Chebyshev) from every pixel of the other mask value keeps its mask value."""
    rng = np.random.default_rng(3)
    h, w = 40, 50
    p = np.zeros((h, w), np.int64)
    p[:, 25:] = 255
    p[10:14, 3:6] = 255
    guide = rng.integers(0, 256, (h, w))
    far = np.ones((h, w), bool)
    for y in range(h):
        for x in range(w):
            win = p[max(0, y - 2 * r):y + 2 * r + 1, max(0, x - 2 * r):x + 2 * r + 1]
            far[y, x] = (win == p[y, x]).all()
    assert far.any() and (~far).any()
    for eps in EPS:
        alpha = R.refine(guide, p, r, eps)
        assert (alpha[far] == p[far]).all(), (r, eps)
        assert (alpha[~far] != p[~far]).any()


def test_a_constant_guide_gives_the_twice_box_averaged_mask():
    rng = np.random.default_rng(4)
    for (h, w), r in (((13, 17), 1), ((13, 17), 2), ((9, 40), 16), ((3, 2), 2)):
        p = MR.random_mask(rng, h, w).astype(np.int64)
        n = (2 * r + 1) ** 2
        ys = [[MR.reflect101(y + j, h) for j in range(-r, r + 1)] for y in range(h)]
        xs = [[MR.reflect101(x + i, w) for i in range(-r, r + 1)] for x in range(w)]
        for level in (0, 77, 255):
            guide = np.full((h, w), level, np.int64)
            a, b = R.coefficients(guide, p, r, 64)
            assert (a == 0).all()
            # independently: B = rdiv(4096 S_p, n) of the window, alpha = ((sum of B + 2048 n) >> 12) // n
            mean = [[(4096 * sum(int(p[yy, xx]) for yy in ys[y] for xx in xs[x]) + n // 2) // n for x in range(w)] for y in range(h)]
            want = np.array([[((sum(mean[yy][xx] for yy in ys[y] for xx in xs[x]) + 2048 * n) >> 12) // n for x in range(w)]
                             for y in range(h)])
            assert want.min() >= 0 and want.max() <= 255
            assert np.array_equal(R.refine(guide, p, r, 64), want.astype(np.uint8)), (h, w, r, level)


def test_the_edge_follows_the_guide():
    """Mask edge at x = 20, guide step at x = 23, r = 4, eps = 64: the alpha falls off a cliff at the guide's edge, where the
    feathered alpha of the same mask is flat."""
    rng = np.random.default_rng(7)
    h, w = 24, 48
    guide = np.clip(np.where(np.arange(w) < 23, 200, 40)[None, :] + rng.integers(-3, 4, (h, w)), 0, 255)
    p = np.repeat(np.where(np.arange(w) < 20, 255, 0)[None, :], h, 0)
    alpha = R.refine(guide, p, 4, 64).astype(np.int64)
    drop = alpha[:, 22] - alpha[:, 23]
    assert drop[8:16].min() >= 64, drop
    assert (alpha[8:16, 23:] <= 2).all() and (alpha[8:16, 22] >= 64).all()
    feathered = MR.alpha_separable(p.astype(np.uint8), 5).astype(np.int64)
    assert (feathered[:, 22] == 0).all() and (feathered[:, 23] == 0).all()
    # ... and over a flat guide the same mask gives no cliff anywhere
    flat = R.refine(np.full((h, w), 200), p, 4, 64).astype(np.int64)
    assert np.abs(np.diff(flat, axis=1)).max() < 64


def test_stripes_need_more_than_32_bits():
    r = 16
    guide, p = R.stripes(40, 70, r)
    a, b = R.coefficients(guide, p, r, 1)
    assert np.abs(b).max() > 2 ** 25
    assert np.abs(R.box(b, r)).max() > 2 ** 35
    rows = np.zeros_like(b)
    for i in range(-r, r + 1):
        rows += b[:, [MR.reflect101(x + i, 70) for x in range(70)]]
    assert np.abs(rows).max() > 2 ** 30                       # a row sum already fills 31 bits at this input
    crops, labels = R.stripe_inputs(3, 40, 70, r)
    assert np.array_equal(R.gray(crops[0]), guide) and np.array_equal(MR.mask(labels[0], MR.DEFAULT_BITS), p)
    alpha = R.refine(guide, p, r, 1)
    assert alpha.min() < 64 and alpha.max() > 192


def test_q_leaves_the_byte_range_before_the_clamp():
    """r = 1, eps = 1, a random 0 / 255 mask: with the mask itself as the guide the filter reproduces it (q stays inside
    0..255: a = var / (var + eps) < 1); over a random gray guide the slope is large and q over- and undershoots."""
    rng = np.random.default_rng(9)
    h, w = 40, 40
    p = MR.random_mask(rng, h, w).astype(np.int64)
    a, b = R.coefficients(p, p, 1, 1)
    q = R.q_of(p, a, b, 1)
    assert q.min() >= 0 and q.max() <= 255
    guide = rng.integers(0, 256, (h, w))
    a, b = R.coefficients(guide, p, 1, 1)
    q = R.q_of(guide, a, b, 1)
    assert q.min() < 0 and q.max() > 255, (q.min(), q.max())
    alpha = R.refine(guide, p, 1, 1)
    assert alpha.min() == 0 and alpha.max() == 255


# ---- constructor, defaults, CLI
def test_argument_checks():
    from face_crop_plus_amd import matte as M
    assert M.check_refine(None) is None and M.check_refine(1) == 1 and M.check_refine(16) == 16 and M.check_refine(np.int64(4)) == 4
    assert M.check_refine(3.0) == 3
    for bad in (0, 17, -1, True, False, "4", 2.5, [4], float("nan")):
        with pytest.raises(ValueError, match="refine"):
            M.check_refine(bad)
    assert M.check_refine_eps(None) == 64 == M.DEFAULT_REFINE_EPS
    assert M.check_refine_eps(1) == 1 and M.check_refine_eps(4096) == 4096 and M.check_refine_eps(np.int32(9)) == 9
    for bad in (0, 4097, -64, True, "64", 0.5, (64,)):
        with pytest.raises(ValueError, match="refine_eps"):
            M.check_refine_eps(bad)
    assert (M.MIN_REFINE, M.MAX_REFINE, M.MIN_REFINE_EPS, M.MAX_REFINE_EPS) == (R.MIN_RADIUS, R.MAX_RADIUS, R.MIN_EPS, R.MAX_EPS)
    for fn in (M.matte, M.matte_blur):
        assert list(inspect.signature(fn).parameters)[-1] == "alpha" and inspect.signature(fn).parameters["alpha"].default is None


def test_constructor_checks(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    params = inspect.signature(Cropper).parameters
    assert params["refine"].default is None and params["refine_eps"].default is None
    for bad in (0, 17, True, "4", 2.5):
        with pytest.raises(ValueError, match="refine must be"):
            Cropper(background=0, refine=bad)
    for bad in (0, 4097, True, "64"):
        with pytest.raises(ValueError, match="refine_eps must be"):
            Cropper(background=0, refine=4, refine_eps=bad)
    with pytest.raises(ValueError, match="refine_eps needs refine"):
        Cropper(background=0, refine_eps=64)
    with pytest.raises(ValueError, match="refine needs background or background_blur"):
        Cropper(refine=4)
    with pytest.raises(ValueError, match="refine needs background or background_blur"):
        Cropper(refine=4, refine_eps=8)
    for kw in ({"background": 0}, {"background_blur": 3.0}):
        for feather in (0, 5):
            with pytest.raises(ValueError, match="exclude each other"):
                Cropper(refine=4, feather=feather, **kw)
    # the messages of before stand word for word
    with pytest.raises(ValueError, match="foreground / feather need background or background_blur: without one they would do nothing"):
        Cropper(feather=3)
    with pytest.raises(ValueError, match="background and background_blur exclude each other: the background is filled or blurred"):
        Cropper(background=0, background_blur=3.0, refine=4)
    with pytest.raises(ValueError, match="no alignment"):
        Cropper(background=0, refine=4, det_threshold=None, landmarks=None)
    for kw in ({"background": 0, "refine": 1}, {"background_blur": 3.0, "refine": 16, "refine_eps": 4096},
               {"background": (1, 2, 3), "refine": np.int64(8), "refine_eps": 1, "foreground": [1, 17]}):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(**kw)


def test_cropper_resolves_the_defaults(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    c = Cropper(background=9, refine=4)
    assert (c.refine, c.refine_eps, c.feather, c.background, c.foreground_bits) == (4, 64, 0, (9, 9, 9), MR.DEFAULT_BITS)
    c = Cropper(background_blur=2, refine=16, refine_eps=1, foreground=[17, 1])
    assert (c.refine, c.refine_eps, c.feather, c.background, c.foreground) == (16, 1, 0, None, (1, 17))
    assert len(c.blur_taps) == 7
    c = Cropper(background=9)
    assert (c.refine, c.refine_eps, c.feather) == (None, None, 5)
    c = Cropper()
    assert (c.refine, c.refine_eps, c.feather) == (None, None, None)


def test_init_models_works_without_the_new_attributes(monkeypatch):
    from face_crop_plus_amd import Cropper
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: None)
    c = Cropper.__new__(Cropper)
    c.device, c.det_threshold, c.landmarks, c.enh_threshold = torch.device("cuda:0"), None, (None, None), None
    c.attr_groups, c.mask_groups, c.batch_size, c.weights, c.precision, c.encoder = None, None, 8, {}, None, "host"
    c.background, c.background_blur = None, None
    assert "refine" not in vars(c)
    c._init_models()
    assert c.par_model is None


def test_cli_flags(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    plain = parse_args(base)
    assert "refine" not in plain and "refine_eps" not in plain
    assert parse_args(base + ["-rf", "4"])["refine"] == 4
    assert parse_args(base + ["--refine", "16"])["refine"] == 16
    got = parse_args(base + ["-bg", "0,177,64", "-rf", "8", "-re", "256"])
    assert (got["background"], got["refine"], got["refine_eps"]) == ([0, 177, 64], 8, 256)
    assert parse_args(base + ["--refine-eps", "1", "-rf", "2"])["refine_eps"] == 1
    got = parse_args(base + ["-rf", "4", "-re", "64"])
    assert {k: v for k, v in got.items() if k not in ("refine", "refine_eps")} == plain          # nothing else moves
    for bad in (["-rf", "soft"], ["-rf"], ["-rf", "2.5"], ["-re", "x"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"refine": 6, "refine-eps": 128, "background-blur": 3.0}))
    got = parse_args(base + ["-c", str(cfg)])
    assert (got["refine"], got["refine_eps"], got["background_blur"]) == (6, 128, 3.0)
    assert {k: v for k, v in got.items() if k not in ("refine", "refine_eps", "background_blur")} == plain


def test_header_exports_and_ops():
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import torch_ops as T
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    assert "#define FCP_ABI_VERSION 15" in hdr and N.ABI_VERSION == 15 and N.lib().fcp_abi_version() == 15
    for name in ("fcp_matte_refine_workspace_bytes", "fcp_matte_refine_u8", "fcp_matte_alpha_u8", "fcp_matte_blur_alpha_u8"):
        assert name + "(" in hdr and name in N.EXPORTS and hasattr(N.lib(), name)
    ops = T.load()
    for name in ("matte_refine", "matte_alpha", "matte_blur_alpha"):
        assert name in T.OPS and hasattr(ops, name)
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"fcp::{name}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"fcp::{name}", "CPU")
    assert str(ops.matte_refine.default._schema) == \
        "fcp::matte_refine(Tensor crops, Tensor labels, int class_bits, int radius, int eps) -> Tensor"
    with pytest.raises(RuntimeError):                      # no CPU kernel: a missing device is an error, not a fallback
        ops.matte_refine(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8), 2, 1, 64)


def test_c_exports_refuse_bad_arguments_before_any_device_call():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    lib = N.lib()
    one = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its checks first

    def err():
        return lib.fcp_last_error().decode()

    def refine(f=1, h=4, w=4, bits=2, radius=4, eps=64, crops=one, labels=one, alpha=one, ws=one, ws_bytes=1 << 20):
        return lib.fcp_matte_refine_u8(crops, labels, f, h, w, bits, radius, eps, alpha, ws, ws_bytes, None)
    assert lib.fcp_matte_refine_workspace_bytes(3, 5, 7) == 3 * 5 * 7 * 8
    assert lib.fcp_matte_refine_workspace_bytes(0, 5, 7) == 0
    for bad in ((1, 8193, 1), (1, 1, 8193), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (65536, 1, 1)):
        assert lib.fcp_matte_refine_workspace_bytes(*bad) == -1
    for kw, text in (({"radius": 0}, "radius"), ({"radius": 17}, "radius"), ({"eps": 0}, "eps"), ({"eps": 4097}, "eps"),
                     ({"bits": 1 << 19}, "class_bits"), ({"h": 8193}, "8192"), ({"w": 8193}, "8192"), ({"w": 0}, "bad sizes"),
                     ({"f": -1}, "bad sizes"), ({"f": 65536}, "65535"), ({"crops": None}, "null pointer"),
                     ({"labels": None}, "null pointer"), ({"alpha": None}, "null pointer"), ({"ws": None}, "workspace"),
                     ({"ws_bytes": 127}, "workspace"), ({"ws": ctypes.c_void_p(8)}, "aligned")):
        assert refine(**kw) == -1, kw
        assert text in err() and err().startswith("matte_refine:"), (kw, err())
    assert refine(f=0, crops=None, labels=None, alpha=None, ws=None, ws_bytes=0) == 0          # a no-op

    def fill(f=1, h=4, w=4, r=0, g=0, b=0, crops=one, alpha=one, out=one):
        return lib.fcp_matte_alpha_u8(crops, alpha, f, h, w, r, g, b, out, None)
    for kw, text in (({"h": 8193}, "8192"), ({"w": 0}, "bad sizes"), ({"f": -1}, "bad sizes"), ({"f": 65536}, "65535"),
                     ({"r": 256}, "fill"), ({"g": -1}, "fill"), ({"b": 256}, "fill"), ({"crops": None}, "null pointer"),
                     ({"alpha": None}, "null pointer"), ({"out": None}, "null pointer")):
        assert fill(**kw) == -1, kw
        assert text in err() and err().startswith("matte_alpha:"), (kw, err())
    assert fill(f=0, crops=None, alpha=None, out=None) == 0

    taps = [4096 - 2 * (1000 + 500 + 100), 1000, 500, 100]
    t16 = (ctypes.c_uint16 * 49)(*taps)

    def blur(f=1, h=4, w=4, bits=2, t=t16, radius=3, crops=one, labels=one, alpha=one, out=one, ws=one, ws_bytes=1 << 20):
        return lib.fcp_matte_blur_alpha_u8(crops, labels, alpha, f, h, w, bits, t, radius, out, ws, ws_bytes, None)
    for kw, text in (({"radius": 2}, "radius"), ({"radius": 49}, "radius"), ({"bits": 1 << 19}, "class_bits"), ({"h": 8193}, "8192"),
                     ({"w": 0}, "bad sizes"), ({"f": 65536}, "65535"), ({"t": None}, "taps"), ({"radius": 4}, "tap 4 is 0"),
                     ({"crops": None}, "null pointer"), ({"labels": None}, "null pointer"), ({"alpha": None}, "null pointer"),
                     ({"out": None}, "null pointer"), ({"ws": None}, "workspace"), ({"ws_bytes": 255}, "workspace"),
                     ({"ws": ctypes.c_void_p(8)}, "aligned")):
        assert blur(**kw) == -1, kw
        assert text in err() and err().startswith("matte_blur_alpha:"), (kw, err())
    short = (ctypes.c_uint16 * 49)(*([4089, 1, 1, 1]))
    assert blur(t=short) == -1 and "sum to 4096" in err()
    assert blur(f=0, crops=None, labels=None, alpha=None, out=None, ws=None, ws_bytes=0) == 0
