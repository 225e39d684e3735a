"""Cropper(edge_shift=N) without a GPU: the reference tests/mask_shift_ref.py against scipy in both directions, the
properties of the definition (duality, monotony, identity, the fixed points, the Euclidean disc, the crop's border), the
header, exports and op schema, the C export's refusals, the argument checks, the resolved defaults, the order of the
matte step, the CLI flags, the documents and the demonstration number."""
import importlib.util
import inspect
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


R = _load("mask_shift_ref")
SIZES = [(1, 1), (1, 2), (2, 1), (3, 3), (7, 7), (13, 17), (64, 65)]
RADII = (1, 2, 3, 5, 8, 13, 64)
DENSITIES = (0, 0.02, 0.5, 0.98, 1)


def _masks():
    for h, w in SIZES:
        rng = np.random.default_rng(100 * h + w)
        for density in DENSITIES:
            yield (h, w, density), rng.random((h, w)) < density


def _art(rows):
    return np.array([[c == "#" for c in row] for row in rows])


# ---- the reference against scipy
def test_reference_equals_scipy_in_both_directions():
    ndimage = pytest.importorskip("scipy").ndimage
    n = 0
    for what, m in _masks():
        for r in RADII:
            y, x = np.mgrid[-r:r + 1, -r:r + 1]
            disc = y * y + x * x <= r * r
            assert np.array_equal(R.grow(m, r), ndimage.binary_dilation(m, disc, border_value=0)), (what, r)
            assert np.array_equal(R.shrink(m, r), ndimage.binary_erosion(m, disc, border_value=1)), (what, -r)
            # and the threshold of the exact squared Euclidean distance to the nearest source inside the crop
            for source, got in ((m, R.grow(m, r)), (~m, ~R.shrink(m, r))):
                near = ndimage.distance_transform_edt(~source) if source.any() else np.full(m.shape, np.inf)
                assert np.array_equal(got, np.round(near ** 2) <= r * r), (what, r)
            n += 2
    assert n == 490


def test_the_planes_of_a_packed_call_are_each_their_own():
    rng = np.random.default_rng(5)
    m = rng.random((21, 9, 11)) < 0.3
    for shift in (-3, -1, 0, 2, 5):
        want = np.stack([R.grow(p, shift) if shift >= 0 else R.shrink(p, -shift) for p in m]).astype(np.uint8)
        got = R.shift_planes(m, shift)
        assert got.dtype == np.uint8 and np.array_equal(got, want), shift
        assert np.array_equal(R.shift_planes(m[:3], shift), want[:3]) and np.array_equal(R.shift_planes(m[:9], shift), want[:9])
    labels = rng.integers(0, 19, (3, 9, 11)).astype(np.uint8)
    for bits in R.CLASS_BITS:
        assert np.array_equal(R.shift_mask(labels, bits, -2), R.shrink(R.mask0(labels, bits), 2).astype(np.uint8))


# ---- properties
def test_duality_monotony_identity_and_fixed_points():
    for what, m in _masks():
        assert np.array_equal(R.shift_planes(m[None], 0)[0], m.astype(np.uint8)), what          # shift = 0: the identity
        before_grow, before_shrink = m, m
        for r in RADII:
            g, s = R.grow(m, r), R.shrink(m, r)
            assert np.array_equal(s, ~R.grow(~m, r)), (what, r)                                   # shrink(m) = 1 - grow(1 - m)
            assert not (before_grow & ~g).any() and not (s & ~before_shrink).any(), (what, r)   # monotone in r
            before_grow, before_shrink = g, s
            if not m.any():
                assert not g.any() and not s.any()
            if m.all():
                assert g.all() and s.all()                       # the crop's border is not background: nothing is eaten


def test_the_disc_is_euclidean():
    m = np.zeros((21, 21), bool)
    m[10, 10] = True
    assert R.grow(m, 5)[10 + 3, 10 + 4] and R.grow(m, 5)[10 - 4, 10 + 3]          # 9 + 16 = 25 <= 25
    assert not R.grow(m, 4)[10 + 3, 10 + 4]                                       # 25 > 16
    assert not R.grow(m, 5)[10 + 4, 10 + 4]                                       # 32 > 25: not the square, not the diamond's
    assert R.grow(m, 5)[10 + 5, 10] and not R.grow(m, 5)[10 + 5, 10 + 1]
    assert R.grow(m, 5).sum() == len(R.disc(5)) == 81
    hole = ~m
    assert not R.shrink(hole, 5)[13, 14] and R.shrink(hole, 4)[13, 14] and R.shrink(hole, 5)[14, 14]
    assert len(R.disc(0)) == 1 and len(R.disc(1)) == 5 and len(R.disc(2)) == 13 and len(R.disc(64)) == 12853


def test_a_shrink_does_not_eat_inwards_from_the_border():
    yy, xx = np.mgrid[0:40, 0:60]
    m = (xx - 30) ** 2 / 20.0 ** 2 + (yy - 39) ** 2 / 25.0 ** 2 <= 1                # an ellipse standing on the last row
    assert m[-1].sum() == 41 and not m[0].any() and not m[:, 0].any() and not m[:, -1].any()
    s = R.shrink(m, 4)
    assert s[-1].sum() == 33                                  # 4 columns a side, taken by the background beside it, not 0
    assert np.array_equal(s[-1], R.shrink(m[-1:], 4)[0])      # the last row shrinks as if it were alone: nothing from below
    art = _art(["....",
                ".##.",
                "####"])
    assert np.array_equal(R.shrink(art, 1), _art(["....", "....", ".##."]))
    assert np.array_equal(R.grow(art, 1), _art([".##.", "####", "####"]))


def test_label_bytes_past_the_classes_are_background_and_faces_do_not_touch():
    labels = np.array([[[1, 19, 1], [200, 1, 255], [1, 1, 1]]], np.uint8)
    assert np.array_equal(R.mask0(labels, R.DEFAULT_BITS)[0], _art(["#.#", ".#.", "###"]))
    out = R.shift_mask(labels, R.DEFAULT_BITS, -1)
    assert out.dtype == np.uint8 and np.array_equal(out[0], _art(["...", "...", ".#."]))    # (2, 1): nothing below it exists
    three = R.labels_of(R.SEPARATION, None, 5, 7)
    assert three[0].all() and not three[1].any() and three[2].all()
    assert np.array_equal(R.shift_mask(three, R.SUBJECT_BITS, 3), three) and np.array_equal(R.shift_mask(three, R.SUBJECT_BITS, -3), three)
    assert (R.TILE_H, R.TILE_W, R.MAX_SHIFT) == (64, 64, 64)
    src = open(os.path.join(ROOT, "face-crop-plus_amd", "csrc", "fcp_mask_shift.hip")).read()
    assert "constexpr int kTile = 64;" in src and "constexpr int kMaxShift = 64;" in src


# ---- header, exports, ops
def test_header_exports_and_ops():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import torch_ops as T
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    assert "#define FCP_ABI_VERSION 15" in hdr and N.ABI_VERSION == 15 and N.lib().fcp_abi_version() == 15
    assert "fcp_mask_shift_u8(" in hdr and "fcp_mask_shift_u8" in N.EXPORTS and hasattr(N.lib(), "fcp_mask_shift_u8")
    Pt, I, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    assert N.SIGNATURES["fcp_mask_shift_u8"] == [Pt, I, I, I, U, I, Pt, Pt]
    text = re.sub(r"[\s*]+", " ", hdr)                        # line breaks and the comment's stars aside
    for phrase in ("(class_bits >> labels(y,x)) & 1", "never a source", "(y-y')^2 + (x-x')^2 <= r^2", "border_value=0",
                   "border_value=1", "no workspace", "no float and no atomics", "must not overlap", "a shift outside -64..64",
                   'a "mask_shift:" message'):
        assert phrase in text, phrase
    ops = T.load()
    assert "mask_shift" in T.OPS and hasattr(ops, "mask_shift")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcp::mask_shift", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcp::mask_shift", "CPU")
    assert str(ops.mask_shift.default._schema) == "fcp::mask_shift(Tensor labels, int class_bits, int shift) -> Tensor"
    with pytest.raises(RuntimeError):                      # no CPU kernel: a missing device is an error, not a fallback
        ops.mask_shift(torch.zeros(1, 4, 4, dtype=torch.uint8), 2, -1)


def test_c_export_refuses_bad_arguments_before_any_device_call():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    lib = N.lib()
    one = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its checks first

    def err():
        return lib.fcp_last_error().decode()

    def shift(f=1, h=4, w=4, bits=2, shift=1, labels=one, out=one):
        return lib.fcp_mask_shift_u8(labels, f, h, w, bits, shift, out, None)
    for kw, text in (({"shift": 65}, "shift must be -64..64"), ({"shift": -65}, "shift must be -64..64"),
                     ({"shift": 1 << 30}, "shift must be"), ({"shift": -(1 << 31)}, "shift must be"),
                     ({"bits": 1 << 19}, "class_bits"), ({"bits": 0xFFFFFFFF}, "class_bits"), ({"h": 8193}, "8192"),
                     ({"w": 8193}, "8192"), ({"h": 0}, "bad sizes"), ({"w": 0}, "bad sizes"), ({"f": -1}, "bad sizes"),
                     ({"f": 65536}, "65535"), ({"labels": None}, "null pointer"), ({"out": None}, "null pointer"),
                     ({"labels": None, "shift": 0}, "null pointer")):
        assert shift(**kw) == -1, kw
        assert text in err() and err().startswith("mask_shift:"), (kw, err())
    for s in (-64, 0, 64):
        assert shift(f=0, shift=s, labels=None, out=None) == 0                   # a no-op
    assert shift(f=0, shift=65, labels=None, out=None) == -1                     # the checks come before the no-op


# ---- constructor, defaults, the matte step, CLI
def test_argument_checks():
    from face_crop_plus_amd import matte as M
    assert M.check_edge_shift(None) is None and M.MAX_EDGE_SHIFT == 64 == R.MAX_SHIFT
    for good, want in ((-2, -2), (1, 1), (64, 64), (-64, -64), (np.int64(-3), -3), (np.uint8(7), 7), (2.0, 2), (np.float32(-5.0), -5)):
        got = M.check_edge_shift(good)
        assert got == want and type(got) is int, good
    for bad in (0, 0.0, 65, -65, True, False, np.bool_(True), 2.5, -0.5, "2", "-2", [2], (2,), float("nan"), float("inf")):
        with pytest.raises(ValueError, match="edge_shift must be"):
            M.check_edge_shift(bad)
    assert list(inspect.signature(M.shift_mask).parameters) == ["labels_dev", "class_bits", "shift"]
    assert list(inspect.signature(M.subject_mask).parameters) == ["labels_dev", "class_bits", "keep_largest", "max_hole"]
    for text in ("edge_shift=N", "fcp_mask_shift_u8", "torch.ops.fcp.mask_shift", "never a source", "(y-y')^2 + (x-x')^2 <= r^2"):
        assert text in M.__doc__, text


def test_constructor_checks(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    params = inspect.signature(Cropper).parameters
    assert params["edge_shift"].default is None
    # with the other matte options, after the last of them: the tail of the signature is pinned by tests/test_sharpness_cpu.py
    assert list(params)[list(params).index("decontaminate") + 1] == "edge_shift"
    assert list(params)[-2:] == ["interpolation", "min_sharpness"]
    for bad in (0, 65, -65, True, "2", 2.5, [2]):
        with pytest.raises(ValueError, match="edge_shift must be"):
            Cropper(background=0, edge_shift=bad)
    message = "edge_shift needs background or background_blur: without one it would do nothing"
    for kw in ({"edge_shift": -2}, {"edge_shift": 3, "clahe": 2.0}, {"edge_shift": 1, "min_sharpness": 5.0}):
        with pytest.raises(ValueError, match=message):
            Cropper(**kw)
    # the messages of before stand word for word, and come first
    with pytest.raises(ValueError, match="subject / fill_holes need background or background_blur: without one they would do nothing"):
        Cropper(subject="largest", edge_shift=-2)
    with pytest.raises(ValueError, match="refine needs background or background_blur: without one it would do nothing"):
        Cropper(refine=4, edge_shift=2)
    with pytest.raises(ValueError, match="foreground / feather need background or background_blur: without one they would do nothing"):
        Cropper(feather=3, edge_shift=-2)
    with pytest.raises(ValueError, match="background and background_blur exclude each other: the background is filled or blurred"):
        Cropper(background=0, background_blur=3.0, edge_shift=-2)
    with pytest.raises(ValueError, match="no alignment"):
        Cropper(background=0, edge_shift=-2, det_threshold=None, landmarks=None)
    for kw in ({"background": 0, "edge_shift": -2}, {"background_blur": 3.0, "edge_shift": 64},
               {"background": "transparent", "output_format": "png", "decontaminate": 4, "edge_shift": np.int64(-1)},
               {"background": (1, 2, 3), "subject": "largest", "fill_holes": 8, "refine": 4, "edge_shift": 3.0}):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(**kw)


def test_cropper_resolves_the_defaults(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    c = Cropper(background=9, edge_shift=-2)
    assert (c.edge_shift, c.subject, c.fill_holes, c.feather, c.refine, c.foreground_bits) == (-2, None, None, 5, None, R.DEFAULT_BITS)
    c = Cropper(background_blur=2, edge_shift=3.0, refine=4, foreground=[17, 1])
    assert (c.edge_shift, c.feather, c.foreground) == (3, 0, (1, 17)) and type(c.edge_shift) is int
    assert Cropper(background=9).edge_shift is None and Cropper().edge_shift is None
    doc = Cropper.__init__.__doc__
    assert "``edge_shift``" in doc and "matte.shift_mask" in doc and "section 2o" in doc


def test_the_matte_step_shifts_after_the_subject_and_before_every_soft_edge(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import matte as M
    calls = []
    monkeypatch.setattr(M, "subject_mask", lambda *a: calls.append(("subject", a[0], a[1:])) or "cleaned")
    monkeypatch.setattr(M, "shift_mask", lambda labels, bits, shift: calls.append(("shift", labels, bits, shift)) or "shifted")
    monkeypatch.setattr(M, "matte", lambda crops, labels, bits, *a, **k: calls.append(("matte", labels, bits)) or ("out", None))
    monkeypatch.setattr(M, "matte_blur", lambda crops, labels, bits, *a, **k: calls.append(("blur", labels, bits)) or ("out", None))
    monkeypatch.setattr(M, "refine_alpha", lambda crops, labels, bits, *a: calls.append(("refine", labels, bits)) or "alpha")
    monkeypatch.setattr(M, "feather_alpha", lambda labels, bits, feather: calls.append(("feather", labels, bits)) or "alpha")
    monkeypatch.setattr(M, "cutout", lambda crops, alpha, *a: calls.append(("cutout", alpha)) or "rgba")
    c = Cropper.__new__(Cropper)
    c.background, c.background_blur, c.foreground_bits, c.feather = (0, 0, 0), None, R.ONE_17, 5
    assert "edge_shift" not in vars(c)
    assert c._matte_device("crops", "labels") == ("out", None)
    assert calls == [("matte", "labels", R.ONE_17)]                  # the attribute absent: nothing new is called
    del calls[:]
    c.edge_shift = None
    c._matte_device("crops", "labels")
    assert calls == [("matte", "labels", R.ONE_17)]                  # and None launches nothing
    del calls[:]
    c.edge_shift = -2
    c._matte_device("crops", "labels")
    assert calls == [("shift", "labels", R.ONE_17, -2), ("matte", "shifted", 2)]                  # alone: the labels' own bits
    del calls[:]
    c.subject, c.fill_holes, c.refine, c.refine_eps, c.edge_shift = "largest", None, 4, 64, 3
    c._matte_device("crops", "labels")
    assert calls == [("subject", "labels", (R.ONE_17, True, 0)), ("shift", "cleaned", 2, 3), ("refine", "shifted", 2),
                     ("matte", "shifted", 2)]
    del calls[:]
    c.subject, c.fill_holes, c.refine, c.background, c.background_blur, c.blur_taps = None, 16, None, None, 3.0, [1]
    c._matte_device("crops", "labels")
    assert calls == [("subject", "labels", (R.ONE_17, False, 16)), ("shift", "cleaned", 2, 3), ("blur", "shifted", 2)]
    del calls[:]
    c.fill_holes, c.background, c.background_blur, c.decontaminate_taps, c.edge_shift = None, M.TRANSPARENT, None, None, -1
    assert c._matte_device("crops", "labels", with_alpha=True) == ("rgba", "alpha")
    assert calls == [("shift", "labels", R.ONE_17, -1), ("feather", "shifted", 2), ("cutout", "alpha")]


def test_cli_flags(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    plain = parse_args(base)
    assert "edge_shift" not in plain
    assert parse_args(base + ["-es", "-2"])["edge_shift"] == -2
    assert parse_args(base + ["--edge-shift", "3"])["edge_shift"] == 3
    assert parse_args(base + ["--edge-shift=-64"])["edge_shift"] == -64
    got = parse_args(base + ["-bg", "255,255,255", "-es", "-2", "-rf", "4"])
    assert (got["background"], got["edge_shift"], got["refine"]) == ([255, 255, 255], -2, 4)
    got = parse_args(base + ["-es", "-2"])
    assert {k: v for k, v in got.items() if k != "edge_shift"} == plain                            # nothing else moves
    for bad in (["-es", "2.5"], ["-es", "x"], ["-es"], ["-es", "-2.5"], ["--edge-shift", "two"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"edge-shift": -3, "background-blur": 3.0}))
    got = parse_args(base + ["-c", str(cfg)])
    assert (got["edge_shift"], got["background_blur"]) == (-3, 3.0)
    assert {k: v for k, v in got.items() if k not in ("edge_shift", "background_blur")} == plain
    assert parse_args(base + ["-c", str(cfg), "-es", "5"])["edge_shift"] == 5


# ---- the documents and the demonstration number
def test_the_demonstration_number_is_what_the_reference_gives():
    """A mask 2 px outside the true subject, over a new fill through the feather of 5: the ring's mean colour error with
    the mask as it is and with edge_shift=-2 (measured: 14.26 and 0.09 gray levels over 378 ring pixels)."""
    without, with_shift, ring = R.demo(_load("matte_ref").matte)
    print("ring", ring, "without", without, "with edge_shift=-2", with_shift)
    assert ring == 378
    assert with_shift < without / 10
    sentence = f"from {without:.1f} gray levels to {with_shift:.2f}"
    assert sentence == "from 14.3 gray levels to 0.09"
    readme = re.sub(r"\s+", " ", open(os.path.join(ROOT, "README.md")).read())
    integration = re.sub(r"\s+", " ", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    section = integration[integration.index("## 2o."):integration.index("## 3.")]
    assert sentence in readme and sentence in section


def test_docs_say_what_moves_and_what_does_not():
    readme = re.sub(r"\s+", " ", open(os.path.join(ROOT, "README.md")).read())
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`Cropper(edge_shift=N)` / `-es N`" in readme and "INTEGRATION.md section 2o" in readme
    assert integration.index("## 2n.") < integration.index("## 2o.") < integration.index("## 3.")
    section = re.sub(r"\s+", " ", integration[integration.index("## 2o."):integration.index("## 3.")])   # line breaks aside
    for phrase in ("`-es N` / `--edge-shift N`", "never a source", "(y-y')^2 + (x-x')^2 <= r^2", "binary_dilation", "binary_erosion",
                   "border_value=1", "fcp_mask_shift_u8", "torch.ops.fcp.mask_shift", "matte.shift_mask", "tests/mask_shift_ref.py",
                   "One launch", "no workspace", "must not overlap", "matte.SUBJECT_BITS", "The ABI version stays 15",
                   "fcp_feather_alpha_u8", "64 crops of 256 x 256"):
        assert phrase in section, phrase
    before = re.sub(r"\s+", " ", integration[integration.index("## 2n."):integration.index("## 2o.")])
    for phrase in ("exactly 255", "exactly 0", "the crop's colour stands", "width of the soft edge", "fcp_cutout_u8"):
        assert phrase in before, phrase                      # section 2n keeps what it said
