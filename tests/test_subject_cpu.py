"""Cropper(subject=, fill_holes=) without a GPU: the reference tests/subject_ref.py against its own pixel-by-pixel form and
against scipy, the properties of the definition (subset, connectedness, superset, idempotence, the hole threshold, the tie
rule, the diagonal pocket, the island inside a hole), label bytes past the classes, independent faces, the argument
checks, the resolved defaults, the CLI flags and the C export's refusals."""
import importlib.util
import inspect
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load():
    spec = importlib.util.spec_from_file_location("_subject_ref", os.path.join(os.path.dirname(__file__), "subject_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
SIZES = [(1, 1), (1, 2), (2, 1), (3, 3), (5, 4), (7, 7), (13, 17), (R.TILE_H + 1, R.TILE_W + 1)]
OPTIONS = [(True, 0), (False, 1), (False, 5), (True, 5)]


def _masks():
    """(name, shape, m0) of every pattern at every small size, and of the random ones at three seeds."""
    for h, w in SIZES:
        rng = np.random.default_rng(100 * h + w)
        for name, make in R.PATTERNS.items():
            yield name, (h, w), R.mask0(make(rng, h, w), R.DEFAULT_BITS)
        for seed in range(3):
            yield f"random41/{seed}", (h, w), R.mask0(R.PATTERNS["random41"](rng, h, w), R.DEFAULT_BITS)


def _art(rows):
    return np.array([[c == "#" for c in row] for row in rows])


# ---- the reference against itself and against scipy
def test_run_form_equals_the_pixel_form():
    n = 0
    for name, shape, m in _masks():
        for s, conn in ((m, 8), (~m, 4), (m, 4), (~m, 8)):
            a, b = R.components(s, conn), R.components_slow(s, conn)
            assert a.dtype == np.int64 and np.array_equal(a, b), (name, shape, conn)
            assert np.array_equal(a >= 0, s) and (a[s] <= np.flatnonzero(s)).all()       # a root is its component's first pixel
            n += 1
    assert n == 4 * len(SIZES) * (len(R.PATTERNS) + 3)
    labels = np.stack([R.PATTERNS[p](np.random.default_rng(3), 13, 17) for p in ("random41", "nested", "classes")])
    for keep, hole in OPTIONS + [(True, 13 * 17), (False, 13 * 17), (False, 0)]:
        for bits in (R.DEFAULT_BITS, 1, R.ONE_17):
            assert np.array_equal(R.subject_mask(labels, bits, keep, hole),
                                  R.subject_mask(labels, bits, keep, hole, comp=R.components_slow)), (keep, hole, bits)


def test_reference_equals_scipy():
    ndimage = pytest.importorskip("scipy").ndimage
    n = 0
    for name, (h, w), m in _masks():
        lab8, k8 = ndimage.label(m, structure=np.ones((3, 3), int))
        if k8:
            areas = ndimage.sum(m, lab8, range(1, k8 + 1))
            want = lab8 == 1 + int(np.argmax(areas))                  # scipy numbers by first pixel: the first maximum is the tie rule
        else:
            want = m
        assert np.array_equal(R.largest(m), want), (name, h, w)
        assert np.array_equal(R.filled(m, h * w), ndimage.binary_fill_holes(m)), (name, h, w)
        lab4, k4 = ndimage.label(~m)
        for limit in (1, 5):
            want = m.copy()
            for c in range(1, k4 + 1):
                region = lab4 == c
                ys, xs = np.nonzero(region)
                if ys.min() > 0 and xs.min() > 0 and ys.max() < h - 1 and xs.max() < w - 1 and region.sum() <= limit:
                    want |= region
            assert np.array_equal(R.filled(m, limit), want), (name, h, w, limit)
        n += 1
    assert n == len(SIZES) * (len(R.PATTERNS) + 3)


# ---- properties
def test_subject_is_a_connected_subset_and_holes_a_superset_and_both_idempotent():
    for name, shape, m in _masks():
        m1 = R.largest(m)
        assert not (m1 & ~m).any() and R.connected(m1, 8, R.components_slow), (name, shape)
        assert m1.any() == m.any()
        assert np.array_equal(R.largest(m1), m1), (name, shape)
        for n in (1, 5, m.size):
            m2 = R.filled(m1, n)
            assert not (m1 & ~m2).any() and np.array_equal(R.filled(m2, n), m2), (name, shape, n)
        both = R.subject_mask(m[None].astype(np.uint8), R.SUBJECT_BITS, True, 5)
        assert np.array_equal(R.subject_mask(both, R.SUBJECT_BITS, True, 5), both), (name, shape)


def test_a_hole_of_exactly_n_is_filled_and_one_of_n_plus_one_is_not():
    m = _art(["#########",
              "#..#...##",
              "#..#...##",
              "#########"])
    assert np.array_equal(R.filled(m, 3), m)
    four = R.filled(m, 4)
    assert four[1:3, 1:3].all() and not four[1:3, 4:7].any()
    assert np.array_equal(R.filled(m, 5), four)
    assert R.filled(m, 6).all()


def test_the_tie_goes_to_the_first_pixel_in_raster_order():
    h, w = 5, 9
    m = R.mask0(R.PATTERNS["tie"](None, h, w), R.DEFAULT_BITS)
    a, b = np.zeros_like(m), np.zeros_like(m)
    a[0:2, w - 1] = True                                    # starts at (0, w - 1): raster index w - 1
    b[1:3, 0] = True                                        # starts at (1, 0): raster index w, though its box starts at column 0
    assert np.array_equal(m, a | b) and a.sum() == b.sum()
    assert np.array_equal(R.largest(m), a)
    assert np.array_equal(R.largest(m, R.components_slow), a)
    assert np.array_equal(R.largest(m[:, ::-1]), a[:, ::-1])          # mirrored, A starts at (0, 0) and still comes first
    assert np.array_equal(R.largest(m[::-1]), b[::-1])                # upside down, B starts at (2, 0) before A at (3, w - 1)


def test_a_pocket_joined_to_the_outside_only_diagonally_is_a_hole():
    m = _art([".#...",
              "#.#..",
              ".#...",
              "....."])
    got = R.filled(m, 1)
    assert got[1, 1] and got.sum() == m.sum() + 1
    assert R.connected(m, 8) and not R.connected(m, 4)


def test_an_island_inside_a_hole_is_removed_and_counts_in_its_area():
    m = _art(["#######",
              "#.....#",
              "#..#..#",
              "#.....#",
              "#######"])
    labels = m[None].astype(np.uint8)
    ring = m.copy()
    ring[2, 3] = False
    assert (~m).sum() == 14 and ring.sum() == 20
    # the island stands: the hole around it has 14 pixels
    assert np.array_equal(R.subject_mask(labels, R.SUBJECT_BITS, False, 13)[0], m)
    assert R.subject_mask(labels, R.SUBJECT_BITS, False, 14)[0].all()
    # the subject first: the island is background by then, and the hole has 15
    assert np.array_equal(R.subject_mask(labels, R.SUBJECT_BITS, True, 0)[0], ring)
    assert np.array_equal(R.subject_mask(labels, R.SUBJECT_BITS, True, 14)[0], ring)
    assert R.subject_mask(labels, R.SUBJECT_BITS, True, 15)[0].all()


# ---- bytes and faces
def test_label_bytes_past_the_classes_are_background():
    labels = np.array([[[1, 19, 1], [200, 1, 255], [1, 1, 1]]], np.uint8)
    m = R.mask0(labels, R.DEFAULT_BITS)[0]
    assert np.array_equal(m, _art(["#.#", ".#.", "###"]))
    assert not R.mask0(np.arange(19, 256, dtype=np.uint8)[None, None], (1 << 19) - 1).any()
    assert R.mask0(np.arange(19, dtype=np.uint8)[None, None], (1 << 19) - 1).all()
    out = R.subject_mask(labels, R.DEFAULT_BITS, True, 9)
    assert out.dtype == np.uint8 and set(np.unique(out)) <= {0, 1}


def test_faces_do_not_touch():
    labels = np.zeros((2, 4, 6), np.uint8)
    labels[0, -1] = 1                                       # the full last row of face 0
    labels[1, 0] = 1                                        # the full first row of face 1, next to it in memory
    labels[1, 2, 0:2] = 1                                   # and a smaller component in face 1
    labels[0, 0, 0:5] = 1                                   # a smaller one in face 0
    out = R.subject_mask(labels, R.DEFAULT_BITS, True, 0)
    want = np.zeros_like(labels)
    want[0, -1] = want[1, 0] = 1
    assert np.array_equal(out, want)
    assert np.array_equal(R.subject_mask(labels[:1], R.DEFAULT_BITS, True, 0), want[:1])


# ---- constructor, defaults, CLI
def test_argument_checks():
    from face_crop_plus_amd import matte as M
    assert M.check_subject(None) is None and M.check_subject("largest") == "largest" and M.SUBJECTS == ("largest",)
    for bad in ("all", "Largest", "", True, 1, ["largest"]):
        with pytest.raises(ValueError, match="subject must be"):
            M.check_subject(bad)
    assert M.check_fill_holes(None) is None and M.check_fill_holes(1) == 1 and M.check_fill_holes(67108864) == 67108864
    assert M.check_fill_holes(np.int64(64)) == 64 and M.check_fill_holes(16.0) == 16 and M.MAX_FILL_HOLES == 8192 * 8192
    for bad in (0, -1, 67108865, True, False, 2.5, "64", [64], float("nan")):
        with pytest.raises(ValueError, match="fill_holes must be"):
            M.check_fill_holes(bad)
    assert M.SUBJECT_BITS == 2 == R.SUBJECT_BITS
    assert list(inspect.signature(M.subject_mask).parameters) == ["labels_dev", "class_bits", "keep_largest", "max_hole"]
    for text in ("subject=\"largest\"", "fill_holes=N", "m0(y,x)", "SMALLER", "8-connected", "4-connected"):
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
    assert params["subject"].default is None and params["fill_holes"].default is None
    for bad in ("all", True, 1):
        with pytest.raises(ValueError, match="subject must be"):
            Cropper(background=0, subject=bad)
    for bad in (0, 67108865, True, "64", 2.5):
        with pytest.raises(ValueError, match="fill_holes must be"):
            Cropper(background=0, fill_holes=bad)
    message = "subject / fill_holes need background or background_blur: without one they would do nothing"
    for kw in ({"subject": "largest"}, {"fill_holes": 64}, {"subject": "largest", "fill_holes": 64}):
        with pytest.raises(ValueError, match=message):
            Cropper(**kw)
    # the messages of before stand word for word
    with pytest.raises(ValueError, match="foreground / feather need background or background_blur: without one they would do nothing"):
        Cropper(feather=3, subject="largest")
    with pytest.raises(ValueError, match="refine needs background or background_blur: without one it would do nothing"):
        Cropper(refine=4, fill_holes=8)
    with pytest.raises(ValueError, match="background and background_blur exclude each other: the background is filled or blurred"):
        Cropper(background=0, background_blur=3.0, subject="largest")
    with pytest.raises(ValueError, match="refine and feather exclude each other: the soft edge is the guided filter's or the Gaussian's"):
        Cropper(background=0, refine=4, feather=3, fill_holes=8)
    with pytest.raises(ValueError, match="refine_eps needs refine: without it it would do nothing"):
        Cropper(background=0, refine_eps=64, subject="largest")
    with pytest.raises(ValueError, match="no alignment"):
        Cropper(background=0, subject="largest", det_threshold=None, landmarks=None)
    for kw in ({"background": 0, "subject": "largest"}, {"background_blur": 3.0, "fill_holes": 67108864},
               {"background": (1, 2, 3), "subject": "largest", "fill_holes": np.int64(8), "refine": 4, "foreground": [1, 17]}):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(**kw)


def test_cropper_resolves_the_defaults(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    c = Cropper(background=9, subject="largest")
    assert (c.subject, c.fill_holes, c.feather, c.refine, c.foreground_bits) == ("largest", None, 5, None, R.DEFAULT_BITS)
    c = Cropper(background_blur=2, fill_holes=64.0, foreground=[17, 1], refine=4)
    assert (c.subject, c.fill_holes, c.feather, c.foreground) == (None, 64, 0, (1, 17)) and type(c.fill_holes) is int
    c = Cropper(background=9)
    assert (c.subject, c.fill_holes) == (None, None)
    c = Cropper()
    assert (c.subject, c.fill_holes) == (None, None)
    assert "subject" in Cropper.__init__.__doc__ and "fill_holes" in Cropper.__init__.__doc__


def test_a_cropper_built_with_new_works_without_the_attributes(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import matte as M
    calls = []
    monkeypatch.setattr(M, "subject_mask", lambda *a: calls.append(("subject", a[1:])) or "cleaned")
    monkeypatch.setattr(M, "matte", lambda crops, labels, bits, *a, **k: calls.append(("matte", labels, bits)) or ("out", None))
    monkeypatch.setattr(M, "matte_blur", lambda crops, labels, bits, *a, **k: calls.append(("blur", labels, bits)) or ("out", None))
    monkeypatch.setattr(M, "refine_alpha", lambda crops, labels, bits, *a: calls.append(("refine", labels, bits)) or "alpha")
    c = Cropper.__new__(Cropper)
    c.background, c.background_blur, c.foreground_bits, c.feather = (0, 0, 0), None, R.ONE_17, 5
    assert "subject" not in vars(c) and "fill_holes" not in vars(c) and "refine" not in vars(c)
    assert c._matte_device("crops", "labels") == ("out", None)
    assert calls == [("matte", "labels", R.ONE_17)]                  # nothing new runs, the labels and the bits go through
    del calls[:]
    c.subject, c.fill_holes, c.refine, c.refine_eps = "largest", None, 4, 64
    c._matte_device("crops", "labels")
    assert calls == [("subject", (R.ONE_17, True, 0)), ("refine", "cleaned", 2), ("matte", "cleaned", 2)]
    del calls[:]
    c.subject, c.fill_holes, c.refine, c.background, c.background_blur, c.blur_taps = None, 16, None, None, 3.0, [1]
    c._matte_device("crops", "labels")
    assert calls == [("subject", (R.ONE_17, False, 16)), ("blur", "cleaned", 2)]


def test_cli_flags(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    plain = parse_args(base)
    assert "subject" not in plain and "fill_holes" not in plain
    assert parse_args(base + ["-su", "largest"])["subject"] == "largest"
    assert parse_args(base + ["--subject", "largest"])["subject"] == "largest"
    assert parse_args(base + ["-fh", "64"])["fill_holes"] == 64
    got = parse_args(base + ["-bg", "255,255,255", "-su", "largest", "--fill-holes", "16"])
    assert (got["background"], got["subject"], got["fill_holes"]) == ([255, 255, 255], "largest", 16)
    got = parse_args(base + ["-su", "largest", "-fh", "8"])
    assert {k: v for k, v in got.items() if k not in ("subject", "fill_holes")} == plain           # nothing else moves
    for bad in (["-su", "all"], ["-su"], ["-fh", "2.5"], ["-fh", "x"], ["-fh"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps({"subject": "largest", "fill-holes": 128, "background-blur": 3.0}))
    got = parse_args(base + ["-c", str(cfg)])
    assert (got["subject"], got["fill_holes"], got["background_blur"]) == ("largest", 128, 3.0)
    assert {k: v for k, v in got.items() if k not in ("subject", "fill_holes", "background_blur")} == plain


# ---- header, exports, ops
def test_header_exports_and_ops():
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import torch_ops as T
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    assert "#define FCP_ABI_VERSION 15" in hdr and N.ABI_VERSION == 15 and N.lib().fcp_abi_version() == 15
    for name in ("fcp_subject_mask_workspace_bytes", "fcp_subject_mask_u8"):
        assert name + "(" in hdr and name in N.EXPORTS and hasattr(N.lib(), name)
    assert "12 f h w bytes" in hdr
    ops = T.load()
    assert "subject_mask" in T.OPS and hasattr(ops, "subject_mask")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcp::subject_mask", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcp::subject_mask", "CPU")
    assert str(ops.subject_mask.default._schema) == \
        "fcp::subject_mask(Tensor labels, int class_bits, bool keep_largest, int max_hole) -> Tensor"
    with pytest.raises(RuntimeError):                      # no CPU kernel: a missing device is an error, not a fallback
        ops.subject_mask(torch.zeros(1, 4, 4, dtype=torch.uint8), 2, True, 0)


def test_c_exports_refuse_bad_arguments_before_any_device_call():
    import ctypes
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    lib = N.lib()
    one = ctypes.c_void_p(16)                       # never dereferenced: every call below fails its checks first

    def err():
        return lib.fcp_last_error().decode()

    def subject(f=1, h=4, w=4, bits=2, keep=1, hole=0, labels=one, out=one, ws=one, ws_bytes=1 << 20):
        return lib.fcp_subject_mask_u8(labels, f, h, w, bits, keep, hole, out, ws, ws_bytes, None)
    assert lib.fcp_subject_mask_workspace_bytes(3, 5, 7) == 3 * 5 * 7 * 12
    assert lib.fcp_subject_mask_workspace_bytes(0, 5, 7) == 0
    assert lib.fcp_subject_mask_workspace_bytes(65535, 8192, 8192) == 65535 * 8192 * 8192 * 12 <= 16 * 65535 * 8192 * 8192
    for bad in ((1, 8193, 1), (1, 1, 8193), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (65536, 1, 1)):
        assert lib.fcp_subject_mask_workspace_bytes(*bad) == -1
    for kw, text in (({"keep": 2}, "keep_largest"), ({"keep": -1}, "keep_largest"), ({"hole": -1}, "max_hole"),
                     ({"hole": 67108865}, "max_hole"), ({"bits": 1 << 19}, "class_bits"), ({"h": 8193}, "8192"), ({"w": 8193}, "8192"),
                     ({"h": 0}, "bad sizes"), ({"w": 0}, "bad sizes"), ({"f": -1}, "bad sizes"), ({"f": 65536}, "65535"),
                     ({"labels": None}, "null pointer"), ({"out": None}, "null pointer"), ({"ws": None}, "workspace"),
                     ({"ws_bytes": 191}, "workspace"), ({"ws": ctypes.c_void_p(8)}, "aligned")):
        assert subject(**kw) == -1, kw
        assert text in err() and err().startswith("subject_mask:"), (kw, err())
    assert subject(f=0, labels=None, out=None, ws=None, ws_bytes=0) == 0          # a no-op
