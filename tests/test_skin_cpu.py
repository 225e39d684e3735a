"""Cropper(smooth_skin=S) without a GPU: the reference tests/skin_ref.py against the plain loops of its definition and
against the shared feather, the host's tables and their bounds, the argument checks of skin.py and of the Cropper, the
order of the finishing chain, the CLI flags, the header, exports and op schema, the C export's refusals, and what the
filter is for: the noise it removes from the skin of a synthetic portrait and the brows and lips it leaves alone."""
import contextlib
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


R = _load("skin_ref")
M = _load("matte_ref")


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    return N


# ---- the reference
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (9, 11)])
def test_reference_equals_the_plain_loops(h, w):
    rng = np.random.default_rng(h * 100 + w)
    y, x = np.mgrid[0:h, 0:w]
    crop = np.clip(np.stack([12 * x + 20, 14 * y + 30, 100 + 5 * x - 4 * y], -1) + rng.integers(-8, 9, (h, w, 3)), 0, 255).astype(np.uint8)
    labels = rng.integers(0, 19, (h, w)).astype(np.uint8)
    mixed = rng.integers(0, 65536, 256).astype(np.uint16)               # any table: not monotone, entries above ONE, zeros
    mixed[::5] = 0
    bits = R.DEFAULT_BITS | 1 << 2 | 1 << 12
    cases = [(R.blur_taps(0.5), R.range_lut(10), 256), (R.blur_taps(1.4), R.range_lut(64), 13), (R.blur_taps(2.0), mixed, 200),
             ([4096, 4096, 0, 4096], mixed, 256)]
    for taps, table, amount in cases:
        want = R.smooth_loops(crop, labels, bits, taps, table, amount)
        got = R.smooth_one(crop, labels, bits, taps, table, amount)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        off = R.mask01(labels, bits) == 0
        assert np.array_equal(got[off], crop[off])                       # what is not skin is byte-identical
    assert np.array_equal(R.smooth(crop[None], labels[None], bits, *cases[0][:])[0], R.smooth_one(crop, labels, bits, *cases[0]))
    assert R.smooth(crop[None][:0], labels[None][:0], bits, *cases[0]).shape == (0, h, w, 3)
    assert np.array_equal(R.smooth_one(crop, labels, bits, [0, 5, 5, 5], np.zeros(256, np.uint16), 256), crop)     # W == 0 copies


def test_reference_alpha_is_the_shared_feather():
    rng = np.random.default_rng(5)
    for h, w in ((1, 1), (2, 3), (7, 5), (33, 20)):
        labels = rng.integers(0, 19, (h, w)).astype(np.uint8)
        for bits in (R.DEFAULT_BITS, 1 << 0, M.DEFAULT_BITS):
            m = R.mask01(labels, bits)
            assert np.array_equal(255 * m, M.mask(labels, bits))
            assert np.array_equal(R.feather7(m), M.alpha_separable(M.mask(labels, bits), 7))
    assert R.FEATHER == M.TAPS[7]
    odd = np.array([[19, 31, 32, 255, 1]], np.uint8)                     # labels that never count, and one that does
    assert R.mask01(odd, 0xffffffff).tolist() == [[1, 1, 0, 0, 1]] and R.mask01(odd, R.DEFAULT_BITS).tolist() == [[0, 0, 0, 0, 1]]


# ---- the tables
def test_range_lut():
    from face_crop_plus_amd import skin as S
    assert (S.ONE, S.RANGE, S.MIN_RADIUS, S.MAX_RADIUS, S.DEFAULT_CLASSES, S.FEATHER) == (4096, 256, 3, 24, (1, 7, 8, 10, 14), 7)
    for strength in list(np.arange(1, 64.5, 0.5)) + [np.float32(7.5), np.int64(3)]:
        lut = S.range_lut(strength)
        assert lut.dtype == np.uint16 and lut.shape == (256,) and np.array_equal(lut, R.range_lut(float(strength))), strength
        assert lut[0] == 4096 and (np.diff(lut.astype(np.int64)) <= 0).all(), strength
    # pinned: floor(4096 exp(-d^2 / (2 S^2)) + 0.5), worked out by hand from the formula
    assert S.range_lut(1)[:6].tolist() == [4096, 2484, 554, 46, 1, 0] and not S.range_lut(1)[5:].any()
    assert S.range_lut(10)[[0, 5, 10, 20, 30, 40, 50]].tolist() == [4096, 3615, 2484, 554, 46, 1, 0]
    assert S.range_lut(64)[[0, 64, 128, 255]].tolist() == [4096, 2484, 554, 1]
    assert [S.amount_q8(a) for a in (0.05, 0.5, 1, 1.0)] == [13, 128, 256, 256] == [R.amount_q8(a) for a in (0.05, 0.5, 1, 1.0)]


def test_taps_keep_the_sums_in_32_bits():
    from face_crop_plus_amd import matte, skin as S
    for sigma in np.round(np.arange(0.5, 8.0001, 0.05), 2):
        taps = S.taps_of(float(sigma))
        assert taps == matte.blur_taps(float(sigma)) == R.blur_taps(float(sigma))
        r = len(taps) - 1
        assert S.MIN_RADIUS <= r <= S.MAX_RADIUS and max(taps) <= 4096
        s = R.spatial(taps)
        assert s.shape == (2 * r + 1, 2 * r + 1) and s[r, r] >= 1 and s.max() <= 4096        # W >= 1 at every skin pixel
        assert int(s.sum()) * 255 + int(s.sum()) // 2 < 2 ** 32
    assert [len(S.taps_of(v)) - 1 for v in (0.5, 3, 8)] == [3, 9, 24]
    worst = np.full((49, 49), 4096, np.int64)                            # any table within the entry's limits
    assert int(worst.sum()) * 255 + int(worst.sum()) // 2 < 2 ** 32 and np.array_equal(R.spatial([4096] * 25), worst)


# ---- argument checks
def test_checks_of_the_module():
    from face_crop_plus_amd import skin as S
    assert S.check_smooth_skin(None) is None
    for good, want in ((1, 1.0), (64, 64.0), (10.5, 10.5), (np.float32(2.5), 2.5), (np.int64(12), 12.0)):
        got = S.check_smooth_skin(good)
        assert got == want and type(got) is float, good
    for bad in (True, False, np.bool_(True), "8", 0.99, 64.5, 0, -8, float("nan"), float("inf"), (8,), [8.0]):
        with pytest.raises(ValueError, match="smooth_skin must be"):
            S.check_smooth_skin(bad)
    assert S.check_sigma(None) == 3.0 and S.check_sigma(0.5) == 0.5 and S.check_sigma(8) == 8.0 and type(S.check_sigma(8)) is float
    for bad in (True, "3", 0.49, 8.01, 0, float("nan"), float("inf"), [3.0]):
        with pytest.raises(ValueError, match="smooth_sigma must be"):
            S.check_sigma(bad)
    assert S.check_amount(None) == 1.0 and S.check_amount(0.05) == 0.05 and S.check_amount(1) == 1.0 and type(S.check_amount(1)) is float
    for bad in (True, "1", 0.049, 1.01, 0, -1, float("nan"), float("inf"), [0.5]):
        with pytest.raises(ValueError, match="smooth_amount must be"):
            S.check_amount(bad)
    assert S.check_classes(None) == R.DEFAULT_BITS == 0b100010110000010
    assert S.check_classes([1]) == 2 and S.check_classes((0, 18, 18)) == 1 | 1 << 18 and S.check_classes([np.int64(7), 8.0]) == 0x180
    for bad in ([], [19], [-1], [1.5], ["1"], [True], 5, None.__class__, "x"):
        with pytest.raises(ValueError, match="skin_classes must"):
            S.check_classes(bad)
    assert list(inspect.signature(S.skin_smooth).parameters) == ["crops_dev", "labels_dev", "class_bits", "taps", "lut_dev", "amount_q8"]
    assert list(inspect.signature(S.smooth).parameters) == ["crops_dev", "labels_dev", "strength", "sigma", "amount", "class_bits"]
    for text in ("smooth_skin=S", "fcp_skin_smooth_u8", "torch.ops.fcp.skin_smooth", "byte-identical", "section 2s", "matte.blur_taps",
                 "tests/skin_ref.py", "matte.feather_alpha(l, bits, 7)"):
        assert text in S.__doc__, text


def _no_device(*a, **k):
    raise AssertionError("device work before the argument check")


def test_cropper_checks_without_a_device(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    monkeypatch.setattr(CR.Cropper, "_init_models", _no_device)
    monkeypatch.setattr(torch.cuda, "set_device", _no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    params = inspect.signature(Cropper).parameters
    for name in ("smooth_skin", "smooth_sigma", "smooth_amount", "skin_classes"):
        assert params[name].default is None
    for bad in (True, "8", 0.99, 64.5, 0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="smooth_skin must be"):
            Cropper(smooth_skin=bad)
    with pytest.raises(ValueError) as err:
        Cropper(smooth_skin=10, det_threshold=None, landmarks=None)
    assert str(err.value) == ("smooth_skin needs aligned crops: it cannot be combined with det_threshold=None and landmarks=None (no "
                              "alignment), where the faces are the images themselves")
    for name, value in (("smooth_sigma", 3.0), ("smooth_amount", 0.5), ("skin_classes", [1])):
        with pytest.raises(ValueError) as err:
            Cropper(**{name: value})
        assert str(err.value) == f"{name} needs smooth_skin: without it it would do nothing"
    with pytest.raises(ValueError, match="smooth_sigma must be"):
        Cropper(smooth_skin=10, smooth_sigma=8.5)
    with pytest.raises(ValueError, match="smooth_amount must be"):
        Cropper(smooth_skin=10, smooth_amount=0)
    with pytest.raises(ValueError, match="skin_classes must name at least one class, each 0..18"):
        Cropper(smooth_skin=10, skin_classes=[19])
    with pytest.raises(ValueError, match="skin_classes must name at least one class"):
        Cropper(smooth_skin=10, skin_classes=[])
    given = {"det_threshold": None, "landmarks": (np.zeros((1, 5, 2)), np.array(["a"]))}
    for kw in ({"smooth_skin": 10}, {"smooth_skin": 1, "output_size": 1}, {"smooth_skin": 64.0, "smooth_sigma": 8, "smooth_amount": 0.05, **given},
               {"smooth_skin": np.float32(2.5), "skin_classes": (1, 10), "denoise": 8, "clahe": 2.0, "background": 0, "refine": 4}):
        with pytest.raises(AssertionError, match="device work"):
            Cropper(**kw)


def test_cropper_resolves_the_defaults_and_retouch_needs_smooth_skin(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    c = Cropper(smooth_skin=10)
    assert (c.smooth_skin, c.smooth_sigma, c.smooth_amount, c.skin_classes, c.skin_bits) == (10.0, 3.0, 1.0, (1, 7, 8, 10, 14), R.DEFAULT_BITS)
    assert type(c.smooth_skin) is float and c._needs_labels() is True and c._has_background() is False
    c = Cropper(smooth_skin=4, smooth_sigma=1, smooth_amount=0.5, skin_classes=[10, 1, 1])
    assert (c.smooth_sigma, c.smooth_amount, c.skin_classes, c.skin_bits) == (1.0, 0.5, (1, 10), 1 << 1 | 1 << 10)
    c = Cropper()
    assert c.smooth_skin is None and c.skin_bits == 0 and c._needs_labels() is False
    assert Cropper(background=0)._needs_labels() is True
    with pytest.raises(ValueError, match="Cropper.retouch needs a Cropper with smooth_skin"):
        c.retouch(np.zeros((1, 16, 16, 3), np.uint8), np.zeros((1, 16, 16), np.uint8))
    c = Cropper(smooth_skin=10)
    for bad in (np.zeros((1, 16, 16, 3), np.float32), np.zeros((16, 16, 3), np.uint8), np.zeros((1, 16, 16, 4), np.uint8)):
        with pytest.raises(ValueError, match="crops must be"):
            c.retouch(bad, np.zeros((1, 16, 16), np.uint8))
    for bad in (np.zeros((1, 16, 16), np.int32), np.zeros((1, 16, 15), np.uint8), np.zeros((2, 16, 16), np.uint8)):
        with pytest.raises(ValueError, match="labels must be"):
            c.retouch(np.zeros((1, 16, 16, 3), np.uint8), bad)
    assert c.retouch(np.zeros((0, 16, 16, 3), np.uint8), np.zeros((0, 16, 16), np.uint8)).shape == (0, 16, 16, 3)
    doc = Cropper.__init__.__doc__
    assert "``smooth_skin``" in doc and "skin.smooth" in doc and "section 2s" in doc and "byte-identical" in doc


def test_a_bare_cropper_reads_the_new_options_as_off():
    from face_crop_plus_amd import Cropper
    c = Cropper.__new__(Cropper)
    assert vars(c) == {}
    for name in ("smooth_skin", "smooth_sigma", "smooth_amount", "skin_classes"):
        assert getattr(c, name) is None, name
    assert c.skin_bits == 0 and type(c.skin_bits) is int and c._needs_labels() is False
    with open(os.path.join(ROOT, "face-crop-plus_amd", "cropper.py"), encoding="utf-8") as fh:
        assert "getattr(self" not in fh.read()


# ---- the chain
@pytest.fixture
def chain(monkeypatch):
    """A bare Cropper whose finishing steps are recorders: (calls, cropper).  A call is (step, open ranges, arguments)."""
    from face_crop_plus_amd import cropper as CR
    calls, open_ranges = [], []

    @contextlib.contextmanager
    def span(name):
        open_ranges.append(name)
        try:
            yield
        finally:
            open_ranges.pop()

    def recorder(step, result):
        return lambda *a, **k: calls.append((step, tuple(open_ranges), a, k)) or result
    monkeypatch.setattr(CR.trace, "range", span)
    monkeypatch.setattr(CR.denoising, "denoise", recorder("denoise", "denoised"))
    monkeypatch.setattr(CR.smoothing, "smooth", recorder("skin", "smoothed"))
    monkeypatch.setattr(CR.equalizing, "clahe", recorder("clahe", "equalised"))
    monkeypatch.setattr(CR.sharpening, "sharpen", recorder("sharpen", "sharpened"))
    monkeypatch.setattr(CR.Cropper, "_matte_device", lambda self, *a, **k: recorder("matte", ("matted", None))(*a, **k))
    c = CR.Cropper.__new__(CR.Cropper)
    c.strategy, c.output_format = "largest", "png"
    return calls, c


NAMES = np.array(["x.jpg", "y.jpg"])


def test_the_chain_runs_denoise_skin_clahe_sharpen_matte(chain):
    calls, c = chain
    c.denoise, c.clahe, c.clahe_grid, c.sharpen, c.sharpen_sigma, c.sharpen_threshold = 8.0, 2.0, 8, 1.0, 1.5, 0
    c.smooth_skin, c.smooth_sigma, c.smooth_amount, c.skin_bits = 10.0, 3.0, 0.5, 2
    c.background = (1, 2, 3)
    assert c._finish_crops("crops", "labels", NAMES, "out", skin_labels="skin labels") == "matted"
    assert calls == [("denoise", ("fcp:denoise",), ("crops", 8.0), {}),
                     ("skin", ("fcp:skin",), ("denoised", "skin labels", 10.0, 3.0, 0.5, 2), {}),
                     ("clahe", ("fcp:clahe",), ("smoothed", 2.0, 8), {}),
                     ("sharpen", ("fcp:sharpen",), ("equalised", 1.0, 1.5, 0), {}),
                     ("matte", ("fcp:matte",), ("sharpened", "labels"), {})]


def test_smooth_skin_alone_runs_no_matte_and_nothing_set_returns_the_input(chain):
    calls, c = chain
    crops = object()
    assert c._finish_crops(crops, None, NAMES, "out") is crops and calls == []
    assert c._finish_crops(crops, None, NAMES, "out", skin_labels="skin labels") is crops and calls == []     # the option is off
    c.smooth_skin, c.smooth_sigma, c.smooth_amount, c.skin_bits = 10.0, 3.0, 1.0, R.DEFAULT_BITS
    assert c._finish_crops(crops, None, NAMES, "out", skin_labels="skin labels") == "smoothed"
    assert [call[0] for call in calls] == ["skin"] and calls[0][2][0] is crops


def test_process_images_hands_the_matte_its_labels_only_with_a_background(monkeypatch):
    """The label map of one parse goes to the skin step always and to the matte only when a background mode is on."""
    from face_crop_plus_amd import cropper as CR
    seen = []
    faces_dev = torch.zeros(2, 4, 4, 3, dtype=torch.uint8)
    monkeypatch.setattr(CR.torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(CR.Cropper, "_locate", lambda self, *a: ([0, 1], np.zeros((2, 5, 2), np.float32), None, None, None))
    monkeypatch.setattr(CR.Cropper, "_align", lambda self, *a: (np.zeros((2, 4, 4, 3), np.uint8), faces_dev, [0, 1]))
    monkeypatch.setattr(CR.Cropper, "_parse", lambda self, *a: seen.append("parse") or ((None, None), "label map"))
    monkeypatch.setattr(CR.Cropper, "_finish_crops", lambda self, f, labels, n, o, skin_labels=None: seen.append((labels, skin_labels)) or f)
    monkeypatch.setattr(CR.Cropper, "save_groups", lambda self, *a: None)
    for background, want in ((None, (None, "label map")), ((0, 0, 0), ("label map", "label map"))):
        del seen[:]
        c = CR.Cropper.__new__(CR.Cropper)
        c.device, c.enh_model, c.par_model, c.smooth_skin, c.background = "cpu", None, object(), 10.0, background
        c._process_images([np.zeros((8, 8, 3), np.uint8)] * 2, NAMES, "out")
        assert seen == ["parse", want]


# ---- the CLI
def test_cli_flags(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    plain = parse_args(base)
    new = ("smooth_skin", "smooth_sigma", "smooth_amount", "skin_classes")
    assert not any(k in plain for k in new)
    got = parse_args(base + ["-sk", "10"])
    assert got["smooth_skin"] == 10.0 and type(got["smooth_skin"]) is float
    assert {k: v for k, v in got.items() if k != "smooth_skin"} == plain                 # nothing else moves
    got = parse_args(base + ["--smooth-skin", "2.5", "--smooth-sigma", "4", "--smooth-amount", "0.5", "--skin-classes", "[1, 10]"])
    assert [got[k] for k in new] == [2.5, 4.0, 0.5, [1, 10]]
    got = parse_args(base + ["-sk", "12", "-sks", "0.5", "-ska", "1", "-skc", "[7]", "-dn", "8"])
    assert [got[k] for k in new] == [12.0, 0.5, 1.0, [7]] and got["denoise"] == 8.0
    assert {k: v for k, v in got.items() if k not in new + ("denoise",)} == plain
    for bad in (["-sk", "strong"], ["-sk"], ["-sks", "wide"], ["-ska", "all"], ["-skc", "[1,"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)


# ---- the library and the op
def test_header_signatures_and_exports_agree(native):
    N = native
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    norm = lambda s: re.sub(r"[\s*]+", " ", s).strip()
    params = [re.sub(r"\s+", " ", p).strip() for p in re.search(r"int fcp_skin_smooth_u8\(([^)]*)\)", hdr).group(1).split(",")]
    assert params == ["const uint8_t* crops", "const uint8_t* labels", "int f", "int h", "int w", "uint32_t class_bits",
                      "const uint16_t* taps", "int radius", "const uint16_t* range_lut", "int amount_q8", "uint8_t* out",
                      "fcp_stream_t stream"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert N.SIGNATURES["fcp_skin_smooth_u8"] == [P, P, I, I, I, ctypes.c_uint32, P, I, P, I, P, P]
    assert "fcp_skin_smooth_u8" in N.EXPORTS and hasattr(N.lib(), "fcp_skin_smooth_u8")
    assert "#define FCP_ABI_VERSION 15" in hdr and N.ABI_VERSION == 15 and N.lib().fcp_abi_version() == 15
    doc = norm(hdr[hdr.index("Parser-guided skin smoothing"):hdr.index("int fcp_skin_smooth_u8(")])
    for phrase in ("min(range_lut[|g(p + o) - g(p)|], ONE)", "W == 0: b = c(p)", "no workspace, no float and no atomics", "must not overlap",
                   "out == crops included", 'a "skin_smooth:" message', "nothing is reflected", "byte-identical"):
        assert phrase in doc, phrase
    src = open(os.path.join(ROOT, "face-crop-plus_amd", "csrc", "fcp_skin.hip")).read()
    assert '#include "fcp_gray.h"' in src and "9798u" not in src                    # the gray is shared, not copied
    assert '#include "fcp_feather.h"' in src and "Tile<3, kTileW, kTileH>" in src                  # the feather is shared too
    assert "static_assert" in src and "(1ull << 32)" in src and '#include "fcp_crop_bytes.h"' in src and "(size_t)f * h * w" in src


def test_entry_point_refuses_before_any_device_work(native):
    """Null pointers everywhere: a call that got past its checks would fault, a refused one returns with its message."""
    lib = native.lib()
    ok = dict(f=1, h=64, w=64, bits=R.DEFAULT_BITS, radius=3, amount=256)
    good = (ctypes.c_uint16 * 25)(*([4096] + [1] * 24))
    big = (ctypes.c_uint16 * 25)(*([100] * 24 + [4097]))

    def call(crops=None, labels=None, table=None, out=None, taps=good, **change):
        a = dict(ok, **change)
        return lib.fcp_skin_smooth_u8(crops, labels, a["f"], a["h"], a["w"], a["bits"], taps, a["radius"], table, a["amount"], out, None)
    for change, word in (({"f": -1}, b"bad sizes"), ({"h": 0}, b"bad sizes"), ({"w": -3}, b"bad sizes"), ({"h": 8193}, b"8192"),
                         ({"w": 8193}, b"8192"), ({"f": 65536}, b"65535"), ({"bits": 1 << 19}, b"class at or above 19"),
                         ({"radius": 2}, b"radius must be 3..24"), ({"radius": 25}, b"radius must be 3..24"), ({"radius": -1}, b"radius"),
                         ({"taps": None}, b"null taps"), ({"taps": big, "radius": 24}, b"tap 24 is 4097"),
                         ({"amount": 0}, b"amount_q8 must be 1..256"), ({"amount": 257}, b"amount_q8 must be 1..256"),
                         ({}, b"null pointer"), ({"h": 1, "w": 1, "radius": 24, "amount": 1}, b"null pointer"),
                         ({"taps": big, "radius": 23}, b"null pointer")):
        assert call(**change) == -1, change
        assert word in lib.fcp_last_error() and lib.fcp_last_error().startswith(b"skin_smooth:"), (change, lib.fcp_last_error())
    one, two, far, further = ctypes.c_void_p(4096), ctypes.c_void_p(4098), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)   # never dereferenced
    for kw in ({"crops": one}, {"labels": one}, {"table": two}, {"out": one}, {"crops": one, "labels": far, "table": two},
               {"crops": one, "labels": far, "out": further}, {"labels": far, "table": two, "out": further}):
        assert call(**kw) == -1 and b"null pointer" in lib.fcp_last_error(), kw
    for kw in ({"crops": one, "out": one}, {"crops": one, "out": two}, {"crops": two, "out": one},
               {"crops": one, "out": ctypes.c_void_p(4096 + 64 * 64 * 3 - 1)}):
        assert call(labels=further, table=far, **kw) == -1, kw
        assert b"out must not overlap crops" in lib.fcp_last_error() and lib.fcp_last_error().startswith(b"skin_smooth:"), lib.fcp_last_error()
    for kw in ({"labels": one, "out": one}, {"labels": one, "out": ctypes.c_void_p(4096 + 64 * 64 - 1)}, {"labels": far, "out": ctypes.c_void_p((1 << 20) - 1)}):
        assert call(crops=further, table=two, **kw) == -1 and b"out must not overlap labels" in lib.fcp_last_error(), kw
    assert call(crops=one, labels=far, out=further, table=ctypes.c_void_p(4097)) == -1 and b"2-byte aligned" in lib.fcp_last_error()
    assert call(f=0) == 0 and call(f=0, h=1, w=8192, radius=24, amount=1) == 0          # f == 0: a no-op
    assert call(f=0, radius=2) == -1 and call(f=0, amount=0) == -1 and call(f=0, taps=None) == -1 and call(f=0, bits=1 << 19) == -1


def test_op_is_registered_and_refuses_cpu_tensors(native):
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    assert "skin_smooth" in T.OPS and hasattr(ops, "skin_smooth")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcp::skin_smooth", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcp::skin_smooth", "CPU")
    assert str(ops.skin_smooth.default._schema) == ("fcp::skin_smooth(Tensor crops, Tensor labels, int class_bits, int[] taps, "
                                                    "Tensor range_lut, int amount_q8) -> Tensor")
    with pytest.raises((NotImplementedError, RuntimeError)):                # no CPU kernel: a missing device is an error
        ops.skin_smooth(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 16, 16, dtype=torch.uint8), 2, [4096, 1, 1, 1],
                        torch.zeros(256, dtype=torch.uint16), 256)


# ---- what it is for
def test_the_reference_smooths_the_skin_and_leaves_brows_and_lips():
    """The synthetic portrait of tests/skin_ref.py at 96 x 80, noise of sigma 6, a label map that overshoots the skin by 2
    px into brow, lip and hair; S = 10, sigma 3.  Asserted: the error over flat skin falls, and the brow and lip pixels
    the label map wrongly calls skin move less than the flat skin's noise did.  Measured: the figures printed below, which
    README.md and INTEGRATION.md quote."""
    sc = R.scene()
    assert sc["clean"].shape == (96, 80, 3) and sc["flat"].sum() > 500 and sc["mislabelled"].sum() > 50
    before, after, moved, wrong_before, wrong_after = R.scene_figures(10, 3.0)
    print(f"flat skin: error std {before:.2f} before, {after:.2f} after; mislabelled brow and lip pixels move {moved:.2f} on average, "
          f"their error against the clean image goes from {wrong_before:.2f} to {wrong_after:.2f}")
    assert after < before and moved < before
    out = R.smooth_skin(sc["noisy"][None], sc["labels"][None], 10, 3.0)[0]
    off = R.mask01(sc["labels"], R.DEFAULT_BITS) == 0
    assert off.any() and np.array_equal(out[off], sc["noisy"][off])          # every pixel outside the mask is identical
    sentence = f"from {before:.2f} to {after:.2f} gray levels"
    moved_text = f"move by {moved:.2f} gray levels"
    readme = re.sub(r"\s+", " ", open(os.path.join(ROOT, "README.md")).read())
    integration = re.sub(r"\s+", " ", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    for doc in (readme, integration):
        assert sentence in doc and moved_text in doc, (sentence, moved_text)


def test_docs_say_what_it_is():
    readme = re.sub(r"\s+", " ", open(os.path.join(ROOT, "README.md")).read())
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`Cropper(smooth_skin=S)` / `-sk S`" in readme and "INTEGRATION.md section 2s" in readme
    assert "fcp_skin_smooth_u8" in readme and "torch.ops.fcp.skin_smooth" in readme
    assert integration.index("## 2r.") < integration.index("## 2s.") < integration.index("## 3.")
    section = re.sub(r"\s+", " ", integration[integration.index("## 2s."):integration.index("## 3.")])
    for phrase in ("`-sk S` / `--smooth-skin S`", "`-sks`", "`-ska`", "`-skc`", "min(rng[|g(p + o) - g(p)|], 4096)", "fcp_skin_smooth_u8",
                   "torch.ops.fcp.skin_smooth", "skin.range_lut", "tests/skin_ref.py", "One launch", "no workspace", "fcp:skin",
                   "denoise → skin → clahe → sharpen → matte", "Out of scope", "The ABI version stays 15", "tools/bench_skin.py",
                   "64 crops of 256 x 256", "Cropper.retouch"):
        assert phrase in section, phrase
    assert "bench_skin.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
