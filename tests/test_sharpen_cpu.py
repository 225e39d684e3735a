"""Cropper(sharpen=A) without a GPU: the reference tests/sharpen_ref.py against scipy's integer correlation, against the
same formula in float64 and against a true Gaussian; what the filter does to constants, edges and extremes; the argument
checks of sharpen.py and of the Cropper, the CLI flags, the header, exports and op schema, and the C export's refusals."""
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


R = _load("sharpen_ref")
SIGMAS = (0.5, 1.5, 4, 16)
RADII = {0.5: 3, 1.5: 5, 4: 12, 16: 48}
IDENTITY = [4096, 0, 0, 0]


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from face_crop_plus_amd import _native as N
    return N


def _noise(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (*shape, 3), dtype=np.uint8)


# ---- the reference
def test_taps_equal_the_hosts():
    from face_crop_plus_amd import matte as M
    from face_crop_plus_amd import sharpen as S
    for sigma in list(SIGMAS) + [float(s) for s in np.arange(0.5, 16.01, 0.25)]:
        taps = R.blur_taps(sigma)
        assert taps == M.blur_taps(sigma), sigma
        assert taps[0] + 2 * sum(taps[1:]) == 4096 and 3 <= len(taps) - 1 <= 48
    assert {s: len(R.blur_taps(s)) - 1 for s in SIGMAS} == RADII
    assert (S.TAP_SUM, S.MAX_RADIUS, S.DEFAULT_SIGMA) == (R.TAP_SUM, R.MAX_RADIUS, R.DEFAULT_SIGMA) == (4096, 48, 1.5)
    for amount in (0.05, 0.3, 1, 1.0, 2.5, 4):
        assert S.amount_q8(amount) == R.amount_q8(amount) == int(np.floor(256 * amount + 0.5))
    assert (S.amount_q8(0.05), S.amount_q8(1), S.amount_q8(4)) == (13, 256, 1024)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_blur_equals_scipys_integer_correlation(sigma):
    from scipy import ndimage
    taps = R.blur_taps(sigma)
    full = np.array(taps[::-1] + taps[1:], np.int64)              # mirrored: 2 r + 1 weights
    for k, shape in enumerate(((1, 1), (5, 3), (33, 70), (64, 64))):
        g = R.gray(_noise(shape, k))
        want = ndimage.correlate1d(ndimage.correlate1d(g, full, axis=1, mode="nearest"), full, axis=0, mode="nearest")
        got = R.blur(g, taps)
        assert got.dtype == np.int64 and np.array_equal(got, want), shape
        assert 0 <= got.min() and got.max() <= 255 << 24


@pytest.mark.parametrize("sigma", SIGMAS)
def test_output_is_within_one_level_of_float64(sigma):
    """Against the same formula with the same taps in float64.  The blur itself is exact (integers below 2^53), so the
    difference is the rounding of b8, at most half of 1/256 of a level times the amount A <= 4, that is 4 * 0.5 / 256, and
    the final rounding, at most 0.5: 0.5079 in all, below 1."""
    taps = R.blur_taps(sigma)
    worst = 0.0
    for k, (amount_q, threshold) in enumerate(((13, 0), (256, 3), (700, 0), (1024, 0), (1024, 40))):
        crop = _noise((33, 70), 10 + k)
        out = R.unsharp_parts(crop, taps, amount_q, threshold)["out"]
        err = float(np.abs(np.clip(R.unsharp_float(crop, taps, amount_q, threshold), 0, 255) - out).max())
        assert err <= 0.5 + (amount_q / 256) * 0.5 / 256 + 1e-9, (amount_q, threshold, err)
        worst = max(worst, err)
    print(f"sigma {sigma}: at most {worst:.4f} levels from float64")
    assert worst < 1


def test_blur_is_close_to_a_true_gaussian():
    """B / 2^24 against scipy's float64 Gaussian truncated at the same radius, on smoothed noise of 96 x 80 (uniform noise
    under a Gaussian of sigma 3: gray levels 96..157).  Measured maxima: 0.011, 0.018, 0.089 and 0.28 levels at sigma 0.5,
    1.5, 4 and 16 (the integer taps are floored, and the far ones are held at 1); asserted: twice those."""
    from scipy import ndimage
    g = np.rint(ndimage.gaussian_filter(np.random.default_rng(7).uniform(0, 255, (96, 80)), 3.0, mode="nearest")).astype(np.int64)
    assert g.max() - g.min() > 40
    measured = {0.5: 0.011, 1.5: 0.018, 4: 0.089, 16: 0.28}
    for sigma in SIGMAS:
        taps = R.blur_taps(sigma)
        want = ndimage.gaussian_filter(g.astype(np.float64), sigma, mode="nearest", truncate=(len(taps) - 1) / sigma)
        err = float(np.abs(R.blur(g, taps) / 2.0 ** 24 - want).max())
        print(f"sigma {sigma}: {err:.4f} levels from the Gaussian")
        assert err <= 2 * measured[sigma], (sigma, err)


# ---- what it does
def test_identity_taps_and_the_full_threshold_copy_the_crop():
    crop = _noise((33, 47), 3)
    for amount_q in (1, 256, 1024):
        assert np.array_equal(R.unsharp(crop[None], IDENTITY, amount_q, 0)[0], crop)
        for sigma in SIGMAS:
            assert np.array_equal(R.unsharp(crop[None], R.blur_taps(sigma), amount_q, 255)[0], crop)
    assert R.unsharp(crop[None][:0], IDENTITY, 256, 0).shape == (0, 33, 47, 3)
    assert np.array_equal(R.sharpen(crop[None], 1.0)[0], R.unsharp(crop[None], R.blur_taps(1.5), 256, 0)[0])


def test_a_constant_crop_is_unchanged_at_every_amount():
    for value in (0, 1, 77, 254, 255):
        for colour in ((value, value, value), (value, 255 - value, 30)):
            crop = np.broadcast_to(np.array(colour, np.uint8), (9, 11, 3)).copy()
            for sigma in SIGMAS:
                for amount_q in (1, 13, 256, 1024):
                    parts = R.unsharp_parts(crop, R.blur_taps(sigma), amount_q, 0)
                    assert (parts["d"] == 0).all() and np.array_equal(parts["out"], crop), (colour, sigma, amount_q)


def test_a_step_edge_gains_overshoot_on_both_sides():
    crop = np.full((16, 40, 3), 80, np.uint8)
    crop[:, 20:] = 170
    last = (0, 0)
    for amount in (0.25, 0.5, 1.0, 2.0):
        out = R.sharpen(crop[None], amount, 1.5)[0].astype(int)
        row = out[8, :, 0]
        assert (out[..., 0] == out[..., 1]).all() and (out[..., 0] == out[..., 2]).all()      # the gray stays gray
        assert (out == out[8]).all()                                                         # and the rows alike
        under, over = 80 - row[:20].min(), row[20:].max() - 170
        assert under > last[0] and over > last[1], (amount, under, over)                     # growing with the amount
        assert row[19] == row[:20].min() and row[20] == row[20:].max()                       # at the edge itself
        assert (row[:10] == 80).all() and (row[30:] == 170).all()                            # and nowhere far from it
        last = (under, over)
    # the coring keeps a small step as it is and a colour step moves all three channels by the same amount
    small = np.full((8, 40, 3), 100, np.uint8)
    small[:, 20:] = 104
    assert np.array_equal(R.sharpen(small[None], 4, 1.5, 4)[0], small)
    assert not np.array_equal(R.sharpen(small[None], 4, 1.5, 1)[0], small)
    colour = np.zeros((8, 40, 3), np.uint8)
    colour[:, :20], colour[:, 20:] = (120, 60, 30), (140, 160, 90)
    delta = R.sharpen(colour[None], 1.0)[0].astype(int) - colour
    assert (delta[..., 0] == delta[..., 1]).all() and (delta[..., 0] == delta[..., 2]).all() and delta.any()


def test_the_extremes_stay_within_int32():
    y, x = np.mgrid[0:24, 0:31]
    checker = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    for taps in (R.blur_taps(0.5), R.blur_taps(16), [2] + [0] * 47 + [2047], [0, 2048]):
        parts = R.unsharp_parts(checker, taps, 1024, 0)
        assert 0 <= parts["B"].min() and parts["B"].max() <= 255 << 24 < 2 ** 32
        assert np.abs(parts["d"]).max() <= 65280 and np.abs(1024 * parts["e"]).max() <= 66846720
        assert -2 ** 31 <= parts["v"].min() and parts["v"].max() < 2 ** 31
        assert set(np.unique(parts["out"]).tolist()) <= {0, 255}
    assert parts["v"].min() < 0 and (parts["v"] >> 16).max() > 255
    # the bounds are met: a white dot on black and a black dot on white under taps that leave the centre out
    dots = np.zeros((24, 40, 3), np.uint8)
    dots[:, 20:] = 255
    dots[12, 8], dots[12, 31] = 255, 0
    parts = R.unsharp_parts(dots, [0, 2048], 1024, 0)
    assert parts["d"][12, 8] == 65280 and parts["d"][12, 31] == -65280 and np.abs(parts["d"]).max() == 65280
    assert parts["v"].max() == (255 << 16) + 66846720 + 32768 < 2 ** 31 and parts["v"].min() == -66846720 + 32768 >= -2 ** 31
    assert parts["out"][12, 8].tolist() == [255] * 3 and parts["out"][12, 31].tolist() == [0] * 3


# ---- argument checks
def test_checks():
    from face_crop_plus_amd import sharpen as S
    assert S.check_sharpen(None) is None
    for good, want in ((0.05, 0.05), (4, 4.0), (1, 1.0), (np.float32(2.5), 2.5), (np.int64(2), 2.0)):
        got = S.check_sharpen(good)
        assert got == want and type(got) is float, good
    for bad in (True, False, np.bool_(True), "1", "strong", 0.049, 4.01, 0, -1, float("nan"), float("inf"), -float("inf"), (1,), [1.0]):
        with pytest.raises(ValueError, match="sharpen must be"):
            S.check_sharpen(bad)
    assert S.check_sigma(None) == 1.5 and type(S.check_sigma(None)) is float
    for good, want in ((0.5, 0.5), (16, 16.0), (np.float32(2.5), 2.5), (np.int64(3), 3.0)):
        got = S.check_sigma(good)
        assert got == want and type(got) is float, good
    for bad in (True, "1.5", 0.49, 16.5, 0, -2, float("nan"), float("inf"), (1.5,)):
        with pytest.raises(ValueError, match="sharpen_sigma must be"):
            S.check_sigma(bad)
    assert S.check_threshold(None) == 0
    for good in (0, 3, 255, np.int64(7), np.uint8(9)):
        got = S.check_threshold(good)
        assert got == int(good) and type(got) is int
    for bad in (True, False, "3", 3.0, -1, 256, float("nan"), (3,)):
        with pytest.raises(ValueError, match="sharpen_threshold must be"):
            S.check_threshold(bad)
    assert list(inspect.signature(S.unsharp).parameters) == ["crops_dev", "taps", "amount_q8", "threshold"]
    assert list(inspect.signature(S.sharpen).parameters) == ["crops_dev", "amount", "sigma", "threshold"]
    for text in ("sharpen=A", "fcp_unsharp_u8", "torch.ops.fcp.unsharp", "no colour fringes", "section 2q", "matte.blur_taps(S)",
                 "(B + 32768) >> 16", "sign(d) * max(|d| - (T << 8), 0)", "floor(256 A + 0.5)", "BORDER_REPLICATE"):
        assert text in S.__doc__, text


def test_cropper_checks_sharpen_without_a_device(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR

    def no_device(*a, **k):
        raise AssertionError("device work before the argument check")
    monkeypatch.setattr(CR.Cropper, "_init_models", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    params = inspect.signature(Cropper).parameters
    names = list(params)
    assert all(params[n].default is None for n in ("sharpen", "sharpen_sigma", "sharpen_threshold"))
    at = names.index("clahe_grid")
    assert names[at + 1:at + 5] == ["sharpen", "sharpen_sigma", "sharpen_threshold", "interpolation"]
    assert names[names.index("edge_shift") + 1:at] == ["denoise", "clahe"] and names[-2:] == ["interpolation", "min_sharpness"]
    for bad in (True, "1", 0.049, 4.01, 0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sharpen must be"):
            Cropper(sharpen=bad)
    for bad in (True, "1.5", 0.49, 16.5, float("nan")):
        with pytest.raises(ValueError, match="sharpen_sigma must be"):
            Cropper(sharpen=1.0, sharpen_sigma=bad)
    for bad in (True, "3", 3.0, -1, 256):
        with pytest.raises(ValueError, match="sharpen_threshold must be"):
            Cropper(sharpen=1.0, sharpen_threshold=bad)
    with pytest.raises(ValueError, match="sharpen_sigma needs sharpen"):
        Cropper(sharpen_sigma=1.5)
    with pytest.raises(ValueError, match="sharpen_threshold needs sharpen"):
        Cropper(sharpen_threshold=0)
    with pytest.raises(ValueError, match="sharpen needs aligned crops.*no alignment"):
        Cropper(sharpen=1.0, det_threshold=None, landmarks=None)
    given = {"det_threshold": None, "landmarks": (np.zeros((1, 5, 2)), np.array(["a"]))}
    for kw in ({"sharpen": 1.0}, {"sharpen": 0.05, "output_size": 1}, {"sharpen": 4, "sharpen_sigma": 16, "sharpen_threshold": 255,
                                                                      "output_size": (3, 40), **given},
               {"sharpen": np.float32(1.5), "denoise": 8, "clahe": 2.0, "background": 0, "refine": 4, "min_sharpness": 5.0}):
        with pytest.raises(AssertionError, match="device work"):                       # no minimum output_size
            Cropper(**kw)


def test_cropper_resolves_the_defaults_and_unsharp_needs_sharpen(monkeypatch):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import cropper as CR
    monkeypatch.setattr(CR.Cropper, "_init_models", lambda self: None)
    monkeypatch.setattr(CR.align, "resolve_warp_family", lambda *a, **k: "fixed")
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    c = Cropper(sharpen=1)
    assert (c.sharpen, c.sharpen_sigma, c.sharpen_threshold) == (1.0, 1.5, 0)
    assert type(c.sharpen) is float and type(c.sharpen_sigma) is float and type(c.sharpen_threshold) is int
    c = Cropper(sharpen=0.5, sharpen_sigma=3, sharpen_threshold=np.int64(4))
    assert (c.sharpen, c.sharpen_sigma, c.sharpen_threshold) == (0.5, 3.0, 4)
    c = Cropper()
    assert c.sharpen is None and c.sharpen_sigma is None and c.sharpen_threshold is None
    with pytest.raises(ValueError, match="Cropper.unsharp needs a Cropper with sharpen"):
        c.unsharp(np.zeros((1, 16, 16, 3), np.uint8))
    bare = Cropper.__new__(Cropper)                                                  # no attribute at all
    with pytest.raises(ValueError, match="Cropper.unsharp needs a Cropper with sharpen"):
        bare.unsharp(np.zeros((1, 16, 16, 3), np.uint8))
    for bad in (np.zeros((1, 16, 16, 3), np.float32), np.zeros((16, 16, 3), np.uint8), np.zeros((1, 16, 16, 4), np.uint8)):
        with pytest.raises(ValueError, match="crops must be"):
            Cropper(sharpen=1.0).unsharp(bad)
    assert Cropper(sharpen=1.0).unsharp(np.zeros((0, 16, 16, 3), np.uint8)).shape == (0, 16, 16, 3)
    doc = Cropper.__init__.__doc__
    for text in ("``sharpen``", "``sharpen_sigma``", "``sharpen_threshold``", "sharpen.sharpen", "section 2q", "no colour fringes",
                 "``Cropper.unsharp``"):
        assert text in doc, text


def test_cli_flags(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    base = ["-i", str(tmp_path)]
    plain = parse_args(base)
    assert not {"sharpen", "sharpen_sigma", "sharpen_threshold"} & set(plain)
    got = parse_args(base + ["-sh", "1"])
    assert got["sharpen"] == 1.0 and type(got["sharpen"]) is float
    assert {k: v for k, v in got.items() if k != "sharpen"} == plain                     # nothing else moves
    got = parse_args(base + ["--sharpen", "0.6", "--sharpen-sigma", "2.5", "--sharpen-threshold", "3"])
    assert (got["sharpen"], got["sharpen_sigma"], got["sharpen_threshold"]) == (0.6, 2.5, 3)
    assert type(got["sharpen_sigma"]) is float and type(got["sharpen_threshold"]) is int
    assert {k: v for k, v in got.items() if not k.startswith("sharpen")} == plain
    got = parse_args(base + ["-sh", "2", "-shs", "1", "-sht", "0", "-cl", "2", "-dn", "8"])
    assert (got["sharpen"], got["sharpen_sigma"], got["sharpen_threshold"], got["clahe"], got["denoise"]) == (2.0, 1.0, 0, 2.0, 8.0)
    for bad in (["-sh", "strong"], ["-sh"], ["--sharpen-sigma", "wide"], ["-sht", "2.5"], ["-sht"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)


# ---- the library and the op
def test_header_signatures_and_exports_agree(native):
    N = native
    hdr = open(os.path.join(ROOT, "include", "fcp_hip.h")).read()
    norm = lambda s: re.sub(r"[\s*]+", " ", s).strip()
    params = [re.sub(r"\s+", " ", p).strip() for p in re.search(r"int fcp_unsharp_u8\(([^)]*)\)", hdr).group(1).split(",")]
    assert params == ["const uint8_t* crops", "int f", "int h", "int w", "const uint16_t* taps", "int radius", "int amount_q8",
                      "int threshold", "uint8_t* out", "fcp_stream_t stream"]
    P, I = ctypes.c_void_p, ctypes.c_int
    assert N.SIGNATURES["fcp_unsharp_u8"] == [P, I, I, I, P, I, I, I, P, P]
    assert "fcp_unsharp_u8" in N.EXPORTS and hasattr(N.lib(), "fcp_unsharp_u8")
    assert "#define FCP_ABI_VERSION 15" in hdr and N.ABI_VERSION == 15 and N.lib().fcp_abi_version() == 15
    doc = norm(hdr[hdr.index("Unsharp-mask sharpening"):hdr.index("int fcp_unsharp_u8(")])
    for phrase in ("t[0] + 2 sum(t[1..r]) == 4096", "b8 = (B + 32768) >> 16", "e = sign(d) max(|d| - (T << 8), 0)",
                   "v_c = (c << 16) + A_q e + 32768", "out_c = v_c < 0 ? 0 : min(255, v_c >> 16)", "BORDER_REPLICATE",
                   "no workspace, no float and no atomics", "must not overlap", "out == crops included", 'an "unsharp:" message'):
        assert phrase in doc, phrase
    src = open(os.path.join(ROOT, "face-crop-plus_amd", "csrc", "fcp_sharpen.hip")).read()
    assert '#include "fcp_gray.h"' in src and "fcp_gray::gray_of" in src
    assert "9798" not in src and "19235" not in src                                     # the gray is shared, not copied
    assert "9798u * r + 19235u * g + 3735u * b + 16384u) >> 15" in open(os.path.join(ROOT, "face-crop-plus_amd", "csrc", "fcp_gray.h")).read()


def test_entry_point_refuses_before_any_device_work(native):
    """Null and made-up device pointers everywhere: a call that got past its checks would fault, a refused one returns with
    its message.  The taps are host memory, which the entry point reads: those are real."""
    lib = native.lib()
    ok = dict(f=1, h=64, w=64, radius=5, amount=256, threshold=0)
    good = R.blur_taps(1.5)

    def table(values):
        return (ctypes.c_uint16 * len(values))(*values)

    def call(crops=None, taps=table(good), out=None, **change):
        a = dict(ok, **change)
        return lib.fcp_unsharp_u8(crops, a["f"], a["h"], a["w"], taps, a["radius"], a["amount"], a["threshold"], out, None)
    wide = table([4096 - 2 * 48] + [1] * 48)
    for change, word in (({"f": -1}, b"bad sizes"), ({"h": 0}, b"bad sizes"), ({"w": -3}, b"bad sizes"), ({"h": 8193}, b"8192"),
                         ({"w": 8193}, b"8192"), ({"f": 65536}, b"65535"), ({"radius": 0}, b"radius must be 1..48"),
                         ({"radius": 49}, b"radius must be 1..48"), ({"radius": -1}, b"radius must be 1..48"),
                         ({"amount": 0}, b"amount_q8 must be 1..1024"), ({"amount": 1025}, b"amount_q8 must be 1..1024"),
                         ({"amount": -256}, b"amount_q8"), ({"threshold": -1}, b"threshold must be 0..255"),
                         ({"threshold": 256}, b"threshold must be 0..255"), ({"taps": None}, b"null pointer"),
                         ({"radius": 4}, b"must sum to 4096"), ({"taps": table([4095, 0, 0, 0]), "radius": 3}, b"must sum to 4096"),
                         ({"taps": table([4098, 0, 0, 0]), "radius": 3}, b"must sum to 4096"),
                         ({"taps": table([0] + [65535] * 48), "radius": 48}, b"must sum to 4096"),
                         ({}, b"null pointer"), ({"h": 1, "w": 1, "radius": 1, "taps": table([2048, 1024])}, b"null pointer"),
                         ({"taps": table(IDENTITY), "radius": 3, "amount": 1024, "threshold": 255}, b"null pointer"),
                         ({"taps": wide, "radius": 48, "h": 8192, "w": 8192}, b"null pointer")):
        assert call(**change) == -1, change
        assert word in lib.fcp_last_error() and lib.fcp_last_error().startswith(b"unsharp:"), (change, lib.fcp_last_error())
    one, two, far = ctypes.c_void_p(4096), ctypes.c_void_p(4098), ctypes.c_void_p(1 << 20)      # never dereferenced
    for kw in ({"crops": one}, {"out": one}, {"out": far}):
        assert call(**kw) == -1 and b"null pointer" in lib.fcp_last_error(), kw
    for kw in ({"crops": one, "out": one}, {"crops": one, "out": two}, {"crops": two, "out": one},
               {"crops": one, "out": ctypes.c_void_p(4096 + 64 * 64 * 3 - 1)}, {"crops": ctypes.c_void_p(4096 + 64 * 64 * 3 - 1), "out": one}):
        assert call(**kw) == -1, kw
        assert b"must not overlap" in lib.fcp_last_error() and lib.fcp_last_error().startswith(b"unsharp:"), lib.fcp_last_error()
    spare = table(good + [0])
    odd = ctypes.c_void_p(ctypes.addressof(spare) + 1)
    assert call(crops=one, out=far, taps=odd) == -1 and b"2-byte aligned" in lib.fcp_last_error()
    assert call(f=0) == 0 and call(f=0, h=1, w=8192, radius=48, taps=wide, amount=1024, threshold=255) == 0      # f == 0: a no-op
    # the checks come before the no-op
    assert call(f=0, h=0) == -1 and call(f=0, radius=49) == -1 and call(f=0, amount=0) == -1 and call(f=0, threshold=256) == -1
    assert call(f=0, radius=4) == -1 and b"must sum to 4096" in lib.fcp_last_error()
    assert call(f=0, taps=None) == -1 and b"null pointer" in lib.fcp_last_error()


def test_op_is_registered_and_refuses_cpu_tensors(native):
    from face_crop_plus_amd import torch_ops as T
    ops = T.load()
    assert "unsharp" in T.OPS and hasattr(ops, "unsharp")
    assert torch._C._dispatch_has_kernel_for_dispatch_key("fcp::unsharp", "CUDA")
    assert not torch._C._dispatch_has_kernel_for_dispatch_key("fcp::unsharp", "CPU")
    assert str(ops.unsharp.default._schema) == "fcp::unsharp(Tensor crops, int[] taps, int amount_q8, int threshold) -> Tensor"
    with pytest.raises((NotImplementedError, RuntimeError)):                # no CPU kernel: a missing device is an error
        ops.unsharp(torch.zeros(1, 16, 16, 3, dtype=torch.uint8), IDENTITY, 256, 0)


def test_docs_say_what_it_is():
    readme = re.sub(r"\s+", " ", open(os.path.join(ROOT, "README.md")).read())
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`Cropper(sharpen=A)` / `-sh A`" in readme and "INTEGRATION.md section 2q" in readme
    assert integration.index("## 2p.") < integration.index("## 2q.") < integration.index("## 3.")
    section = re.sub(r"\s+", " ", integration[integration.index("## 2q."):integration.index("## 3.")])
    for phrase in ("`-sh A` / `--sharpen A`", "`-shs S` / `--sharpen-sigma S`", "`-sht T` / `--sharpen-threshold T`",
                   "BORDER_REPLICATE", "(B + 32768) >> 16", "sign(d) * max(|d| - (T << 8), 0)", "floor(256 A + 0.5)",
                   "fcp_unsharp_u8", "torch.ops.fcp.unsharp", "matte.blur_taps", "tests/sharpen_ref.py", "One launch", "no workspace",
                   "no colour fringes", "The ABI version stays 15", "tools/bench_sharpen.py", "64 crops of 256 x 256"):
        assert phrase in section, phrase
    assert "bench_sharpen.py" in open(os.path.join(ROOT, "tools", "README.md")).read()
