"""The float32 warpAffine family on the device: byte-equal to the oracle's float restatement
(``oracle.align_ref.warp_affine_float32``), selectable through ``align``, ``Cropper`` and ``$FCP_WARP_FAMILY``."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu

BORDERS = ("constant", "replicate", "reflect", "wrap", "reflect_101")


def _warp(device, img, mats, out_size, border, ok=None, family="float32"):
    """Every matrix applied to the one image ``img`` (1,h,w,3)."""
    from face_crop_plus_amd import align
    f = len(mats)
    return align.warp_affine(torch.from_numpy(img).to(device), torch.zeros(f, dtype=torch.int32, device=device),
                             torch.from_numpy(np.asarray(mats, np.float64).reshape(f, 6)).to(device),
                             None if ok is None else torch.as_tensor(ok, dtype=torch.int32, device=device), None,
                             out_size, border, family).cpu().numpy()


def _float_ref(src, m, out_size, border):
    return A.warp_affine(src, np.asarray(m, np.float64).reshape(2, 3), out_size, border, variant="float32")


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("out_size", [(256, 256), (200, 300), (37, 29)])
def test_float_family_bit_exact(border, out_size, device):
    from face_crop_plus_amd import align
    rng = np.random.default_rng(100 * BORDERS.index(border) + out_size[1])
    n, h, w = 3, 96, 128
    imgs = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    pads = np.array([[0, 0, 0, 0], [8, 9, 0, 0], [0, 0, 13, 12]], np.int32)
    tgt = A.landmarks_target(out_size, 0.65)
    f = 14
    idx = rng.integers(0, n, f).astype(np.int32)
    lms = []
    for k in range(f):       # faces of assorted scale / rotation / position, some far outside the image
        th, s = rng.uniform(-1.2, 1.2), rng.uniform(0.15, 2.5)
        Rm = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) * s
        shift = rng.uniform(-60, 120, 2) if k < f - 2 else rng.uniform(400, 900, 2) * rng.choice([-1, 1], 2)
        lms.append(tgt @ Rm.T + shift + rng.normal(0, 1.5, (5, 2)))
    lms = np.stack(lms).astype(np.float32)
    crops, ok, mat = align.crop_align(torch.from_numpy(imgs).to(device), torch.from_numpy(idx), torch.from_numpy(lms),
                                      tgt, out_size, align.border_code(border), False, torch.from_numpy(pads),
                                      family="float32")
    crops, ok, mat = crops.cpu().numpy(), ok.cpu().numpy(), mat.cpu().numpy()
    assert ok.all()
    for k in range(f):
        t, b, l, r = pads[idx[k]]
        ref = _float_ref(imgs[idx[k]][t:h - b, l:w - r], mat[k], out_size, A.BORDER[border])
        assert crops[k].shape == ref.shape == (out_size[1], out_size[0], 3)
        assert np.array_equal(crops[k], ref), f"face {k}: max |d| {np.abs(crops[k].astype(int) - ref).max()}"


def test_identity_and_integer_shifts_reproduce_source(device):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (1, 48, 64, 3), dtype=np.uint8)
    mats = [[1, 0, 0, 0, 1, 0], [1, 0, 5, 0, 1, -3], [1, 0, -7, 0, 1, 9]]
    for b in range(5):
        out = _warp(device, img, mats, (64, 48), b)
        assert np.array_equal(out[0], img[0]), b
        assert np.array_equal(out[1][:45, 5:], img[0][3:, :59]), b          # dst(x, y) = src(x - 5, y + 3)
        assert np.array_equal(out[2][9:, :57], img[0][:39, 7:]), b          # dst(x, y) = src(x + 7, y - 9)
        for j, m in enumerate(mats):
            assert np.array_equal(out[j], _float_ref(img[0], m, (64, 48), b)), (b, j)


@pytest.mark.parametrize("border", range(5))
def test_tiny_source_slices(border, device):
    """1 x 1 and 2 x 2 un-padded slices of an 8 x 8 image (never the interior path / the interior path at its limit)."""
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (2, 8, 8, 3), dtype=np.uint8)
    pads = np.array([[3, 4, 3, 4], [3, 3, 3, 3]], np.int32)
    mats = np.array([[0.37, 0.11, 0.2, -0.11, 0.37, 0.3], [3.0, 0, 1.5, 0, 3.0, 1.5], [1.7, -0.4, -2.2, 0.4, 1.7, 0.9]])
    idx = torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.int32, device=device)
    from face_crop_plus_amd import align
    out = align.warp_affine(torch.from_numpy(imgs).to(device), idx, torch.from_numpy(np.concatenate([mats, mats])).to(device),
                            None, torch.from_numpy(pads).to(device), (13, 11), border, "float32").cpu().numpy()
    for k in range(6):
        t, b, l, r = pads[k // 3]
        assert np.array_equal(out[k], _float_ref(imgs[k // 3][t:8 - b, l:8 - r], mats[k % 3], (13, 11), border)), k


@pytest.mark.parametrize("border", range(5))
def test_coordinates_past_the_short_range_are_clamped(border, device):
    """Inverse maps that send output pixels beyond +-32768 source pixels: the float clamp before the int conversion."""
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, (1, 40, 56, 3), dtype=np.uint8)
    mats = [[0.001, 0, 0, 0, -0.002, 0],                          # sx = 1000 x, sy = -500 y
            [0.0007, 0.0003, 2.5, -0.0003, 0.0007, 31.7],
            [1, 0, 40000.5, 0, 1, -40000.25]]
    out = _warp(device, img, mats, (80, 72), border)
    for j, m in enumerate(mats):
        assert np.array_equal(out[j], _float_ref(img[0], m, (80, 72), border)), j


def test_ok_zero_rows_are_zero(device):
    rng = np.random.default_rng(1)
    img = rng.integers(1, 256, (1, 32, 32, 3), dtype=np.uint8)
    mats = [[1, 0, 0, 0, 1, 0], [0.9, 0.1, 1, -0.1, 0.9, 2], [1, 0, 0, 0, 1, 0]]
    out = _warp(device, img, mats, (32, 32), 1, ok=[1, 0, 1])
    assert not out[1].any() and out[0].all() and np.array_equal(out[0], img[0])


def test_both_boundaries_give_the_same_bits(device):
    from face_crop_plus_amd import align, torch_ops as T
    rng = np.random.default_rng(4)
    imgs = torch.from_numpy(rng.integers(0, 256, (2, 80, 96, 3), dtype=np.uint8)).to(device)
    pads = torch.tensor([[0, 0, 0, 0], [4, 3, 6, 2]], dtype=torch.int32)
    tgt = A.landmarks_target((64, 48), 0.65)
    lms = torch.from_numpy((tgt[None] * rng.uniform(0.5, 1.6, (6, 1, 1)) + rng.uniform(-10, 40, (6, 1, 2))).astype(np.float32))
    idx = torch.tensor([0, 1, 1, 0, 1, 0], dtype=torch.int32)
    res = {}
    prev = T.ENABLED
    for mode in (False, True):
        T.ENABLED = mode
        try:
            res[mode] = align.crop_align(imgs, idx, lms, tgt, (64, 48), 2, False, pads, family="float32")[0]
            torch.cuda.synchronize()
        finally:
            T.ENABLED = prev
    assert torch.equal(res[False], res[True])


def test_the_selector_changes_the_bytes(device):
    """On a generic rotation of a noise image the two families differ (by up to several grey levels; no bound asserted)."""
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (1, 64, 64, 3), dtype=np.uint8)
    m = [[0.93 * np.cos(0.4), -0.93 * np.sin(0.4), 11.3], [0.93 * np.sin(0.4), 0.93 * np.cos(0.4), -7.7]]
    fx = _warp(device, img, [m], (64, 64), 0, family="fixed")
    fl = _warp(device, img, [m], (64, 64), 0, family="float32")
    assert not np.array_equal(fx, fl)
    assert np.array_equal(fx[0], A.warp_affine(img[0], np.asarray(m), (64, 64), 0))
    assert np.array_equal(fl[0], _float_ref(img[0], m, (64, 64), 0))


def _device_mats(lms, tgt, device):
    from face_crop_plus_amd import align
    mat, ok = align.estimate_transform(torch.from_numpy(np.ascontiguousarray(lms, np.float32)).to(device),
                                       torch.from_numpy(np.ascontiguousarray(tgt, np.float32)).to(device))
    return mat.cpu().numpy().reshape(-1, 2, 3), ok.cpu().numpy()


def test_cropper_crop_align_follows_warp_family(monkeypatch, device):
    from face_crop_plus_amd import Cropper
    monkeypatch.delenv("FCP_WARP_FAMILY", raising=False)
    rng = np.random.default_rng(2)
    imgs = rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    c = Cropper(output_size=32, det_threshold=None, device="cuda:0", warp_family="float32")
    assert c.warp_family == "float32"
    th = 0.3
    rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    lm = np.stack([c.landmarks_target * 1.5 + 4, c.landmarks_target @ rot.T * 1.2 + 9]).astype(np.float32)
    mats, ok = _device_mats(lm, c.landmarks_target, device)
    assert ok.all()
    out = c.crop_align(imgs, None, [0, 1], lm)
    for k in range(2):
        assert np.array_equal(out[k], _float_ref(imgs[k], mats[k], (32, 32), 0)), k
    default = Cropper(output_size=32, det_threshold=None, device="cuda:0")
    assert default.warp_family == "fixed"
    out_fixed = default.crop_align(imgs, None, [0, 1], lm)
    for k in range(2):
        assert np.array_equal(out_fixed[k], A.warp_affine(imgs[k], mats[k], (32, 32), 0)), k
    assert not np.array_equal(out, out_fixed)


def test_process_dir_given_landmarks_with_env_float32(tmp_path, monkeypatch, device):
    from PIL import Image
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd.cropper import landmarks_target
    rng = np.random.default_rng(12)
    src = tmp_path / "in"
    src.mkdir()
    names, imgs = [], []
    for i in range(3):
        img = rng.integers(0, 256, (96, 80, 3), dtype=np.uint8)
        Image.fromarray(img).save(src / f"{i:03d}.png")
        names.append(f"{i:03d}.png")
        imgs.append(img)
    tgt = landmarks_target((48, 48), 0.65)
    lms = np.stack([tgt @ np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]).T * s + d
                    for t, s, d in [(0.2, 1.3, 5.5), (-0.5, 0.8, 20.25), (1.0, 1.7, 2.0)]]).astype(np.float32)
    monkeypatch.setenv("FCP_WARP_FAMILY", "float32")
    c = Cropper(output_size=48, landmarks=(lms, np.array(names)), det_threshold=None, padding="reflect", device="cuda:0")
    assert c.warp_family == "float32"
    out = tmp_path / "out"
    c.process_dir(str(src), str(out), desc=None)
    assert sorted(os.listdir(out)) == names
    mats, ok = _device_mats(lms, tgt, device)
    assert ok.all()
    for k, name in enumerate(names):
        got = np.asarray(Image.open(out / name).convert("RGB"))
        assert np.array_equal(got, _float_ref(imgs[k], mats[k], (48, 48), A.BORDER["reflect"])), name


def _fake_cv2(version, warp):
    mod = types.ModuleType("cv2")
    mod.__version__ = version
    mod.warpAffine = lambda img, M, dsize, borderMode=0: warp(img, M, dsize, borderMode)
    return mod


@pytest.mark.parametrize("border", ["constant", "reflect_101", "wrap"])
def test_auto_picks_the_family_cv2_runs(border, monkeypatch, device):
    from face_crop_plus_amd import align
    monkeypatch.setattr(align, "_AUTO_FAMILY", {})
    for variant in ("float32", "fixed"):
        calls = []

        def warp(img, M, dsize, b, variant=variant):
            calls.append(b)
            return A.warp_affine(img, M, dsize, b, variant=variant)
        monkeypatch.setitem(sys.modules, "cv2", _fake_cv2(f"test-{variant}", warp))
        assert align.resolve_warp_family("auto", border, device) == variant
        assert calls and set(calls) == {align.border_code(border)}
        n = len(calls)
        assert align.resolve_warp_family("auto", border, device) == variant      # cached per (version, border)
        assert len(calls) == n


def test_auto_warns_and_falls_back_when_neither_family_matches(monkeypatch, device):
    from face_crop_plus_amd import align, Cropper
    monkeypatch.setattr(align, "_AUTO_FAMILY", {})

    def perturbed(img, M, dsize, b):
        out = A.warp_affine(img, M, dsize, b).copy()
        out[3, 5, 1] ^= 4
        return out
    monkeypatch.setitem(sys.modules, "cv2", _fake_cv2("test-perturbed", perturbed))
    with pytest.warns(UserWarning, match="neither"):
        assert align.resolve_warp_family("auto", 0, device) == "fixed"
    # through the Cropper and the environment variable: a float-family cv2 selects the float kernel
    monkeypatch.setitem(sys.modules, "cv2", _fake_cv2("test-float-cropper", lambda img, M, dsize, b:
                                                      A.warp_affine(img, M, dsize, b, variant="float32")))
    monkeypatch.setenv("FCP_WARP_FAMILY", "auto")
    assert Cropper(output_size=32, det_threshold=None, padding="replicate", device="cuda:0").warp_family == "float32"
