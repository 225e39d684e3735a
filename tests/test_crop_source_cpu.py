"""crop_source="original": the host steps (landmark mapping, level choice, matrix composition) against the contract of
INTEGRATION.md section 2c written out again here, and the command-line flag.  Host logic only."""
import inspect
import math

import numpy as np
import pytest

from face_crop_plus_amd import align


def _level(M, w, h):
    s = math.sqrt(abs(M[0][0] * M[1][1] - M[0][1] * M[1][0]))
    L = 0
    while s * 2.0 ** (L + 1) <= 1.0:
        L += 1
    while L > 0 and ((w >> L) < 1 or (h >> L) < 1):
        L -= 1
    return L


def _compose(M, w, h, L):
    sx, sy = (w >> L) / w, (h >> L) / h
    return np.array([[M[r][0] / sx, M[r][1] / sy, M[r][2] + M[r][0] * (0.5 / sx - 0.5) + M[r][1] * (0.5 / sy - 0.5)]
                     for r in range(2)])


def _sim(s, theta=0.3, tx=-120.25, ty=37.5):
    a, b = s * math.cos(theta), s * math.sin(theta)
    return np.array([[a, -b, tx], [b, a, ty]], np.float64)


def test_source_landmarks_formula_and_identity():
    rng = np.random.default_rng(0)
    lm = rng.uniform(0, 1024, (4, 5, 2)).astype(np.float32)
    w, h, ww, hh, left, top = 4001, 2999, 1024, 767, 0, 128
    got = align.source_landmarks(lm, w, h, ww, hh, left, top)
    x = ((lm[..., 0].astype(np.float64) - left + 0.5) * (w / ww) - 0.5).astype(np.float32)
    y = ((lm[..., 1].astype(np.float64) - top + 0.5) * (h / hh) - 0.5).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got[..., 0], x) and np.array_equal(got[..., 1], y)
    # per-face geometry (one image per face)
    per = align.source_landmarks(lm, [w] * 4, [h] * 4, [ww] * 4, [hh] * 4, [left] * 4, [top] * 4)
    assert np.array_equal(per, got)
    # no resize, no padding: bit-identical
    same = align.source_landmarks(lm, 1024, 1024, 1024, 1024, 0, 0)
    assert np.array_equal(same.view(np.uint32), lm.view(np.uint32))


@pytest.mark.parametrize("s,want", [(1.7, 0), (0.8, 0), (0.5000001, 0), (0.5, 1), (0.3, 1), (0.25, 2), (0.2, 2),
                                    (1 / 64, 6), (0.01, 6)])
def test_pyramid_level(s, want):
    M = _sim(s, theta=0.0)                                   # s exact: sqrt(s^2) without rotation rounding
    assert align.pyramid_level(M, 4000, 3000) == want == _level(M, 4000, 3000)


def test_pyramid_level_rotated_skewed_and_odd_sizes():
    rng = np.random.default_rng(1)
    for _ in range(200):
        M = rng.normal(0, 0.3, (2, 3))
        w, h = int(rng.integers(1, 5000)), int(rng.integers(1, 5000))
        assert align.pyramid_level(M, w, h) == _level(M, w, h)
    skew = np.array([[0.2, 0.05, 3.0], [-0.01, 0.11, 7.0]])
    assert align.pyramid_level(skew, 3001, 1999) == _level(skew, 3001, 1999) == 2      # s = 0.15


def test_pyramid_level_cap_keeps_one_pixel():
    M = _sim(1e-6, theta=0.0)
    assert align.pyramid_level(M, 40, 7) == 2                 # 7 >> 2 == 1, 7 >> 3 == 0
    assert align.pyramid_level(M, 1, 900) == 0
    assert align.pyramid_level(M, 2, 2) == 1
    assert align.pyramid_level(np.zeros((2, 3)), 100, 100) == 0   # degenerate (ok == 0) rows


def test_compose_level_zero_is_bit_identical():
    M = _sim(0.731, 0.4, -17.123456789, 1234.5)
    for w, h in [(4000, 3000), (4001, 2999), (1, 1)]:
        got = align.compose_level(M, w, h, 0)
        assert np.array_equal(got.view(np.uint64), M.view(np.uint64))


@pytest.mark.parametrize("w,h,L", [(4000, 3000, 1), (4001, 2999, 1), (4001, 2999, 3), (5000, 2800, 2), (37, 11, 3),
                                   (40, 7, 2)])
def test_compose_level_formula_and_geometry(w, h, L):
    rng = np.random.default_rng(w * 7 + L)
    for M in (_sim(0.21, 0.7, 55.5, -3.25), np.array([[0.2, 0.05, 3.0], [-0.01, 0.11, 7.0]])):
        got = align.compose_level(M, w, h, L)
        assert np.array_equal(got.view(np.uint64), _compose(M, w, h, L).view(np.uint64))
        # the level's pixel p_L = (p + 0.5) * s - 0.5 maps where the original's p does
        sx, sy = (w >> L) / w, (h >> L) / h
        p = rng.uniform(-50, max(w, h) + 50, (64, 2))
        pl = np.stack([(p[:, 0] + 0.5) * sx - 0.5, (p[:, 1] + 0.5) * sy - 0.5, np.ones(len(p))], 1)
        ref = np.concatenate([p, np.ones((len(p), 1))], 1) @ M.T
        assert np.abs(pl @ got.T - ref).max() < 1e-9


def test_cli_flag(tmp_path):
    from face_crop_plus_amd.__main__ import parse_args
    from face_crop_plus_amd.cropper import Cropper
    assert parse_args(["-i", str(tmp_path), "-cs", "original"])["crop_source"] == "original"
    assert parse_args(["-i", str(tmp_path), "--crop-source", "batch"])["crop_source"] == "batch"
    # not given: left out of the kwargs (they stay the reference parser's), so Cropper's default "batch" applies
    assert parse_args(["-i", str(tmp_path)]).get("crop_source", "batch") == "batch"
    assert inspect.signature(Cropper).parameters["crop_source"].default == "batch"
    with pytest.raises(SystemExit):
        parse_args(["-i", str(tmp_path), "-cs", "file"])
