"""Cropper(min_sharpness=...): the sharpness kernel's integer sums against tests/sharpness_ref.py (exact equality: odd
sizes, strips that do not divide H, the ok mask, the worst case of the accumulators), both boundaries, the entry point's
checks, Cropper.sharpness, and the filter end to end on given landmarks against the oracle's crops."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A, batch_ref as B

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 7), (5, 1), (2, 2), (3, 5), (17, 23), (64, 64), (112, 96), (256, 256), (257, 263)]
OK = np.array([1, 0, 1, 1, 0], np.int32)


def _load():
    spec = importlib.util.spec_from_file_location("_sharpness_ref", os.path.join(os.path.dirname(__file__), "sharpness_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()


@pytest.fixture(scope="module")
def cases():
    """shape -> (crops (5,H,W,3) uint8, reference sums (5,2) int64), computed once."""
    rng = np.random.default_rng(11)
    out = {}
    for h, w in SHAPES:
        crops = rng.integers(0, 256, (5, h, w, 3), dtype=np.uint8)
        out[(h, w)] = (crops, np.array([R.sums(c) for c in crops], np.int64))
    return out


def _checkerboard(f, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    return np.stack([board if k % 2 == 0 else 255 - board for k in range(f)])


@pytest.mark.parametrize("masked", [False, True], ids=["ok_none", "ok_mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_sums_equal_reference(device, cases, shape, masked):
    from face_crop_plus_amd import align
    crops, want = cases[shape]
    ok = torch.from_numpy(OK).to(device) if masked else None
    got = align.sharpness_sums(torch.from_numpy(crops).to(device), ok)
    assert got.dtype == torch.int64 and tuple(got.shape) == (5, 2) and got.device.type == "cuda"
    want = want * OK[:, None] if masked else want
    assert np.array_equal(got.cpu().numpy(), want), shape
    n = shape[0] * shape[1]
    assert align.sharpness_score(got, n).tolist() == [(n * int(b) - int(a) * int(a)) / (n * n) for a, b in want]


@pytest.mark.parametrize("f,h,w", [(3, 256, 256), (1, 1024, 1024)])
def test_checkerboard_does_not_overflow(device, f, h, w):
    """Every pixel has |L| = 1020, L*L = 1 040 400: the worst case of the per-lane and per-wave accumulators."""
    from face_crop_plus_amd import align
    crops = _checkerboard(f, h, w)
    want = np.array([R.sums(c) for c in crops], np.int64)
    assert (want[:, 0] == 0).all() and (want[:, 1] == h * w * 1040400).all()
    got = align.sharpness_sums(torch.from_numpy(crops).to(device))
    assert np.array_equal(got.cpu().numpy(), want)
    assert align.sharpness_score(got, h * w).tolist() == [1040400.0] * f


def test_boundaries_give_equal_sums_and_calls_repeat(device, cases, monkeypatch):
    from face_crop_plus_amd import align
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    ok = torch.from_numpy(OK).to(device)
    for shape in ((17, 23), (257, 263)):
        crops, want = cases[shape]
        dev = torch.from_numpy(crops).to(device)
        res = {}
        for enabled in (True, False):
            monkeypatch.setattr(T, "ENABLED", enabled)
            res[enabled] = [align.sharpness_sums(dev).cpu().numpy(), align.sharpness_sums(dev).cpu().numpy(),
                            align.sharpness_sums(dev, ok).cpu().numpy()]
        for enabled in (True, False):
            assert np.array_equal(res[enabled][0], want) and np.array_equal(res[enabled][1], want)
            assert np.array_equal(res[enabled][2], want * OK[:, None])


def test_unaligned_views_of_the_crops(device, cases):
    """A slice of a larger tensor starts at any byte: rows whose first dword straddles the crop's start."""
    from face_crop_plus_amd import align
    crops, want = cases[(17, 23)]
    flat = torch.zeros(crops.size + 8, dtype=torch.uint8, device=device)
    for lead in (1, 2, 3):
        flat[lead:lead + crops.size].copy_(torch.from_numpy(crops.reshape(-1)).to(device))
        view = flat[lead:lead + crops.size].view(crops.shape)
        assert view.data_ptr() % 4 == lead
        assert np.array_equal(align.sharpness_sums(view).cpu().numpy(), want), lead


def test_entry_point_refuses_bad_sizes_and_accepts_no_crops(device, monkeypatch):
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import align
    from face_crop_plus_amd import torch_ops as T
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        with pytest.raises(RuntimeError, match="bad sizes"):
            align.sharpness_sums(torch.zeros((1, 0, 4, 3), dtype=torch.uint8, device=device))
        with pytest.raises(RuntimeError, match="at most 8192 px wide"):
            align.sharpness_sums(torch.zeros((1, 1, 8193, 3), dtype=torch.uint8, device=device))
        empty = align.sharpness_sums(torch.zeros((0, 8, 8, 3), dtype=torch.uint8, device=device))
        assert empty.dtype == torch.int64 and tuple(empty.shape) == (0, 2)
        assert align.sharpness_score(empty, 64).shape == (0,)
    # the C entry point itself: a negative code and a message, nothing launched
    crops = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=device)
    sums = torch.full((1, 2), 7, dtype=torch.int64, device=device)
    lib = N.lib()
    assert lib.fcp_crop_sharpness_u8(N.ptr(crops), 1, 0, 4, None, N.ptr(sums), N.stream_ptr()) < 0
    assert b"bad sizes" in lib.fcp_last_error()
    assert lib.fcp_crop_sharpness_u8(N.ptr(crops), 1, 4, 8193, None, N.ptr(sums), N.stream_ptr()) < 0
    assert b"8192" in lib.fcp_last_error()
    assert lib.fcp_crop_sharpness_u8(N.ptr(crops), 0, 4, 4, None, N.ptr(sums), N.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert sums.cpu().tolist() == [[7, 7]]
    assert lib.fcp_crop_sharpness_u8(N.ptr(crops), 1, 4, 4, None, N.ptr(sums), N.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert sums.cpu().tolist() == [[0, 0]]


def test_cropper_sharpness_equals_reference_scores(device, cases):
    from face_crop_plus_amd import Cropper
    c = Cropper(output_size=48, det_threshold=None, device="cuda:0")
    assert c.min_sharpness is None
    for shape in ((1, 7), (17, 23), (112, 96), (257, 263)):
        crops, _ = cases[shape]
        got = c.sharpness(crops)
        assert got.dtype == np.float64 and got.shape == (5,)
        assert got.tolist() == [R.score(x) for x in crops], shape
    assert c.sharpness(_checkerboard(1, 64, 64)).tolist() == [1040400.0]
    assert c.sharpness(np.zeros((0, 8, 8, 3), np.uint8)).shape == (0,)
    with pytest.raises(ValueError, match="uint8"):
        c.sharpness(np.zeros((1, 8, 8, 3), np.float32))


# ---- end to end: given landmarks, the oracle's crops
BORDER = 4                                       # reflect_101


def _level(M, w, h):
    s = math.sqrt(abs(M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]))
    L = 0
    while s * 2.0 ** (L + 1) <= 1.0:
        L += 1
    while L > 0 and ((w >> L) < 1 or (h >> L) < 1):
        L -= 1
    return L


def _compose(M, w, h, L):
    if L == 0:
        return M
    sx, sy = (w >> L) / w, (h >> L) / h
    return np.array([[M[r, 0] / sx, M[r, 1] / sy, M[r, 2] + M[r, 0] * (0.5 / sx - 0.5) + M[r, 1] * (0.5 / sy - 0.5)]
                     for r in range(2)])


def _oracle_crop(img, five, tgt, size, crop_source):
    """The crop the default (linear, fixed-point) warp writes for one 5-point set, on the CPU."""
    M = A.estimate_transform(five, tgt)
    assert M is not None
    if crop_source == "batch":
        return A.warp_affine(img, M, size, BORDER)
    h, w = img.shape[:2]
    L = _level(M, w, h)
    lvl = img if L == 0 else B.resize_area_u8(img, w >> L, h >> L)
    return A.warp_affine(lvl, _compose(M, w, h, L), size, BORDER)


def _noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _smooth(h, w):
    """Low-frequency gradient: periods of hundreds of pixels, so the Laplacian is rounding noise of a level or two."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([127.5 + 100 * np.sin(xx / 90.0 + 0.4 * c) * np.cos(yy / 70.0 - 0.3 * c) for c in range(3)],
                    -1).round().astype(np.uint8)


def _run(d, out, **kw):
    from face_crop_plus_amd import Cropper
    c = Cropper(output_format="png", device="cuda:0", padding="reflect_101", **kw)
    c.process_dir(str(d), str(out), desc=None)
    return {n: (out / n).read_bytes() for n in sorted(os.listdir(out))} if out.is_dir() else {}


@pytest.mark.parametrize("crop_source", ["batch", "original"])
def test_given_landmarks_drop_the_blurry_file(device, tmp_path, crop_source):
    import io
    from PIL import Image
    from face_crop_plus_amd import utils
    d = tmp_path / "given"
    d.mkdir()
    imgs = {"sharp.png": _noise(np.random.default_rng(21), 240, 320), "smooth.png": _smooth(300, 260)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name, compress_level=1)
    size = (96, 80)
    tgt = A.landmarks_target(size, 0.65)
    rng = np.random.default_rng(4)
    table = {}
    for name, scale, shift in [("sharp.png", 1.3, (100.0, 60.0)), ("smooth.png", 1.6, (40.0, 90.0))]:
        five = tgt * scale + np.array(shift, np.float32)
        pts = rng.uniform(0, 200, (68, 2)).astype(np.float32)
        for sl, p in zip(utils.get_ldm_slices(5, 68), five):
            pts[sl] = p
        table[name] = pts.tolist()
    path = tmp_path / "lm.json"
    path.write_text(json.dumps(table))
    lms, fnames = utils.parse_landmarks_file(str(path))
    five = np.stack([lms[:, sl].mean(1) for sl in utils.get_ldm_slices(5, 68)], 1)     # as Cropper reduces them
    ref = {str(n): _oracle_crop(imgs[str(n)], five[k], tgt, size, crop_source) for k, n in enumerate(fnames)}
    score = {n: R.score(crop) for n, crop in ref.items()}
    print("reference scores:", score)
    # conditions on the inputs, from the reference alone
    assert score["smooth.png"] > 0 and score["sharp.png"] >= 4 * score["smooth.png"], score
    kw = dict(output_size=size, landmarks=str(path), crop_source=crop_source)
    plain = _run(d, tmp_path / "plain", **kw)
    assert sorted(plain) == ["sharp.png", "smooth.png"]
    for n in plain:
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(plain[n])).convert("RGB")), ref[n]), n
    mid = math.sqrt(score["sharp.png"] * score["smooth.png"])
    kept = _run(d, tmp_path / "mid", min_sharpness=mid, **kw)
    assert sorted(kept) == ["sharp.png"] and kept["sharp.png"] == plain["sharp.png"]
    assert _run(d, tmp_path / "zero", min_sharpness=0.0, **kw) == plain
    assert _run(d, tmp_path / "none", min_sharpness=2.0 * score["sharp.png"], **kw) == {}


def test_strategy_all_numbers_the_surviving_faces(device, tmp_path):
    import io
    from PIL import Image
    d = tmp_path / "all"
    d.mkdir()
    img = _smooth(260, 520)
    img[:, 260:] = _noise(np.random.default_rng(22), 260, 260)          # smooth left half, noise right half
    Image.fromarray(img).save(d / "two.png", compress_level=1)
    size = (64, 64)
    tgt = A.landmarks_target(size, 0.65)
    # the smooth face first: without the filter it is two_0 and the sharp one two_1
    rows = np.stack([tgt * 1.5 + np.float32([60.0, 70.0]), tgt * 1.5 + np.float32([340.0, 80.0])]).astype(np.float32)
    names = np.array(["two.png", "two.png"])
    ref = [A.warp_affine(img, A.estimate_transform(r, tgt), size, BORDER) for r in rows]
    score = [R.score(c) for c in ref]
    assert score[0] > 0 and score[1] >= 4 * score[0], score
    kw = dict(output_size=size, landmarks=(rows, names), strategy="all")
    plain = _run(d, tmp_path / "plain", **kw)
    assert sorted(plain) == ["two_0.png", "two_1.png"]
    for k in range(2):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(plain[f"two_{k}.png"])).convert("RGB")), ref[k]), k
    # the threshold is inclusive and the device's score is the reference's exactly: the sharp face's own score keeps it
    kept = _run(d, tmp_path / "kept", min_sharpness=score[1], **kw)
    assert sorted(kept) == ["two_0.png"] and kept["two_0.png"] == plain["two_1.png"]
