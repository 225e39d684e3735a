"""Cropper(interpolation="cubic" | "lanczos4"): the INTER_CUBIC / INTER_LANCZOS4 warp kernels (batch and ragged sources)
byte for byte against tests/warp_interp_ref.py, both boundaries, process_dir and the given-landmark path against the oracle
chain, and the sharpness the option exists for."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A, batch_ref as B

pytestmark = pytest.mark.gpu

BORDERS = {"constant": 0, "replicate": 1, "reflect": 2, "wrap": 3, "reflect_101": 4}
METHODS = ("cubic", "lanczos4")


def _load():
    spec = importlib.util.spec_from_file_location("_warp_interp_ref", os.path.join(os.path.dirname(__file__),
                                                                                   "warp_interp_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()


def _sim(s, theta, tx, ty):
    a, b = s * math.cos(theta), s * math.sin(theta)
    return np.array([[a, -b, tx], [b, a, ty]], np.float64)


def _centred(s, theta, src_hw, out_wh, dx=0.0, dy=0.0):
    """Similarity with scale s (crop px per source px) mapping the source centre (+ dx, dy source px) to the crop centre."""
    M = _sim(s, theta, 0.0, 0.0)
    c = M[:, :2] @ np.array([(src_hw[1] - 1) / 2 + dx, (src_hw[0] - 1) / 2 + dy])
    M[:, 2] = np.array([(out_wh[0] - 1) / 2, (out_wh[1] - 1) / 2]) - c
    return M


def _images(rng):
    """Random and gradient content."""
    h, w = 40, 52
    yy, xx = np.mgrid[0:h, 0:w]
    grad = np.stack([(xx * 5) % 256, (yy * 7) % 256, (xx * 3 + yy * 4) % 256], -1).astype(np.uint8)
    return np.stack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8), grad,
                     rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)])


# paddings (t, b, l, r) of the 40 x 52 batch images: un-padded slices 40x52, 1x1, 3x5, 7x9
PADS = np.array([[0, 0, 0, 0], [20, 19, 30, 21], [10, 27, 4, 43], [1, 32, 40, 3]], np.int32)


def _faces(out_wh):
    """(img_idx, matrices, ok) over the batch: enlargement 0.25x to 6x, rotations, fractional shifts, faces partly and
    fully outside their source, a face with ok == 0."""
    sizes = [(40, 52), (1, 1), (3, 5), (7, 9)]
    idx, mats = [], []
    for i, hw in enumerate(sizes):
        for s, th, dx, dy in [(0.25, 0.1, 0.3, -0.2), (1.0, 0.0, 0.0, 0.0), (1.7, 0.45, 0.37, 0.61), (4.0, -0.3, 0.1, 0.2),
                              (6.0, 1.2, -0.45, 0.3), (2.3, 0.2, hw[1] * 0.6, -hw[0] * 0.4),
                              (1.3, -2.0, hw[1] * 3.0 + 20, hw[0] * 2.0 + 20)]:
            idx.append(i)
            mats.append(_centred(s, th, hw, out_wh, dx, dy))
    idx.append(0)
    mats.append(np.zeros((2, 3)))
    ok = np.ones(len(idx), np.int32)
    ok[-1] = 0
    return np.array(idx, np.int32), mats, ok


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("border", list(BORDERS))
@pytest.mark.parametrize("size", [(50, 38), (48, 64)])
def test_batch_kernel_matches_reference(device, method, border, size):
    from face_crop_plus_amd import align
    imgs = _images(np.random.default_rng(1))
    idx, mats, ok = _faces(size)
    crops = align.warp_affine(torch.from_numpy(imgs).to(device), torch.from_numpy(idx).to(device),
                              torch.from_numpy(np.stack(mats).reshape(-1, 6)).to(device), torch.from_numpy(ok).to(device),
                              torch.from_numpy(PADS).to(device), size, BORDERS[border], interpolation=method)
    want = R.warp_batch(imgs, idx, mats, ok, PADS, size, BORDERS[border], R.INTERP[method])
    got = crops.cpu().numpy()
    for k in range(len(idx)):
        assert np.array_equal(got[k], want[k]), (k, method, border)
    assert not got[-1].any()


def _ragged_case(device):
    from face_crop_plus_amd.batch import upload_sources
    rng = np.random.default_rng(2)
    shapes = [(40, 52), (1, 1), (3, 5), (7, 9), (97, 131)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    blob, table = upload_sources(imgs, device)
    return imgs, blob, table


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("border", list(BORDERS))
def test_ragged_kernel_matches_reference(device, method, border):
    from face_crop_plus_amd import align
    imgs, blob, table = _ragged_case(device)
    size = (50, 38)
    idx, mats, ok = _faces(size)
    idx = np.concatenate([idx, [4, 4]]).astype(np.int32)
    mats = mats + [_centred(0.6, 0.05, (97, 131), size, 1.5, -2.5), _centred(3.1, -0.7, (97, 131), size, 20.3, 10.6)]
    ok = np.concatenate([ok, [1, 1]]).astype(np.int32)
    crops = align.warp_affine_ragged(blob, table[idx], torch.from_numpy(np.stack(mats).reshape(-1, 6)).to(device),
                                     torch.from_numpy(ok).to(device), size, BORDERS[border], interpolation=method)
    got = crops.cpu().numpy()
    for k in range(len(idx)):
        want = (R.warp_affine_interp(imgs[idx[k]], mats[k], size, BORDERS[border], R.INTERP[method]) if ok[k]
                else np.zeros_like(got[k]))
        assert np.array_equal(got[k], want), (k, method, border)


def test_ragged_offsets_past_2gib(device):
    from face_crop_plus_amd import align
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (61, 83, 3), dtype=np.uint8)
    far = (1 << 31) + 12345
    blob = torch.empty(far + img.size + 4096, dtype=torch.uint8, device=device)
    src = torch.from_numpy(img.reshape(-1)).to(device)
    blob[:img.size].copy_(src)
    blob[far:far + img.size].copy_(src)
    mats = [_centred(0.7, 0.3, (61, 83), (64, 48)), _centred(3.9, -0.4, (61, 83), (64, 48), 4.2, -3.1)]
    mat = torch.from_numpy(np.stack(mats * 2).reshape(-1, 6)).to(device)
    srcs = np.array([(0, 61, 83)] * 2 + [(far, 61, 83)] * 2, np.int64)
    for method in METHODS:
        crops = align.warp_affine_ragged(blob, srcs, mat, None, (64, 48), 4, interpolation=method).cpu().numpy()
        assert np.array_equal(crops[:2], crops[2:])
        for k in range(2):
            assert np.array_equal(crops[k], R.warp_affine_interp(img, mats[k], (64, 48), 4, R.INTERP[method]))
    del blob
    torch.cuda.empty_cache()


def test_boundaries_give_equal_bytes(device, monkeypatch):
    from face_crop_plus_amd import align
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    imgs = torch.from_numpy(_images(np.random.default_rng(4))).to(device)
    size = (44, 36)
    idx, mats, ok = _faces(size)
    idx_d, mat_d, ok_d = (torch.from_numpy(idx).to(device), torch.from_numpy(np.stack(mats).reshape(-1, 6)).to(device),
                          torch.from_numpy(ok).to(device))
    pads = torch.from_numpy(PADS).to(device)
    _, blob, table = _ragged_case(device)
    res = {}
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        res[enabled] = [f(m, b).cpu().numpy() for m in METHODS for b in (0, 3)
                        for f in (lambda m, b: align.warp_affine(imgs, idx_d, mat_d, ok_d, pads, size, b, interpolation=m),
                                  lambda m, b: align.warp_affine_ragged(blob, table[idx], mat_d, ok_d, size, b,
                                                                        interpolation=m))]
    for a, b in zip(res[True], res[False]):
        assert np.array_equal(a, b)


def test_c_export_refuses_other_methods(device):
    import ctypes
    from face_crop_plus_amd import _native as N
    imgs = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=device)
    idx = torch.zeros(1, dtype=torch.int32, device=device)
    mat = torch.from_numpy(np.eye(2, 3).reshape(1, 6)).to(device)
    out = torch.empty((1, 4, 4, 3), dtype=torch.uint8, device=device)
    for bad in (0, 1, 3, 5, -1):
        rc = N.lib().fcp_warp_affine_u8_interp(N.ptr(imgs), 1, 8, 8, N.ptr(idx), N.ptr(mat), None, None, 1, 4, 4, 0, bad,
                                               N.ptr(out), N.stream_ptr())
        assert rc < 0 and b"interpolation" in N.lib().fcp_last_error()
    assert N.lib().fcp_warp_affine_u8_interp(N.ptr(imgs), 1, 8, 8, N.ptr(idx), N.ptr(mat), None, None, 1, 4, 4, 0, 2,
                                             N.ptr(out), N.stream_ptr()) == 0
    torch.cuda.synchronize()


# ---- Cropper: the oracle chain with the reference warp
def _src_lm(lm_b, w, h, ww, hh, left, top):
    lm = lm_b.astype(np.float64)
    return np.stack([(lm[..., 0] - left + 0.5) * (w / ww) - 0.5, (lm[..., 1] - top + 0.5) * (h / hh) - 0.5],
                    -1).astype(np.float32)


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


def _oracle_original(img, lm_src, tgt, size, method, border="constant", cache=None):
    M = A.estimate_transform(lm_src, tgt)
    if M is None:
        return None, None
    h, w = img.shape[:2]
    L = _level(M, w, h)
    key = (id(img), L)
    if L == 0:
        lvl = img
    elif cache is not None and key in cache:
        lvl = cache[key]
    else:
        lvl = B.resize_area_u8(img, w >> L, h >> L)
        if cache is not None:
            cache[key] = lvl
    return R.warp_affine_interp(lvl, _compose(M, w, h, L), size, BORDERS[border], R.INTERP[method]), L


def _write_images(d, shapes, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    names = []
    for i, (h, w) in enumerate(shapes):
        lo = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 3), dtype=np.uint8)
        img = np.kron(lo, np.ones((8, 8, 1), np.uint8))[:h, :w]
        img = (img.astype(np.int16) + rng.integers(-6, 7, img.shape)).clip(0, 255).astype(np.uint8)
        names.append(f"{i:03d}.png")
        Image.fromarray(img).save(d / names[-1], compress_level=1)
    return names


@pytest.fixture(scope="module")
def retina_sd():
    from face_crop_plus_amd import weights
    return weights.generate_state_dict("retinaface")


@pytest.fixture(scope="module")
def big_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("interp_big")
    return d, _write_images(d, [(4000, 3000), (2800, 5000), (180, 200)], 8)


@pytest.mark.parametrize("crop_source", ["batch", "original"])
@pytest.mark.parametrize("method", METHODS)
def test_process_dir_matches_oracle(device, retina_sd, big_dir, tmp_path, method, crop_source):
    from PIL import Image
    from face_crop_plus_amd import Cropper, utils
    from face_crop_plus_amd.batch import batch_geometry, build_batch
    d, names = big_dir
    rs, size, thr = 320, (128, 128), 0.55
    out = tmp_path / "faces"
    c = Cropper(output_size=size, resize_size=rs, strategy="all", det_threshold=thr, batch_size=3, output_format="png",
                device="cuda:0", weights={"retinaface": retina_sd}, crop_source=crop_source, interpolation=method)
    assert c.interpolation == method and c.warp_family == "fixed"
    c.process_dir(str(d), str(out), desc=None)
    imgs, _ = utils.read_images(names, str(d))
    batch, _, pads = build_batch(imgs, rs, "constant", device)
    lm_b, idx = c.det_model.predict(batch)
    batch_np = batch.cpu().numpy()
    tgt = A.landmarks_target(size, 0.65)
    written = set(os.listdir(out))
    nth, levels, cache, checked = {}, set(), {}, 0
    for k, i in enumerate(idx):
        if crop_source == "original":
            h, w = imgs[i].shape[:2]
            ww, hh, pad, _, _ = batch_geometry(h, w, (rs, rs))
            ref, L = _oracle_original(imgs[i], _src_lm(lm_b[k], w, h, ww, hh, pad[2], pad[0]), tgt, size, method,
                                      cache=cache)
        else:
            t, b, l, r = (int(v) for v in pads[i])
            M = A.estimate_transform(lm_b[k] - np.array([l, t], np.float32), tgt)
            ref, L = (None, None) if M is None else (
                R.warp_affine_interp(batch_np[i][t:rs - b, l:rs - r], M, size, 0, R.INTERP[method]), 0)
        if ref is None:
            continue
        levels.add(L)
        j = nth.get(i, 0)
        nth[i] = j + 1
        name = f"{names[i][:-4]}_{j}.png"
        assert name in written, name
        got = np.asarray(Image.open(out / name).convert("RGB"))
        assert np.array_equal(got, ref), (name, L)
        checked += 1
    assert checked == len(written) and checked > 0
    if crop_source == "original":
        assert max(levels) >= 1, f"levels exercised: {sorted(levels)}"


@pytest.mark.parametrize("crop_source", ["batch", "original"])
def test_given_landmarks_match_oracle(device, tmp_path, crop_source):
    from PIL import Image
    from face_crop_plus_amd import Cropper, utils
    d = tmp_path / "given"
    d.mkdir()
    names = _write_images(d, [(600, 801), (240, 320)], 9)
    size = (96, 80)
    tgt = A.landmarks_target(size, 0.65)
    rng = np.random.default_rng(4)
    table = {}
    for name, scale, shift in [(names[0], 2.5, (300.0, 200.0)), (names[1], 0.4, (100.0, 80.0))]:
        five = tgt * scale + np.array(shift, np.float32)
        pts = rng.uniform(0, 200, (68, 2)).astype(np.float32)
        for sl, p in zip(utils.get_ldm_slices(5, 68), five):
            pts[sl] = p
        table[name] = pts.tolist()
    path = tmp_path / "lm.json"
    path.write_text(json.dumps(table))
    lms, fnames = utils.parse_landmarks_file(str(path))
    five = np.stack([lms[:, sl].mean(1) for sl in utils.get_ldm_slices(5, 68)], 1)
    imgs, _ = utils.read_images(names, str(d))
    for method in METHODS:
        out = tmp_path / f"faces_{method}"
        c = Cropper(output_size=size, landmarks=str(path), output_format="png", device="cuda:0", crop_source=crop_source,
                    padding="reflect_101", interpolation=method)
        c.process_dir(str(d), str(out), desc=None)
        for k, name in enumerate(fnames):
            i = names.index(str(name))
            if crop_source == "original":
                ref, _ = _oracle_original(imgs[i], five[k], tgt, size, method, border="reflect_101")
            else:
                ref = R.warp_affine_interp(imgs[i], A.estimate_transform(five[k], tgt), size, 4, R.INTERP[method])
            got = np.asarray(Image.open(out / name).convert("RGB"))
            assert np.array_equal(got, ref), (name, method)
    # "linear" is the default: the same files as no argument
    files = {}
    for kw in ({}, {"interpolation": "linear"}):
        out = tmp_path / f"faces_linear_{len(kw)}"
        Cropper(output_size=size, landmarks=str(path), output_format="png", device="cuda:0", crop_source=crop_source,
                padding="reflect_101", **kw).process_dir(str(d), str(out), desc=None)
        files[len(kw)] = {n: np.asarray(Image.open(out / n)) for n in sorted(os.listdir(out))}
    assert files[0].keys() == files[1].keys() and files[0]
    assert all(np.array_equal(files[0][n], files[1][n]) for n in files[0])


def test_numpy_crop_align_honours_interpolation(device):
    from face_crop_plus_amd import Cropper
    rng = np.random.default_rng(6)
    imgs = rng.integers(0, 256, (2, 64, 80, 3), dtype=np.uint8)
    tgt = A.landmarks_target((48, 48), 0.65)
    lms = np.stack([tgt * 1.3 + np.float32([5.0, 3.0]), tgt * 0.8 + np.float32([20.5, 10.25])]).astype(np.float32)
    for method in ("linear",) + METHODS:
        c = Cropper(output_size=48, det_threshold=None, device="cuda:0", interpolation=method)
        got = c.crop_align(imgs, None, [0, 1], lms)
        for k in range(2):
            M = A.estimate_transform(lms[k], tgt)
            want = (A.warp_affine(imgs[k], M, (48, 48), 0) if method == "linear"
                    else R.warp_affine_interp(imgs[k], M, (48, 48), 0, R.INTERP[method]))
            assert np.array_equal(got[k], want), (method, k)


def _pattern(x, y, c):
    """Fine band-limited signal: sinusoids with periods 3..6 source px, in [16, 239]."""
    v = 127.5
    for per, ang, amp in [(3.0, 0.3, 30.0), (3.7, 1.9, 25.0), (4.5, 2.6, 25.0), (6.0, 0.9, 30.0)]:
        v = v + amp * np.sin(2 * np.pi * (x * np.cos(ang) + y * np.sin(ang)) / per + 0.7 * c)
    return v


def test_cubic_and_lanczos_are_sharper_than_linear(device):
    from face_crop_plus_amd import align
    n = 96
    ys, xs = np.mgrid[0:n, 0:n].astype(np.float64)
    img = np.stack([np.rint(_pattern(xs, ys, c)) for c in range(3)], -1).clip(0, 255).astype(np.uint8)
    size = (256, 256)
    M = _centred(4.0, 0.25, (n, n), size)                   # 4x enlargement
    images = torch.from_numpy(img)[None].to(device)
    idx = torch.zeros(1, dtype=torch.int32, device=device)
    mat = torch.from_numpy(M.reshape(1, 6)).to(device)

    def hf(a):
        a = a.astype(np.float64)
        return float(np.mean((a[1:] - a[:-1]) ** 2) + np.mean((a[:, 1:] - a[:, :-1]) ** 2))
    energy = {m: hf(align.warp_affine(images, idx, mat, None, None, size, 1, interpolation=m).cpu().numpy()[0])
              for m in ("linear",) + METHODS}
    print("high-frequency energy:", energy)
    assert energy["cubic"] > 1.1 * energy["linear"], energy
    assert energy["lanczos4"] > 1.1 * energy["linear"], energy
