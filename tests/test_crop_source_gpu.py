"""crop_source="original": the ragged INTER_AREA level builder and the ragged-source warps against the oracle's OpenCV
restatements, 64-bit blob offsets, the level-0 invariant against batch mode, process_dir end to end (detector and given
landmarks) against the oracle chain, and the sharpness the mode exists for."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A, batch_ref as B

pytestmark = pytest.mark.gpu

BORDERS = {"constant": 0, "replicate": 1, "reflect": 2, "wrap": 3, "reflect_101": 4}


# ---- the contract, restated for the oracle chain
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


def _oracle_crop(img, lm_src, tgt, size, border="constant", family="fixed", cache=None):
    """Steps 2-6 on the CPU: -> (crop or None, level)."""
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
    return A.warp_affine(lvl, _compose(M, w, h, L), size, BORDERS[border], variant=family), L


def _sim(s, theta, tx, ty):
    a, b = s * math.cos(theta), s * math.sin(theta)
    return np.array([[a, -b, tx], [b, a, ty]], np.float64)


# ---- kernels
def test_ragged_levels_match_resize_area(device):
    from face_crop_plus_amd import align
    from face_crop_plus_amd.batch import upload_sources
    rng = np.random.default_rng(11)
    shapes = [(37, 53), (129, 257), (300, 400), (64, 128), (3, 1001)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    blob, table = upload_sources(imgs, device)
    jobs, want, pos = [], [], 0
    for i, (h, w) in enumerate(shapes):
        for L in range(1, 7):
            if (h >> L) < 1 or (w >> L) < 1:
                break
            jobs.append((int(table[i, 0]), h, w, pos, h >> L, w >> L))
            want.append(B.resize_area_u8(imgs[i], w >> L, h >> L))
            pos += ((h >> L) * (w >> L) * 3 + 3) // 4 * 4
    assert any(j[4] == 1 or j[5] == 1 for j in jobs) and any(j[1] >> 6 == j[4] for j in jobs)      # 1-px levels, L = 6
    dst = torch.zeros(pos, dtype=torch.uint8, device=device)
    align.resize_area_ragged(blob, jobs, dst)
    got = dst.cpu().numpy()
    for j, ref in zip(jobs, want):
        n = j[4] * j[5] * 3
        assert np.array_equal(got[j[3]:j[3] + n].reshape(ref.shape), ref), j


def _warp_case(device):
    rng = np.random.default_rng(5)
    shapes = [(97, 131), (200, 150), (64, 80)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    from face_crop_plus_amd.batch import upload_sources
    blob, table = upload_sources(imgs, device)
    mats = [_sim(0.83, 0.37, 7.3, -4.6), _sim(0.45, -0.12, 3.25, 6.7), _sim(2.3, 0.21, -30.7, -41.3),
            _sim(1.1, -0.9, -40.4, 51.9), _sim(0.6, 0.05, -1.5, -2.5), np.zeros((2, 3))]
    img_of = [0, 1, 2, 1, 0, 2]
    ok = np.array([1, 1, 1, 1, 1, 0], np.int32)
    return imgs, blob, table, mats, img_of, ok


@pytest.mark.parametrize("family", ["fixed", "float32"])
@pytest.mark.parametrize("border", list(BORDERS))
@pytest.mark.parametrize("size", [(50, 38), (48, 64)])
def test_ragged_warp_matches_oracle(device, family, border, size):
    from face_crop_plus_amd import align
    imgs, blob, table, mats, img_of, ok = _warp_case(device)
    srcs = table[img_of]
    mat = torch.from_numpy(np.stack(mats).reshape(-1, 6)).to(device)
    crops = align.warp_affine_ragged(blob, srcs, mat, torch.from_numpy(ok).to(device), size, BORDERS[border], family)
    crops = crops.cpu().numpy()
    assert crops.shape == (len(mats), size[1], size[0], 3)
    for k, M in enumerate(mats):
        if ok[k]:
            ref = A.warp_affine(imgs[img_of[k]], M, size, BORDERS[border], variant=family)
            assert np.array_equal(crops[k], ref), (k, family, border)
        else:
            assert not crops[k].any()


def test_offsets_past_2gib(device):
    """A source (and a level source) beyond byte 2**31 of the blob gives the same bytes as the same source at offset 0."""
    from face_crop_plus_amd import align
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (301, 403, 3), dtype=np.uint8)
    far = (1 << 31) + 12345
    nbytes = img.size
    blob = torch.empty(far + nbytes + 4096, dtype=torch.uint8, device=device)
    src = torch.from_numpy(img.reshape(-1)).to(device)
    blob[:nbytes].copy_(src)
    blob[far:far + nbytes].copy_(src)
    mats = [_sim(0.7, 0.3, -20.0, 15.5), _sim(1.9, -0.4, -100.0, 80.0)]
    mat = torch.from_numpy(np.stack(mats * 2).reshape(-1, 6)).to(device)
    srcs = np.array([(0, 301, 403)] * 2 + [(far, 301, 403)] * 2, np.int64)
    for family in ("fixed", "float32"):
        crops = align.warp_affine_ragged(blob, srcs, mat, None, (64, 48), 4, family).cpu().numpy()
        assert np.array_equal(crops[:2], crops[2:])
        assert np.array_equal(crops[0], A.warp_affine(img, mats[0], (64, 48), 4, variant=family))
    n = 75 * 100 * 3
    dst = torch.zeros(2 * n, dtype=torch.uint8, device=device)
    align.resize_area_ragged(blob, [(0, 301, 403, 0, 75, 100), (far, 301, 403, n, 75, 100)], dst)
    d = dst.cpu().numpy()
    assert np.array_equal(d[:n], d[n:])
    assert np.array_equal(d[:n].reshape(75, 100, 3), B.resize_area_u8(img, 100, 75))
    del blob
    torch.cuda.empty_cache()


# ---- the align / batch API
@pytest.fixture(scope="module")
def retina_sd():
    from face_crop_plus_amd import weights
    return weights.generate_state_dict("retinaface")


def test_level0_matches_batch_mode(device, retina_sd):
    """Images already at resize_size (no resize, no padding): every face cropped at level 0 is byte-identical in both
    modes."""
    from face_crop_plus_amd import align
    from face_crop_plus_amd.batch import build_batch
    from face_crop_plus_amd.retinaface import RetinaFace
    rng = np.random.default_rng(21)
    imgs = [np.kron(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), np.ones((4, 4, 1), np.uint8)) for _ in range(3)]
    det = RetinaFace("all", 0.6).load(device, retina_sd)
    batch, _, pads, (blob, table) = build_batch(imgs, 256, "constant", device, keep_sources=True)
    assert not pads.any()
    lm, idx = det.predict(batch)
    assert len(idx) > 0
    src = align.source_landmarks(lm, 256, 256, 256, 256, 0, 0)
    assert np.array_equal(src, lm)
    tgt = A.landmarks_target((224, 224), 0.65)
    for family in ("fixed", "float32"):
        cb, okb, _ = align.crop_align(batch, torch.as_tensor(idx), torch.from_numpy(lm), tgt, (224, 224), 0, family=family)
        co, oko, mat_l, level = align.crop_align_sources(blob, table, idx, src, tgt, (224, 224), 0, family=family)
        assert np.array_equal(okb.cpu().numpy(), oko.cpu().numpy())
        at0 = (level == 0) & (oko.cpu().numpy() != 0)
        assert at0.any(), "no face at level 0"
        assert np.array_equal(cb.cpu().numpy()[at0], co.cpu().numpy()[at0])


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


def test_process_dir_original_matches_oracle(device, retina_sd, tmp_path):
    from PIL import Image
    from face_crop_plus_amd import Cropper, utils
    from face_crop_plus_amd.batch import batch_geometry, build_batch
    d = tmp_path / "big"
    d.mkdir()
    shapes = [(4000, 3000), (2800, 5000), (180, 200)]
    # threshold picked with the CPU oracle detector on these images: 43 faces at levels 0 to 3
    rs, size, thr = 320, (512, 512), 0.55
    names = _write_images(d, shapes, 8)
    out = tmp_path / "faces"
    c = Cropper(output_size=size, resize_size=rs, strategy="all", det_threshold=thr, batch_size=3, output_format="png",
                device="cuda:0", weights={"retinaface": retina_sd}, crop_source="original")
    assert c.crop_source == "original"
    c.process_dir(str(d), str(out), desc=None)
    imgs, _ = utils.read_images(names, str(d))
    batch, _, pads = build_batch(imgs, rs, "constant", device)
    lm_b, idx = c.det_model.predict(batch)
    tgt = A.landmarks_target(size, 0.65)
    written = set(os.listdir(out))
    nth, levels, cache, checked = {}, set(), {}, 0
    for k, i in enumerate(idx):
        h, w = imgs[i].shape[:2]
        ww, hh, pad, _, _ = batch_geometry(h, w, (rs, rs))
        src = _src_lm(lm_b[k], w, h, ww, hh, pad[2], pad[0])
        ref, L = _oracle_crop(imgs[i], src, tgt, size, cache=cache)
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
    assert checked == len(written)
    assert 0 in levels and max(levels) >= 1, f"levels exercised: {sorted(levels)}"
    # once more with a mask group: masks exist at the output size
    out2 = tmp_path / "masked"
    c2 = Cropper(output_size=size, resize_size=rs, strategy="all", det_threshold=thr, batch_size=3, output_format="png",
                 mask_groups={"any": list(range(19))}, device="cuda:0", weights={"retinaface": retina_sd, "bisenet": "generated"},
                 crop_source="original")
    c2.process_dir(str(d), str(out2), desc=None)
    masks = [os.path.join(dp, f) for dp, _, fs in os.walk(out2) if dp.endswith("_mask") for f in fs]
    assert masks
    for m in masks:
        assert np.asarray(Image.open(m)).shape[:2] == (size[1], size[0])
        face = m.replace("any_mask", "any")
        assert os.path.isfile(face)


def test_given_landmarks_original_matches_oracle(device, tmp_path):
    from PIL import Image
    from face_crop_plus_amd import Cropper, utils
    d = tmp_path / "given"
    d.mkdir()
    names = _write_images(d, [(1200, 1601), (480, 640)], 9)
    size = (96, 80)
    tgt = A.landmarks_target(size, 0.65)
    rng = np.random.default_rng(4)
    table = {}
    for name, scale, shift in [(names[0], 7.5, (400.0, 300.0)), (names[1], 1.3, (200.0, 150.0))]:
        five = tgt * scale + np.array(shift, np.float32)
        pts = rng.uniform(0, 400, (68, 2)).astype(np.float32)
        for sl, p in zip(utils.get_ldm_slices(5, 68), five):
            pts[sl] = p
        table[name] = pts.tolist()
    path = tmp_path / "lm.json"
    path.write_text(json.dumps(table))
    out = tmp_path / "faces"
    c = Cropper(output_size=size, landmarks=str(path), output_format="png", device="cuda:0", crop_source="original",
                padding="reflect_101")
    c.process_dir(str(d), str(out), desc=None)
    lms, fnames = utils.parse_landmarks_file(str(path))
    five = np.stack([lms[:, sl].mean(1) for sl in utils.get_ldm_slices(5, 68)], 1)     # as Cropper reduces them
    imgs, _ = utils.read_images(names, str(d))
    levels = set()
    for k, name in enumerate(fnames):
        i = names.index(str(name))
        ref, L = _oracle_crop(imgs[i], five[k], tgt, size, border="reflect_101")
        levels.add(L)
        got = np.asarray(Image.open(out / name).convert("RGB"))
        assert np.array_equal(got, ref), (name, L)
    assert levels == {0, 2}, levels


def _pattern(x, y, c):
    """Band-limited test signal: sinusoids with periods 6..12 source px, in [16, 239]."""
    v = 127.5
    for per, ang, amp in [(6.0, 0.3, 30.0), (7.5, 1.9, 25.0), (9.0, 2.6, 25.0), (12.0, 0.9, 30.0)]:
        v = v + amp * np.sin(2 * np.pi * (x * np.cos(ang) + y * np.sin(ang)) / per + 0.7 * c)
    return v


def test_original_is_sharper_than_batch(device):
    from face_crop_plus_amd import align
    from face_crop_plus_amd.batch import build_batch
    n = 4096
    ys, xs = np.mgrid[0:n, 0:n].astype(np.float64)
    img = np.stack([np.rint(_pattern(xs, ys, c)) for c in range(3)], -1).clip(0, 255).astype(np.uint8)
    del xs, ys
    size = (256, 256)
    tgt = A.landmarks_target(size, 0.65).astype(np.float64)
    M = _sim(0.8, 0.25, 0.0, 0.0)                            # crop pixels per source pixel: 0.8
    centre = M[:, :2] @ np.array([n / 2, n / 2])
    M[:, 2] = np.array([size[0] / 2, size[1] / 2]) - centre
    src = ((tgt - M[:, 2]) @ np.linalg.inv(M[:, :2]).T).astype(np.float32)[None]
    batch, _, pads, (blob, table) = build_batch([img], 1024, "constant", device, keep_sources=True)
    assert not pads.any()
    lm_b = (((src.astype(np.float64) + 0.5) * (1024 / n)) - 0.5).astype(np.float32)
    cb, okb, _ = align.crop_align(batch, torch.zeros(1, dtype=torch.int32), torch.from_numpy(lm_b), tgt.astype(np.float32),
                                  size, 0)
    co, oko, mat_l, level = align.crop_align_sources(blob, table, [0], src, tgt.astype(np.float32), size, 0)
    assert okb.item() == 1 and oko.item() == 1 and level[0] == 0
    Mo = mat_l.cpu().numpy().reshape(2, 3)
    assert np.abs(Mo - M).max() < 1e-3
    Moi = np.linalg.inv(np.vstack([Mo, [0, 0, 1]]))[:2]
    oy, ox = np.mgrid[0:size[1], 0:size[0]].astype(np.float64)
    u = Moi[0, 0] * ox + Moi[0, 1] * oy + Moi[0, 2]
    v = Moi[1, 0] * ox + Moi[1, 1] * oy + Moi[1, 2]
    want = np.stack([_pattern(u, v, c) for c in range(3)], -1)
    rms = {k: float(np.sqrt(np.mean((t.cpu().numpy()[0].astype(np.float64) - want) ** 2)))
           for k, t in (("batch", cb), ("original", co))}
    print("rms vs analytic pattern:", rms)
    assert rms["original"] <= 0.5 * rms["batch"], rms


def test_boundaries_give_equal_bytes(device, monkeypatch):
    from face_crop_plus_amd import align
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    imgs, blob, table, mats, img_of, ok = _warp_case(device)
    mat = torch.from_numpy(np.stack(mats).reshape(-1, 6)).to(device)
    okd = torch.from_numpy(ok).to(device)
    jobs = [(int(table[0, 0]), 97, 131, 0, 48, 65), (int(table[1, 0]), 200, 150, 48 * 65 * 3 + 4, 25, 18)]
    res = {}
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        outs = [align.warp_affine_ragged(blob, table[img_of], mat, okd, (40, 36), b, fam).cpu().numpy()
                for fam in ("fixed", "float32") for b in (0, 2)]
        dst = torch.zeros(48 * 65 * 3 + 4 + 25 * 18 * 3, dtype=torch.uint8, device=device)
        align.resize_area_ragged(blob, jobs, dst)
        res[enabled] = outs + [dst.cpu().numpy()]
    for a, b in zip(res[True], res[False]):
        assert np.array_equal(a, b)


def test_cropper_crop_source_argument(device):
    from face_crop_plus_amd import Cropper
    assert Cropper(output_size=32, det_threshold=None, device="cuda:0").crop_source == "batch"
    assert Cropper(output_size=32, det_threshold=None, device="cuda:0", crop_source="original").crop_source == "original"
    with pytest.raises(ValueError, match="crop_source"):
        Cropper(output_size=32, det_threshold=None, device="cuda:0", crop_source="file")
    with pytest.raises(ValueError, match="enh_threshold"):
        Cropper(output_size=32, det_threshold=None, enh_threshold=0.001, device="cuda:0", crop_source="original")
