"""Cropper(edge_shift=N) on the GPU: the one launch against tests/mask_shift_ref.py byte for byte (sizes below, at and
around the 64 x 64 tile, radii up to the 64-pixel halo, patterns at every border, corner and seam, three faces a call with
a different pattern in each), separate faces, guard bytes around offset views, a poisoned output, repeated calls, both
boundaries, the matte kernels downstream of the shifted mask, Cropper.matte, and process_dir end to end on given
landmarks.  Equality everywhere, no tolerance.  Every call is one the entry point accepts."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(os.path.dirname(__file__), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


S = _load("mask_shift_ref")
R = _load("matte_refine_ref")
RB = _load("matte_blur_ref")
CR = _load("cutout_ref")
MR = R.MR
TH, TW = S.TILE_H, S.TILE_W
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 3), (7, 7), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1), (96, 80)]
LARGEST = sorted(SHAPES, key=lambda s: s[0] * s[1])[-3:]
BIG = (256, 256)
SMALL_SHIFTS = [s * r for r in (1, 2, 3, 5, 8) for s in (1, -1)]
LARGE_SHIFTS = [s * r for r in (63, 64) for s in (1, -1)]
FILL = (0, 177, 64)
_LABELS, _WANT = {}, {}


def _shifts(shape):
    if shape == BIG:
        return [64, -64]
    return SMALL_SHIFTS + (LARGE_SHIFTS if shape in LARGEST else [])


def _cases(shape):
    """(group, class_bits) of every call at a shape."""
    if shape == BIG:
        return [(S.GROUPS[0], S.DEFAULT_BITS)]
    return [(g, bits) for g in S.GROUPS for bits in (S.CLASS_BITS if "classes" in g else (S.DEFAULT_BITS,))]


def _labels(shape, group):
    """Three faces a call, a different pattern in each; made once."""
    key = (shape, group)
    if key not in _LABELS:
        rng = np.random.default_rng(1000 * shape[0] + shape[1])
        _LABELS[key] = S.labels_of(group, rng, *shape)
        _LABELS[key].setflags(write=False)
    return _LABELS[key]


def _want(shape, group, bits, shift):
    """The reference's output of a case.  All cases of a (shape, shift) go through the reference in one call, as the bits of
    one integer plane; computed once and shared by every test."""
    if (shape, shift) not in _WANT:
        cases = _cases(shape)
        planes = np.concatenate([S.mask0(_labels(shape, g), b) for g, b in cases])
        moved = S.shift_planes(planes, shift)
        moved.setflags(write=False)
        _WANT[(shape, shift)] = {case: moved[3 * k:3 * k + 3] for k, case in enumerate(cases)}
    return _WANT[(shape, shift)][(group, bits)]


def _call(labels, bits, shift, out):
    """The C entry point itself, on the pointers as given (views)."""
    from face_crop_plus_amd import _native as N
    f, h, w = labels.shape
    N.check(N.lib().fcp_mask_shift_u8(N.ptr(labels), f, h, w, bits, shift, N.ptr(out), N.stream_ptr()), "fcp_mask_shift_u8")


@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=lambda s: f"{s[0]}x{s[1]}")
def test_output_equals_reference(device, shape):
    from face_crop_plus_amd import matte as M
    checked = 0
    for group, bits in _cases(shape):
        lab_dev = torch.from_numpy(_labels(shape, group).copy()).to(device)
        for shift in _shifts(shape):
            want = _want(shape, group, bits, shift)
            for f in ((3,) if shape == BIG or abs(shift) > 8 else (3, 1)):
                out = M.shift_mask(lab_dev[:f], bits, shift)
                assert out.dtype == torch.uint8 and tuple(out.shape) == (f, *shape)
                got = out.cpu().numpy()
                assert np.array_equal(got, want[:f]), ((shape, group, hex(bits), shift, f), int((got != want[:f]).sum()))
                checked += 1
    cases = len(S.GROUPS) + 2
    assert checked == (2 if shape == BIG else cases * (2 * len(SMALL_SHIFTS) + (len(LARGE_SHIFTS) if shape in LARGEST else 0)))


def test_the_cases_are_not_trivial():
    """From the reference alone: the shifts differ, the halo crosses the seams, the border rule and the class bits decide."""
    assert LARGEST == [(TH + 1, TW + 1), (96, 80), (2 * TH + 1, 2 * TW + 1)]
    shape = (2 * TH + 1, 2 * TW + 1)
    g = S.GROUPS[0]
    m0 = S.mask0(_labels(shape, g), S.DEFAULT_BITS)
    assert 0.01 < m0[0].mean() < 0.03 and 0.45 < m0[1].mean() < 0.55 and 0.97 < m0[2].mean() < 0.99
    sparse = [_want(shape, g, S.DEFAULT_BITS, s)[0] for s in (1, 2, 3, 5, 8, 63)]
    dense = [_want(shape, g, S.DEFAULT_BITS, -s)[2] for s in (1, 2, 3, 5, 8, 63)]
    for a, b in zip(sparse, sparse[1:]):
        assert not (a & ~b).any() and (b & ~a).any()                  # every larger grow reaches pixels the one before did not
    for a, b in zip(dense, dense[1:]):
        assert not (b & ~a).any() and (a & ~b).any()
    pixels, holes, disc = _want(shape, S.GROUPS[2], S.DEFAULT_BITS, 5)
    assert pixels.sum() == 81 + 4 * 26 and pixels[3, 4] and not pixels[4, 4]       # a quarter disc at every corner
    pixels, holes, disc = _want(shape, S.GROUPS[2], S.DEFAULT_BITS, -5)
    assert not pixels.any() and (1 - holes).sum() == 81 + 4 * 26
    checker, seams, shoulders = _want(shape, S.GROUPS[3], S.DEFAULT_BITS, -3)
    lab = _labels(shape, S.GROUPS[3])
    assert not checker.any() and not seams.any()
    assert shoulders[-1].sum() == lab[2][-1].sum() - 6 > 0 and not shoulders[0].any()      # three columns a side, none from below
    grown = _want(shape, S.GROUPS[3], S.DEFAULT_BITS, 1)
    assert grown[0].all() and grown[1][TH - 2:TH + 1].all() and not grown[1][TH - 3, :TW - 1].any()
    three = [_want(shape, S.GROUPS[4], bits, 2) for bits in S.CLASS_BITS]
    assert not np.array_equal(three[0], three[1]) and not np.array_equal(three[1], three[2])
    full, empty, full2 = _want(shape, S.SEPARATION, S.DEFAULT_BITS, 64)
    assert full.all() and not empty.any() and full2.all()


@pytest.mark.parametrize("shift", [1, 8, 64, -1, -8, -64])
def test_faces_are_separate(device, shift):
    """Face 0 full, face 1 empty, face 2 full: the halo of a face never sees the rows of its neighbours in memory."""
    from face_crop_plus_amd import matte as M
    for shape in ((3, 3), (7, 7), (TH, TW), (TH + 1, TW + 1), (96, 80)):
        labels = _labels(shape, S.SEPARATION)
        assert labels[0].all() and not labels[1].any() and labels[2].all()
        got = M.shift_mask(torch.from_numpy(labels.copy()).to(device), S.SUBJECT_BITS, shift).cpu().numpy()
        assert np.array_equal(got, labels), (shape, shift)                    # all three are fixed points, in both directions
        # and the other way round: an empty face between two full ones stays empty, a full one between empty ones full
        inverse = (1 - labels).astype(np.uint8)
        got = M.shift_mask(torch.from_numpy(inverse).to(device), S.SUBJECT_BITS, shift).cpu().numpy()
        assert np.array_equal(got, inverse), (shape, shift)


@pytest.mark.parametrize("shape", [(7, 7), (TH + 1, TW + 1), (5, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bytes_offset_views_and_a_poisoned_output(device, shape):
    f, (h, w) = 3, shape
    n = f * h * w
    G = 64
    for group in (S.GROUPS[0], S.GROUPS[3]):
        labels = _labels(shape, group)
        for lead_in, lead_out in ((1, 3), (3, 1), (2, 2)):
            for shift in (1, -1, 5, -8) + ((64, -63) if shape in LARGEST else ()):
                # labels and out: views at odd byte offsets between 64 guard bytes each
                lbuf = torch.full((G + lead_in + n + G,), 0xA5, dtype=torch.uint8, device=device)
                lbuf[G + lead_in:G + lead_in + n].copy_(torch.from_numpy(labels.reshape(-1).copy()).to(device))
                lv = lbuf[G + lead_in:G + lead_in + n].view(f, h, w)
                for poison in (0x5A, 0x01):                                   # every byte of out is written, whatever it held
                    obuf = torch.full((G + lead_out + n + G,), poison, dtype=torch.uint8, device=device)
                    ov = obuf[G + lead_out:G + lead_out + n].view(f, h, w)
                    assert lv.data_ptr() % 4 == lead_in and ov.data_ptr() % 4 == lead_out
                    _call(lv, S.DEFAULT_BITS, shift, ov)
                    o = obuf.cpu().numpy()
                    what = (shape, group, lead_in, lead_out, shift, poison)
                    assert (o[:G + lead_out] == poison).all() and (o[G + lead_out + n:] == poison).all(), what
                    assert np.array_equal(o[G + lead_out:G + lead_out + n].reshape(f, h, w), _want(shape, group, S.DEFAULT_BITS, shift)), what
                l = lbuf.cpu().numpy()
                assert (l[:G + lead_in] == 0xA5).all() and (l[G + lead_in + n:] == 0xA5).all()
                assert np.array_equal(l[G + lead_in:G + lead_in + n], labels.reshape(-1))          # the input is untouched


def test_calls_repeat_and_boundaries_give_identical_tensors(device, monkeypatch):
    from face_crop_plus_amd import matte as M
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    shape = (96, 80)
    for group, bits in _cases(shape):
        ld = torch.from_numpy(_labels(shape, group).copy()).to(device)
        for shift in (2, -2, 8, -8, 64, -64):
            outs = [M.shift_mask(ld, bits, shift) for _ in range(3)]
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
            res = {}
            for enabled in (True, False):
                monkeypatch.setattr(T, "ENABLED", enabled)
                res[enabled] = M.shift_mask(ld, bits, shift)
            assert torch.equal(res[True], res[False]) and torch.equal(res[True], outs[0])
            assert np.array_equal(res[True].cpu().numpy(), _want(shape, group, bits, shift))
    hard = S.mask0(_labels(shape, group), bits).astype(np.uint8)
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        assert np.array_equal(M.shift_mask(ld, bits, 0).cpu().numpy(), hard)           # shift = 0 is legal here: the hard mask
        with pytest.raises(RuntimeError, match="shift must be"):
            M.shift_mask(ld, 2, 65)
        with pytest.raises(RuntimeError, match="shift must be"):
            M.shift_mask(ld, 2, -65)
        with pytest.raises(RuntimeError, match="class_bits"):
            M.shift_mask(ld, 1 << 19, 1)
        assert tuple(M.shift_mask(ld[:0], 2, -4).shape) == (0, 96, 80)
    ops = T.load()
    with pytest.raises(RuntimeError):
        ops.mask_shift(ld.float(), 2, 1)
    with pytest.raises(RuntimeError, match="labels"):
        ops.mask_shift(ld[0, 0], 2, 1)


# ---- downstream: the matte kernels on the shifted mask
def test_matte_kernels_on_the_shifted_mask_equal_the_references(device):
    from face_crop_plus_amd import matte as M
    shape = (96, 80)
    group = S.GROUPS[2]
    labels = _labels(shape, group)
    crops = MR.random_crops(np.random.default_rng(12), 3, *shape)
    cd, ld = torch.from_numpy(crops).to(device), torch.from_numpy(labels.copy()).to(device)
    taps = M.blur_taps(3.0)
    for shift in (-2, 3, -8):
        moved = _want(shape, group, S.DEFAULT_BITS, shift)
        assert not np.array_equal(moved, S.mask0(labels, S.DEFAULT_BITS))
        out = M.shift_mask(ld, S.DEFAULT_BITS, shift)
        assert np.array_equal(out.cpu().numpy(), moved)
        want, want_a = MR.matte(crops, moved, S.SUBJECT_BITS, 5, FILL)
        got, got_a = M.matte(cd, out, M.SUBJECT_BITS, 5, FILL, with_alpha=True)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_a.cpu().numpy(), want_a)
        bg = RB.background(crops, moved, S.SUBJECT_BITS, taps)[0]
        got, got_a = M.matte_blur(cd, out, M.SUBJECT_BITS, 5, taps, with_alpha=True)
        assert np.array_equal(got_a.cpu().numpy(), want_a) and np.array_equal(got.cpu().numpy(), RB.over(crops, want_a, bg))
        alpha = M.refine_alpha(cd, out, M.SUBJECT_BITS, 4, 64)
        assert np.array_equal(alpha.cpu().numpy(), R.alpha_of(crops, moved, S.SUBJECT_BITS, 4, 64))
        feathered = M.feather_alpha(out, M.SUBJECT_BITS, 5)
        assert np.array_equal(feathered.cpu().numpy(), want_a)
        assert np.array_equal(M.cutout(cd, feathered, None, taps).cpu().numpy(), CR.rgba(crops, want_a, taps))


def test_cropper_matte_equals_reference(device):
    from face_crop_plus_amd import Cropper
    shape = (96, 80)
    group = S.GROUPS[2]
    labels = _labels(shape, group).copy()                            # a writable array for torch
    crops = MR.random_crops(np.random.default_rng(12), 3, *shape)
    lm = (np.zeros((1, 5, 2), np.float32), np.array(["a"]))
    kw = dict(output_size=48, landmarks=lm, det_threshold=None, device="cuda:0", weights={"bisenet": "generated"})
    c = Cropper(background=FILL, edge_shift=-2, **kw)
    assert (c.edge_shift, c.feather) == (-2, 5) and c.par_model is not None
    moved = _want(shape, group, S.DEFAULT_BITS, -2)
    out, alpha = c.matte(crops, labels)
    want, want_a = MR.matte(crops, moved, S.SUBJECT_BITS, 5, FILL)
    assert np.array_equal(alpha, want_a) and np.array_equal(out, want)
    plain, plain_a = Cropper(background=FILL, **kw).matte(crops, labels)
    assert not np.array_equal(plain_a, alpha)
    # after subject / fill_holes, before refine and the blur's background sums
    SR = _load("subject_ref")
    c = Cropper(background_blur=3.0, fill_holes=5, edge_shift=3, refine=4, foreground=[1, 17], **kw)
    moved = S.shift_mask(SR.subject_mask(labels, S.ONE_17, False, 5), S.SUBJECT_BITS, 3)
    out, alpha = c.matte(crops, labels)
    want_a = R.alpha_of(crops, moved, S.SUBJECT_BITS, 4, 64)
    bg = RB.background(crops, moved, S.SUBJECT_BITS, RB.blur_taps(3.0))[0]
    assert np.array_equal(alpha, want_a) and np.array_equal(out, RB.over(crops, want_a, bg))
    # a shrink that erases the subject: the face is the fill, as a face without a foreground pixel is
    gone = np.zeros((1, *shape), np.uint8)
    gone[0, 40:45, 30:35] = 1
    out, alpha = Cropper(background=FILL, edge_shift=-3, **kw).matte(crops[:1], gone)
    assert not alpha.any() and (out == np.array(FILL, np.uint8)).all()


# ---- end to end: process_dir on given landmarks
SIGMA = 3.0
SIZE = (64, 64)


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for n in files:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def _cropper(landmarks, **kw):
    from face_crop_plus_amd import Cropper
    kw.setdefault("output_format", "png")
    return Cropper(output_size=SIZE, landmarks=landmarks, device="cuda:0", padding="reflect_101", batch_size=2,
                   weights={"bisenet": "generated"}, **kw)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """The recipe of tests/test_subject_gpu.py: three files with a landmark set each, their plain crops, the label maps the
    Cropper's own parser gives them (generated weights), and a foreground class set under which every crop has both
    subject and background and a shrink and a grow by 2 change its mask."""
    import itertools
    from PIL import Image
    d = tmp_path_factory.mktemp("shift_in")
    faces = np.load(os.path.join(os.path.dirname(__file__), "golden", "bisenet.npz"))["faces"]
    assert faces.shape == (3, *SIZE, 3)
    imgs = {f"{n}.png": face for n, face in zip("abc", faces)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name, compress_level=1)
    tgt = A.landmarks_target(SIZE, 0.65)
    landmarks = (np.stack([tgt, tgt, tgt]).astype(np.float32), np.array(sorted(imgs)))
    out = tmp_path_factory.mktemp("shift_plain")
    c = _cropper(landmarks)
    assert c.par_model is None
    c.process_dir(str(d), str(out), desc=None)
    plain = _tree(out)
    assert sorted(plain) == sorted(imgs)
    crops = np.stack([_pixels(plain[n]) for n in sorted(plain)])
    parser = _cropper(landmarks, background=0).par_model
    assert parser is not None
    labels = parser.parse(torch.from_numpy(crops).to("cuda:0"))[0].cpu().numpy()
    classes = sorted(set(np.unique(labels).tolist()))
    foreground = None
    for n in (1, 2, 3):
        for cand in itertools.combinations(classes, n):
            bits = sum(1 << k for k in cand)
            hard = S.mask0(labels, bits)
            moved = [S.shift_mask(labels, bits, s).astype(bool) for s in (-2, 2)]
            if all(m.sum() > 10 and (~m).sum() > 10 for m in hard) and all((a != b).any() for mv in moved for a, b in zip(hard, mv)):
                foreground = list(cand)
                break
        if foreground is not None:
            break
    assert foreground is not None, f"the generated parser gives no class set whose mask the shifts change: {classes}"
    return {"dir": d, "landmarks": landmarks, "plain": plain, "crops": crops, "labels": labels, "foreground": foreground}


MODES = {"fill": {"background": FILL}, "blur": {"background_blur": SIGMA}}


def _expected(scene, mode, shift):
    bits = sum(1 << c for c in scene["foreground"])
    moved = S.shift_mask(scene["labels"], bits, shift)
    out, alpha = MR.matte(scene["crops"], moved, S.SUBJECT_BITS, 5, FILL)
    if mode == "fill":
        return out
    return RB.over(scene["crops"], alpha, RB.background(scene["crops"], moved, S.SUBJECT_BITS, RB.blur_taps(SIGMA))[0])


_BEFORE = {}


def _mask_groups(scene):
    return {"fg": scene["foreground"], "all": list(range(19))}


def _before(scene, mode, root):
    """The files of a run of the mode without the option, made once per mode."""
    if mode not in _BEFORE:
        c = _cropper(scene["landmarks"], mask_groups=_mask_groups(scene), foreground=scene["foreground"], **MODES[mode])
        c.process_dir(str(scene["dir"]), str(root / "before"), desc=None)
        _BEFORE[mode] = _tree(root / "before")
    return _BEFORE[mode]


@pytest.mark.parametrize("mode,shift", [("fill", -2), ("blur", 2), ("fill", 2), ("blur", -2)])
def test_process_dir_files_and_masks(device, scene, tmp_path, mode, shift):
    """The written crops are labels -> mask_shift_ref -> the matte reference; the mask files are those of a run without."""
    before = _before(scene, mode, tmp_path)
    masks = [n for n in before if "_mask" + os.sep in n]
    assert len(masks) == 6
    names = sorted(scene["plain"])
    want = _expected(scene, mode, shift)
    c = _cropper(scene["landmarks"], mask_groups=_mask_groups(scene), foreground=scene["foreground"], edge_shift=shift, **MODES[mode])
    c.process_dir(str(scene["dir"]), str(tmp_path / "shifted"), desc=None)
    got = _tree(tmp_path / "shifted")
    assert sorted(before) == sorted(got)
    for n in masks:
        assert got[n] == before[n], n                                # byte-identical files
    for n in set(before) - set(masks):
        assert np.array_equal(_pixels(got[n]), want[names.index(os.path.basename(n))]), (mode, shift, n)
        assert not np.array_equal(_pixels(got[n]), _pixels(before[n])), n


def test_without_the_option_nothing_new_runs(device, scene, tmp_path, monkeypatch):
    from face_crop_plus_amd import matte as M

    def never(*a, **k):
        raise AssertionError("shift_mask without edge_shift")
    monkeypatch.setattr(M, "shift_mask", never)
    bits = sum(1 << c for c in scene["foreground"])
    want, _ = MR.matte(scene["crops"], scene["labels"], bits, 5, FILL)
    c = _cropper(scene["landmarks"], background=FILL, foreground=scene["foreground"])
    assert c.edge_shift is None
    c.process_dir(str(scene["dir"]), str(tmp_path / "bg"), desc=None)
    got = _tree(tmp_path / "bg")
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), want[k]), n
    c = _cropper(scene["landmarks"])
    c.process_dir(str(scene["dir"]), str(tmp_path / "plain"), desc=None)
    assert _tree(tmp_path / "plain") == scene["plain"]
    c = _cropper(scene["landmarks"], background=FILL, foreground=scene["foreground"], edge_shift=-2)
    with pytest.raises(AssertionError, match="without edge_shift"):
        c.matte(scene["crops"], scene["labels"])
