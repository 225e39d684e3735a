"""Cropper(subject=, fill_holes=) on the GPU: the connected-component launches against tests/subject_ref.py byte for byte
(sizes below and around the 64 x 32 tile, patterns that cross every seam, every option pair), a poisoned and a zeroed
workspace, repeated calls, guard bytes around offset views, both boundaries, the matte kernels downstream of the cleaned
mask, Cropper.matte, and process_dir end to end on given landmarks.  Equality everywhere, no tolerance."""
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


S = _load("subject_ref")
R = _load("matte_refine_ref")
RB = _load("matte_blur_ref")
MR = R.MR
TH, TW = S.TILE_H, S.TILE_W
SHAPES = [(1, 1), (1, 2), (2, 1), (3, 3), (5, 4), (7, 7), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 1, 2 * TW + 1),
          (96, 80)]
BIG = (256, 256)
BIG_GROUP = ("random41", "serpentine", "serpentine_t")
FILL = (0, 177, 64)
_LABELS, _WANT = {}, {}


def _options(shape):
    hw = shape[0] * shape[1]
    if shape == BIG:
        return [(True, hw)]
    return [(True, 0), (False, 1), (False, 5), (False, hw), (True, 5), (True, hw), (False, 0)]


def _groups(shape):
    return [BIG_GROUP] if shape == BIG else S.GROUPS


def _bits_of(group):
    return (S.DEFAULT_BITS, 1, S.ONE_17) if "classes" in group else (S.DEFAULT_BITS,)


def _labels(shape, group):
    """Three faces a call, a different pattern in each; made once."""
    key = (shape, group)
    if key not in _LABELS:
        rng = np.random.default_rng(1000 * shape[0] + shape[1])
        _LABELS[key] = S.labels_of(group, rng, *shape)
        _LABELS[key].setflags(write=False)
    return _LABELS[key]


def _want(shape, group, bits, keep, hole):
    """The reference's output of a case, computed once and shared by every test."""
    key = (shape, group, bits, keep, hole)
    if key not in _WANT:
        _WANT[key] = S.subject_mask(_labels(shape, group), bits, keep, hole)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _call(labels, bits, keep, hole, out, work=None):
    """The C entry point itself, on the pointers as given (views)."""
    from face_crop_plus_amd import _native as N
    f, h, w = labels.shape
    need = N.lib().fcp_subject_mask_workspace_bytes(f, h, w)
    assert need == 12 * f * h * w                                     # what include/fcp_hip.h states
    if work is None:
        work = torch.empty((need,), dtype=torch.uint8, device=labels.device)
    assert work.numel() >= need and work.data_ptr() % 16 == 0
    N.check(N.lib().fcp_subject_mask_u8(N.ptr(labels), f, h, w, bits, int(keep), hole, N.ptr(out), N.ptr(work), work.numel(),
                                        N.stream_ptr()), "fcp_subject_mask_u8")


@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=lambda s: f"{s[0]}x{s[1]}")
def test_output_equals_reference(device, shape):
    from face_crop_plus_amd import matte as M
    checked = 0
    for group in _groups(shape):
        lab_dev = torch.from_numpy(_labels(shape, group).copy()).to(device)
        for bits in _bits_of(group):
            for keep, hole in _options(shape):
                want = _want(shape, group, bits, keep, hole)
                for f in ((3,) if shape == BIG else (3, 1)):
                    out = M.subject_mask(lab_dev[:f], bits, keep, hole)
                    assert out.dtype == torch.uint8 and tuple(out.shape) == (f, *shape)
                    got = out.cpu().numpy()
                    assert np.array_equal(got, want[:f]), ((shape, group, hex(bits), keep, hole, f), int((got != want[:f]).sum()))
                    checked += 1
    assert checked == (1 if shape == BIG else 2 * 7 * (len(S.GROUPS) + 2))


def test_the_cases_are_not_trivial():
    """From the reference alone: the options differ, the seams are crossed, the tie and the diagonals decide."""
    shape = (2 * TH + 1, 2 * TW + 1)
    hw = shape[0] * shape[1]
    g = S.GROUPS[0]
    m0 = _want(shape, g, S.DEFAULT_BITS, False, 0)
    assert np.array_equal(m0, S.mask0(_labels(shape, g), S.DEFAULT_BITS))
    outs = [_want(shape, g, S.DEFAULT_BITS, keep, hole) for keep, hole in _options(shape)]
    for i in range(len(outs)):
        for j in range(i):
            assert not np.array_equal(outs[i][0], outs[j][0]), (i, j)              # the percolation map tells every option apart
    big = _want(shape, g, S.DEFAULT_BITS, True, 0)
    for face in big[[0, 2]]:                                                       # the subject spans all four tile quadrants
        ys, xs = np.nonzero(face)
        assert ys.min() < TH - 1 and ys.max() > TH and xs.min() < TW - 1 and xs.max() > TW
    assert np.array_equal(big[1], m0[1]) and np.array_equal(big[2], m0[2])         # checkerboard and serpentine: one component
    one = _want(shape, g, S.DEFAULT_BITS, False, 1)[1]
    assert one[1:-1, 1:-1].all() and np.array_equal(one[0], m0[1][0]) and np.array_equal(one[:, 0], m0[1][:, 0])
    t = S.GROUPS[3]
    tie, main, anti = _want(shape, t, S.DEFAULT_BITS, True, 0)
    assert tie[0, -1] and tie[1, -1] and tie.sum() == 2
    assert main.sum() == 4 and main[TH - 1, TW - 1] and main[TH, TW] and anti.sum() == 4 and anti[TH - 1, TW] and anti[TH, TW - 1]
    ring, nested, _ = _want(shape, S.GROUPS[4], S.DEFAULT_BITS, True, hw)
    assert ring[1:-1, 1:-1].all() and not ring[0].any() and np.array_equal(ring, nested)


@pytest.mark.parametrize("shape", [(7, 7), (TH + 1, TW + 1), (96, 80)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_workspace_contents_do_not_matter_and_calls_repeat(device, shape):
    hw = shape[0] * shape[1]
    for group in (S.GROUPS[0], S.GROUPS[4]):
        lab = torch.from_numpy(_labels(shape, group).copy()).to(device)
        for keep, hole in ((True, 0), (False, 5), (True, hw), (False, 0)):
            want = _want(shape, group, S.DEFAULT_BITS, keep, hole)
            for poison in (0xFF, 0x00):
                work = torch.full((12 * 3 * hw,), poison, dtype=torch.uint8, device=device)
                out = torch.full(lab.shape, 0x77, dtype=torch.uint8, device=device)
                _call(lab, S.DEFAULT_BITS, keep, hole, out, work)
                assert np.array_equal(out.cpu().numpy(), want), (shape, group, keep, hole, poison)
            work = torch.empty((12 * 3 * hw,), dtype=torch.uint8, device=device)
            outs = []
            for _ in range(3):                                                      # the same workspace, as the last call left it
                out = torch.empty_like(lab)
                _call(lab, S.DEFAULT_BITS, keep, hole, out, work)
                outs.append(out)
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2]) and np.array_equal(outs[0].cpu().numpy(), want)
            assert np.array_equal(lab.cpu().numpy(), _labels(shape, group))       # the input is untouched


@pytest.mark.parametrize("shape", [(7, 7), (TH + 1, TW + 1), (5, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bytes_and_offset_views(device, shape):
    f, (h, w) = 3, shape
    n = f * h * w
    G = 64
    group = S.GROUPS[0]
    labels = _labels(shape, group)
    for lead_in, lead_out in ((1, 3), (3, 1), (2, 2)):
        for keep, hole in ((True, 0), (False, 5), (True, h * w), (False, 0)):
            # labels and out: views at odd byte offsets between 64 guard bytes each
            lbuf = torch.full((G + lead_in + n + G,), 0xA5, dtype=torch.uint8, device=device)
            lbuf[G + lead_in:G + lead_in + n].copy_(torch.from_numpy(labels.reshape(-1).copy()).to(device))
            lv = lbuf[G + lead_in:G + lead_in + n].view(f, h, w)
            obuf = torch.full((G + lead_out + n + G,), 0x5A, dtype=torch.uint8, device=device)
            ov = obuf[G + lead_out:G + lead_out + n].view(f, h, w)
            assert lv.data_ptr() % 4 == lead_in and ov.data_ptr() % 4 == lead_out
            _call(lv, S.DEFAULT_BITS, keep, hole, ov)
            o, l = obuf.cpu().numpy(), lbuf.cpu().numpy()
            what = (shape, lead_in, lead_out, keep, hole)
            assert (o[:G + lead_out] == 0x5A).all() and (o[G + lead_out + n:] == 0x5A).all(), what
            assert np.array_equal(o[G + lead_out:G + lead_out + n].reshape(f, h, w), _want(shape, group, S.DEFAULT_BITS, keep, hole)), what
            assert (l[:G + lead_in] == 0xA5).all() and (l[G + lead_in + n:] == 0xA5).all(), what
            assert np.array_equal(l[G + lead_in:G + lead_in + n], labels.reshape(-1)), what          # the input is untouched


def test_boundaries_give_identical_tensors(device, monkeypatch):
    from face_crop_plus_amd import matte as M
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    shape = (96, 80)
    hw = shape[0] * shape[1]
    for group in (S.GROUPS[0], S.GROUPS[4]):
        ld = torch.from_numpy(_labels(shape, group).copy()).to(device)
        for bits in _bits_of(group):
            for keep, hole in _options(shape):
                res = {}
                for enabled in (True, False):
                    monkeypatch.setattr(T, "ENABLED", enabled)
                    res[enabled] = M.subject_mask(ld, bits, keep, hole)
                assert torch.equal(res[True], res[False])
                assert np.array_equal(res[True].cpu().numpy(), _want(shape, group, bits, keep, hole))
    for enabled in (True, False):
        monkeypatch.setattr(T, "ENABLED", enabled)
        with pytest.raises(RuntimeError, match="max_hole"):
            M.subject_mask(ld, 2, True, -1)
        with pytest.raises(RuntimeError, match="max_hole"):
            M.subject_mask(ld, 2, False, 67108865)
        with pytest.raises(RuntimeError, match="class_bits"):
            M.subject_mask(ld, 1 << 19, True, 0)
        assert tuple(M.subject_mask(ld[:0], 2, True, 4).shape) == (0, 96, 80)
    ops = T.load()
    with pytest.raises(RuntimeError):
        ops.subject_mask(ld.float(), 2, True, 0)
    with pytest.raises(RuntimeError, match="labels"):
        ops.subject_mask(ld[0, 0], 2, True, 0)


# ---- downstream: the matte kernels on the cleaned mask
def test_matte_kernels_on_the_cleaned_mask_equal_the_references(device):
    from face_crop_plus_amd import matte as M
    shape = (96, 80)
    group = S.GROUPS[0]
    labels = _labels(shape, group)
    crops = MR.random_crops(np.random.default_rng(12), 3, *shape)
    cd, ld = torch.from_numpy(crops).to(device), torch.from_numpy(labels.copy()).to(device)
    taps = M.blur_taps(3.0)
    for keep, hole in ((True, 0), (False, 5), (True, 16)):
        clean = _want(shape, group, S.DEFAULT_BITS, keep, hole)
        assert not np.array_equal(clean, S.mask0(labels, S.DEFAULT_BITS))
        out = M.subject_mask(ld, S.DEFAULT_BITS, keep, hole)
        assert np.array_equal(out.cpu().numpy(), clean)
        want, want_a = MR.matte(crops, clean, S.SUBJECT_BITS, 5, FILL)
        got, got_a = M.matte(cd, out, M.SUBJECT_BITS, 5, FILL, with_alpha=True)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_a.cpu().numpy(), want_a)
        bg = RB.background(crops, clean, S.SUBJECT_BITS, taps)[0]
        got, got_a = M.matte_blur(cd, out, M.SUBJECT_BITS, 5, taps, with_alpha=True)
        assert np.array_equal(got_a.cpu().numpy(), want_a) and np.array_equal(got.cpu().numpy(), RB.over(crops, want_a, bg))
        alpha = M.refine_alpha(cd, out, M.SUBJECT_BITS, 4, 64)
        assert np.array_equal(alpha.cpu().numpy(), R.alpha_of(crops, clean, S.SUBJECT_BITS, 4, 64))


def test_cropper_matte_equals_reference(device):
    from face_crop_plus_amd import Cropper
    shape = (96, 80)
    group = S.GROUPS[0]
    labels = _labels(shape, group)
    crops = MR.random_crops(np.random.default_rng(12), 3, *shape)
    lm = (np.zeros((1, 5, 2), np.float32), np.array(["a"]))
    kw = dict(output_size=48, landmarks=lm, det_threshold=None, device="cuda:0", weights={"bisenet": "generated"})
    c = Cropper(background=FILL, subject="largest", fill_holes=16, **kw)
    assert (c.subject, c.fill_holes, c.feather) == ("largest", 16, 5) and c.par_model is not None
    clean = _want(shape, group, S.DEFAULT_BITS, True, 16)
    labels = labels.copy()                                           # a writable array for torch
    out, alpha = c.matte(crops, labels)
    want, want_a = MR.matte(crops, clean, S.SUBJECT_BITS, 5, FILL)
    assert np.array_equal(alpha, want_a) and np.array_equal(out, want)
    plain, plain_a = Cropper(background=FILL, **kw).matte(crops, labels)
    assert not np.array_equal(plain_a, alpha)
    c = Cropper(background_blur=3.0, fill_holes=5, refine=4, foreground=[1, 17], **kw)
    clean = S.subject_mask(labels, S.ONE_17, False, 5)
    out, alpha = c.matte(crops, labels)
    want_a = R.alpha_of(crops, clean, S.SUBJECT_BITS, 4, 64)
    bg = RB.background(crops, clean, S.SUBJECT_BITS, RB.blur_taps(3.0))[0]
    assert np.array_equal(alpha, want_a) and np.array_equal(out, RB.over(crops, want_a, bg))


# ---- end to end: process_dir on given landmarks
SIGMA = 3.0
SIZE = (64, 64)
HOLE = 16


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
    """The recipe of tests/test_matte_refine_gpu.py: three files with a landmark set each, their plain crops, the label
    maps the Cropper's own parser gives them (generated weights: noisy maps of many components), and a foreground class
    set under which the cleaning changes the mask of every crop."""
    import itertools
    from PIL import Image
    d = tmp_path_factory.mktemp("subject_in")
    faces = np.load(os.path.join(os.path.dirname(__file__), "golden", "bisenet.npz"))["faces"]
    assert faces.shape == (3, *SIZE, 3)
    imgs = {f"{n}.png": face for n, face in zip("abc", faces)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name, compress_level=1)
    tgt = A.landmarks_target(SIZE, 0.65)
    landmarks = (np.stack([tgt, tgt, tgt]).astype(np.float32), np.array(sorted(imgs)))
    out = tmp_path_factory.mktemp("subject_plain")
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
            clean = S.subject_mask(labels, bits, True, HOLE)
            if all(m.sum() > 10 and (~m).sum() > 10 for m in hard) and all((a != b).any() for a, b in zip(hard, clean)):
                foreground = list(cand)
                break
        if foreground is not None:
            break
    assert foreground is not None, f"the generated parser gives no class set whose mask the cleaning changes: {classes}"
    return {"dir": d, "landmarks": landmarks, "plain": plain, "crops": crops, "labels": labels, "foreground": foreground}


MODES = {"fill": {"background": FILL}, "blur": {"background_blur": SIGMA}}


def _expected(scene, mode, keep, hole):
    bits = sum(1 << c for c in scene["foreground"])
    clean = S.subject_mask(scene["labels"], bits, keep, hole)
    if mode == "fill":
        return MR.matte(scene["crops"], clean, S.SUBJECT_BITS, 5, FILL)[0]
    alpha = MR.matte(scene["crops"], clean, S.SUBJECT_BITS, 5, FILL)[1]
    return RB.over(scene["crops"], alpha, RB.background(scene["crops"], clean, S.SUBJECT_BITS, RB.blur_taps(SIGMA))[0])


_BEFORE = {}


def _mask_groups(scene):
    return {"fg": scene["foreground"], "all": list(range(19))}


def _before(scene, mode, root):
    """The files of a run of the mode without the options, made once per mode."""
    if mode not in _BEFORE:
        c = _cropper(scene["landmarks"], mask_groups=_mask_groups(scene), foreground=scene["foreground"], **MODES[mode])
        c.process_dir(str(scene["dir"]), str(root / "before"), desc=None)
        _BEFORE[mode] = _tree(root / "before")
    return _BEFORE[mode]


CASES = {"both": ({"subject": "largest", "fill_holes": HOLE}, True, HOLE), "su": ({"subject": "largest"}, True, 0),
         "fh": ({"fill_holes": HOLE}, False, HOLE)}


@pytest.mark.parametrize("mode,tag", [("fill", "both"), ("blur", "both"), ("fill", "su"), ("blur", "fh")])
def test_process_dir_files_and_masks(device, scene, tmp_path, mode, tag):
    """The written crops are labels -> subject_ref -> the matte reference; the mask files are those of a run without."""
    before = _before(scene, mode, tmp_path)
    masks = [n for n in before if "_mask" + os.sep in n]
    assert len(masks) == 6
    names = sorted(scene["plain"])
    kw, keep, hole = CASES[tag]
    want = _expected(scene, mode, keep, hole)
    c = _cropper(scene["landmarks"], mask_groups=_mask_groups(scene), foreground=scene["foreground"], **kw, **MODES[mode])
    c.process_dir(str(scene["dir"]), str(tmp_path / tag), desc=None)
    got = _tree(tmp_path / tag)
    assert sorted(before) == sorted(got)
    for n in masks:
        assert got[n] == before[n], n                                # byte-identical files
    for n in set(before) - set(masks):
        assert np.array_equal(_pixels(got[n]), want[names.index(os.path.basename(n))]), (tag, n)
        if tag == "both":
            assert not np.array_equal(_pixels(got[n]), _pixels(before[n])), n


def test_without_the_options_nothing_new_runs(device, scene, tmp_path, monkeypatch):
    from face_crop_plus_amd import matte as M

    def never(*a, **k):
        raise AssertionError("subject_mask without subject / fill_holes")
    monkeypatch.setattr(M, "subject_mask", never)
    bits = sum(1 << c for c in scene["foreground"])
    want, _ = MR.matte(scene["crops"], scene["labels"], bits, 5, FILL)
    c = _cropper(scene["landmarks"], background=FILL, foreground=scene["foreground"])
    assert c.subject is None and c.fill_holes is None
    c.process_dir(str(scene["dir"]), str(tmp_path / "bg"), desc=None)
    got = _tree(tmp_path / "bg")
    for k, n in enumerate(sorted(got)):
        assert np.array_equal(_pixels(got[n]), want[k]), n
    c = _cropper(scene["landmarks"])
    c.process_dir(str(scene["dir"]), str(tmp_path / "plain"), desc=None)
    assert _tree(tmp_path / "plain") == scene["plain"]
    c = _cropper(scene["landmarks"], background=FILL, foreground=scene["foreground"], fill_holes=HOLE)
    with pytest.raises(AssertionError, match="without subject"):
        c.matte(scene["crops"], scene["labels"])
