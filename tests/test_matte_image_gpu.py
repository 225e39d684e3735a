"""Cropper(background_image=...) on the GPU: fcp_matte_image_u8, fcp_matte_image_alpha_u8 and fcp_cutout_image_u8 against
tests/matte_image_ref.py through both boundaries, against the shipped colour kernels with a picture of one colour,
Cropper.matte against the references chained, and process_dir end to end.  Every comparison is byte for byte: equality
everywhere, no tolerance.

Every test fails without the feature: the entry points, the ops, the wrappers and the keywords do not exist there."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join(os.path.dirname(__file__), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("matte_image_ref")
P = _load("png_ref")
RF = _load("matte_refine_ref")
S = _load("subject_ref")
MS = _load("mask_shift_ref")
CR, MR = R.CR, R.MR
BITS = MR.DEFAULT_BITS
FILL = (0, 177, 64)
GUARD = 64
PICKS = list(R.PICKS)
IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")
_TAPS = {}


def _taps(sigma):
    from face_crop_plus_amd import matte as M
    if sigma not in _TAPS:
        _TAPS[sigma] = M.blur_taps(sigma)
    return _TAPS[sigma]


def _boundary(enabled):
    """Context: the torch-op boundary (True) or ctypes (False)."""
    from face_crop_plus_amd import torch_ops as T

    class Ctx:
        def __enter__(self):
            self.old, T.ENABLED = T.ENABLED, enabled

        def __exit__(self, *exc):
            T.ENABLED = self.old
    return Ctx()


BOUNDARIES = pytest.mark.parametrize("boundary", [True, False], ids=["op", "cabi"])


@pytest.fixture(scope="module")
def inputs():
    """(h, w) -> (crops (3,h,w,3), labels (3,h,w), bank (2,h,w,3)), random, made once, read-only."""
    out = {}
    for h, w in R.SHAPES:
        rng = np.random.default_rng(1000 * h + w)
        made = (MR.random_crops(rng, R.F, h, w), MR.random_labels(rng, R.F, h, w), R.random_bank(rng, R.K, h, w))
        for a in made:
            a.setflags(write=False)
        out[(h, w)] = made
    return out


@pytest.fixture(scope="module")
def wanted(inputs):
    """(shape, feather) -> (out, alpha) of the reference, computed once and shared."""
    cache = {}

    def get(shape, feather):
        if (shape, feather) not in cache:
            crops, labels, bank = inputs[shape]
            cache[(shape, feather)] = R.matte_image(crops, labels, BITS, feather, bank, PICKS)
        return cache[(shape, feather)]
    return get


def _dev(device, *arrays):
    return [torch.from_numpy(a.copy()).to(device) for a in arrays]


# ---- fcp_matte_image_u8
@BOUNDARIES
@pytest.mark.parametrize("shape", R.SHAPES, **IDS)
def test_matte_image_equals_the_reference(device, inputs, wanted, shape, boundary):
    from face_crop_plus_amd import matte as M
    crops, labels, bank = inputs[shape]
    cd, ld, bd = _dev(device, crops, labels, bank)
    with _boundary(boundary):
        for feather in MR.FEATHERS:
            want, want_a = wanted(shape, feather)
            out, alpha = M.matte_image(cd, ld, BITS, feather, bd, PICKS, with_alpha=True)
            assert out.dtype == alpha.dtype == torch.uint8 and tuple(out.shape) == crops.shape and tuple(alpha.shape) == labels.shape
            got = out.cpu().numpy()
            bad = int((got != want).sum())
            assert bad == 0, ((shape, feather), bad, np.argwhere(got != want)[:4].tolist())
            assert np.array_equal(alpha.cpu().numpy(), want_a) and torch.equal(alpha, M.feather_alpha(ld, BITS, feather))
            # without the alpha; again, the same bytes; every face alone, the same bytes as in the batch
            again, none = M.matte_image(cd, ld, BITS, feather, bd, PICKS)
            assert none is None and torch.equal(again, out)
            for i in (0, 2):
                alone, _ = M.matte_image(cd[i:i + 1].contiguous(), ld[i:i + 1].contiguous(), BITS, feather, bd, PICKS[i:i + 1])
                assert torch.equal(alone[0], out[i]), (shape, feather, i)
        empty, alpha = M.matte_image(cd[:0], ld[:0], BITS, 5, bd, [], with_alpha=True)
        assert tuple(empty.shape) == (0, *shape, 3) and tuple(alpha.shape) == (0, *shape)
    for t, a in ((cd, crops), (ld, labels), (bd, bank)):
        assert np.array_equal(t.cpu().numpy(), a)                          # the inputs are untouched


@pytest.mark.parametrize("shape", [(1, 7), (5, 3), (33, 47), (70, 130)], **IDS)
def test_c_entry_in_place_at_odd_bytes_between_guard_bytes(device, inputs, wanted, shape):
    """The C entry through ctypes, which can alias and offset: out == crops gives the same bytes; crops, labels, the bank,
    out and alpha each start at a byte of their own, and nothing around out and alpha is written."""
    from face_crop_plus_amd import _native as N
    lib = N.lib()
    h, w = shape
    crops, labels, bank = inputs[shape]
    picks = torch.tensor(PICKS, dtype=torch.int32, device=device)

    def shifted(a, off):
        buf = torch.full((a.size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device)
        buf[GUARD + off:GUARD + off + a.size] = torch.from_numpy(a.copy()).to(device).flatten()
        return buf
    for feather in (0, 5):
        want, want_a = wanted(shape, feather)
        cbuf, lbuf, bbuf = shifted(crops, 1), shifted(labels, 3), shifted(bank, 2)
        obuf = torch.full((crops.size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device)
        abuf = torch.full((labels.size + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=device)
        rc = lib.fcp_matte_image_u8(N.ptr(cbuf, GUARD + 1), N.ptr(lbuf, GUARD + 3), R.F, h, w, BITS, feather, N.ptr(bbuf, GUARD + 2), R.K,
                                    N.ptr(picks), N.ptr(obuf, GUARD + 3), N.ptr(abuf, GUARD + 1), N.stream_ptr())
        assert rc == 0, lib.fcp_last_error()
        for buf, off, expect in ((obuf, 3, want), (abuf, 1, want_a)):
            host = buf.cpu().numpy()
            assert np.array_equal(host[GUARD + off:GUARD + off + expect.size].reshape(expect.shape), expect), (shape, feather)
            assert (host[:GUARD + off] == 0xA5).all() and (host[GUARD + off + expect.size:] == 0xA5).all(), "guard bytes"
        # in place: the crops become the composite, nothing around them moves
        rc = lib.fcp_matte_image_u8(N.ptr(cbuf, GUARD + 1), N.ptr(lbuf, GUARD + 3), R.F, h, w, BITS, feather, N.ptr(bbuf, GUARD + 2), R.K,
                                    N.ptr(picks), N.ptr(cbuf, GUARD + 1), None, N.stream_ptr())
        assert rc == 0, lib.fcp_last_error()
        host = cbuf.cpu().numpy()
        assert np.array_equal(host[GUARD + 1:GUARD + 1 + want.size].reshape(want.shape), want), (shape, feather, "in place")
        assert (host[:GUARD + 1] == 0xA5).all() and (host[GUARD + 1 + want.size:] == 0xA5).all()
        assert np.array_equal(bbuf.cpu().numpy()[GUARD + 2:GUARD + 2 + bank.size].reshape(bank.shape), bank)
    # the plane entry in place
    plane = np.random.default_rng(h * w).integers(0, 256, labels.shape, dtype=np.uint8)
    cbuf, pbuf = shifted(crops, 1), shifted(plane, 1)
    rc = lib.fcp_matte_image_alpha_u8(N.ptr(cbuf, GUARD + 1), N.ptr(pbuf, GUARD + 1), R.F, h, w, N.ptr(bbuf, GUARD + 2), R.K, N.ptr(picks),
                                      N.ptr(cbuf, GUARD + 1), N.stream_ptr())
    assert rc == 0, lib.fcp_last_error()
    want = R.composite(crops, plane, bank, PICKS)
    host = cbuf.cpu().numpy()
    assert np.array_equal(host[GUARD + 1:GUARD + 1 + want.size].reshape(want.shape), want)
    assert (host[:GUARD + 1] == 0xA5).all() and (host[GUARD + 1 + want.size:] == 0xA5).all()


# ---- fcp_matte_image_alpha_u8
@BOUNDARIES
@pytest.mark.parametrize("shape", R.SHAPES, **IDS)
def test_alpha_plane_entry_equals_the_reference(device, inputs, shape, boundary):
    """Through the guided filter's plane (refine 1 and 4, made on the device) and through a random plane that holds 0 and
    255: the composite of the reference through the same plane."""
    from face_crop_plus_amd import matte as M
    crops, labels, bank = inputs[shape]
    cd, ld, bd = _dev(device, crops, labels, bank)
    rng = np.random.default_rng(7 * shape[0] + shape[1])
    random = rng.integers(0, 256, labels.shape, dtype=np.uint8)
    random.reshape(-1)[:2] = (0, 255)
    planes = [torch.from_numpy(random).to(device)] + [M.refine_alpha(cd, ld, BITS, r, 64) for r in (1, 4)]
    with _boundary(boundary):
        for ad in planes:
            plane = ad.cpu().numpy()
            out, alpha = M.matte_image(cd, ld, BITS, 5, bd, PICKS, with_alpha=True, alpha=ad)
            assert alpha is ad and np.array_equal(out.cpu().numpy(), R.composite(crops, plane, bank, PICKS)), shape
            assert M.matte_image(cd, ld, BITS, 5, bd, PICKS, alpha=ad)[1] is None
        assert tuple(M.matte_image(cd[:0], ld[:0], BITS, 5, bd, [], alpha=planes[0][:0])[0].shape) == (0, *shape, 3)


# ---- fcp_cutout_image_u8
@BOUNDARIES
@pytest.mark.parametrize("sigma", [0.5, 4], ids=lambda s: f"sigma{s}")
@pytest.mark.parametrize("shape", R.SHAPES, **IDS)
def test_cutout_image_equals_the_reference(device, inputs, shape, sigma, boundary):
    """The feathered mask (from the device), a random plane, a plane without a soft pixel (every workgroup takes the
    early-out branch) and a plane that is soft everywhere."""
    from face_crop_plus_amd import matte as M
    h, w = shape
    crops, labels, bank = inputs[shape]
    cd, bd = _dev(device, crops, bank)
    taps = _taps(sigma)
    rng = np.random.default_rng(3 * h + w)
    hard = (rng.integers(0, 2, labels.shape) * 255).astype(np.uint8)
    planes = {"feather5": M.feather_alpha(torch.from_numpy(CR.disc_labels(R.F, h, w)).to(device), 1 << 1, 5).cpu().numpy(),
              "random": rng.integers(0, 256, labels.shape, dtype=np.uint8), "hard": hard,
              "soft": rng.integers(1, 255, labels.shape, dtype=np.uint8)}
    assert not ((hard > 0) & (hard < 255)).any() and ((planes["soft"] > 0) & (planes["soft"] < 255)).all()
    with _boundary(boundary):
        for kind, plane in planes.items():
            ad = torch.from_numpy(plane).to(device)
            want = R.composite(crops, plane, bank, PICKS, taps)
            out = M.cutout_image(cd, ad, bd, PICKS, taps)
            assert out.dtype == torch.uint8 and tuple(out.shape) == crops.shape
            got = out.cpu().numpy()
            bad = int((got != want).sum())
            assert bad == 0, ((shape, sigma, kind), bad, np.argwhere(got != want)[:4].tolist())
            alone = M.cutout_image(cd[2:3].contiguous(), ad[2:3].contiguous(), bd, PICKS[2:3], taps)
            assert torch.equal(alone[0], out[2]) and torch.equal(M.cutout_image(cd, ad, bd, PICKS, taps), out)
        assert tuple(M.cutout_image(cd[:0], ad[:0], bd, [], taps).shape) == (0, h, w, 3)
    assert np.array_equal(cd.cpu().numpy(), crops) and np.array_equal(bd.cpu().numpy(), bank)


# ---- against the shipped kernels
@BOUNDARIES
@pytest.mark.parametrize("shape", R.SHAPES, **IDS)
def test_a_picture_of_one_colour_is_the_colour_fill(device, inputs, shape, boundary):
    from face_crop_plus_amd import matte as M
    h, w = shape
    crops, labels, _ = inputs[shape]
    cd, ld = _dev(device, crops, labels)
    one = torch.from_numpy(R.constant_bank(FILL, h, w)).to(device)
    with _boundary(boundary):
        for feather in MR.FEATHERS:
            want, want_a = M.matte(cd, ld, BITS, feather, FILL, with_alpha=True)
            out, alpha = M.matte_image(cd, ld, BITS, feather, one, [0] * R.F, with_alpha=True)
            assert torch.equal(out, want) and torch.equal(alpha, want_a), (shape, feather)
        alpha = M.feather_alpha(ld, BITS, 7)
        assert torch.equal(M.matte_image(cd, ld, BITS, 0, one, [0] * R.F, alpha=alpha)[0], M.matte(cd, ld, BITS, 0, FILL, alpha=alpha)[0])
        for sigma in (0.5, 4):
            assert torch.equal(M.cutout_image(cd, alpha, one, [0] * R.F, _taps(sigma)), M.cutout(cd, alpha, FILL, _taps(sigma))), sigma


def test_refusals_carry_their_messages(device):
    import ctypes
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import matte as M
    from face_crop_plus_amd import torch_ops as T
    lib = N.lib()
    crops = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=device)
    alpha = torch.full((1, 8, 8), 128, dtype=torch.uint8, device=device)
    bank = torch.full((2, 8, 8, 3), 9, dtype=torch.uint8, device=device)
    picks = torch.zeros((1,), dtype=torch.int32, device=device)
    out = torch.full((1, 8, 8, 3), 7, dtype=torch.uint8, device=device)
    taps = _taps(4)
    t16 = (ctypes.c_uint16 * len(taps))(*taps)
    need = lib.fcp_cutout_workspace_bytes(1, 8, 8)
    work = torch.empty((need + 16,), dtype=torch.uint8, device=device)

    def call(radius=len(taps) - 1, b=N.ptr(bank), p=N.ptr(picks), ws=N.ptr(work), wsb=need, k=2):
        return lib.fcp_cutout_image_u8(N.ptr(crops), N.ptr(alpha), 1, 8, 8, b, k, p, t16, radius, N.ptr(out), ws, wsb, N.stream_ptr())
    for kw, word in ((dict(radius=0), b"fcp_matte_image_alpha_u8"), (dict(radius=49), b"radius"), (dict(radius=11), b"sum to 4096"),
                     (dict(k=0), b"pictures"), (dict(k=4097), b"pictures"), (dict(b=None), b"null pointer"), (dict(p=None), b"null pointer"),
                     (dict(wsb=need - 1), b"workspace"), (dict(ws=None), b"workspace"), (dict(ws=N.ptr(work, 4)), b"16-byte aligned")):
        assert call(**kw) < 0, kw
        assert word in lib.fcp_last_error() and lib.fcp_last_error().startswith(b"cutout_image:"), (kw, lib.fcp_last_error())
    assert lib.fcp_matte_image_u8(N.ptr(crops), N.ptr(alpha), 1, 8, 8, 2, 5, None, 2, N.ptr(picks), N.ptr(out), None, N.stream_ptr()) < 0
    assert lib.fcp_last_error() == b"matte_image: null pointer"
    assert lib.fcp_matte_image_alpha_u8(N.ptr(crops), N.ptr(alpha), 1, 8, 8, N.ptr(bank), 2, None, N.ptr(out), N.stream_ptr()) < 0
    assert lib.fcp_last_error() == b"matte_image_alpha: null pointer"
    torch.cuda.synchronize()
    assert (out.cpu() == 7).all()                                    # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), R.composite(crops.cpu().numpy(), alpha.cpu().numpy(), bank.cpu().numpy(), [0], taps))
    ops = T.load()
    for bad_bank in (bank[:, :4], bank[..., :2], bank.float(), bank.cpu(), bank[:, :, ::2]):
        with pytest.raises(RuntimeError, match="pictures"):
            ops.matte_image_alpha(crops, alpha, bad_bank, picks)
    for bad_picks in (picks.long(), torch.zeros((2,), dtype=torch.int32, device=device), picks.cpu()):
        with pytest.raises(RuntimeError, match="picks"):
            ops.matte_image(crops, alpha, 2, 5, bank, bad_picks, False)
    with pytest.raises(RuntimeError, match="radius 3..48"):
        ops.cutout_image(crops, alpha, bank, picks, [])
    with pytest.raises(RuntimeError, match="sum to 4096"):
        ops.cutout_image(crops, alpha, bank, picks, [4000, 1, 1, 1])
    with pytest.raises(RuntimeError, match="feather"):
        ops.matte_image(crops, alpha, 2, 4, bank, picks, False)
    with pytest.raises(RuntimeError, match="class_bits"):
        ops.matte_image(crops, alpha, 1 << 19, 5, bank, picks, False)
    for enabled in (True, False):
        with _boundary(enabled):
            with pytest.raises(ValueError, match="picks"):
                M.matte_image(crops, alpha, 2, 5, bank, [2])
            with pytest.raises(ValueError, match="pictures"):
                M.cutout_image(crops, alpha, bank.cpu(), [0], taps)
            with pytest.raises(RuntimeError, match="radius"):
                M.cutout_image(crops, alpha, bank, [0], [4094, 1])


# ---- Cropper.matte
def test_cropper_matte_equals_the_references_chained(device):
    from face_crop_plus_amd import Cropper
    shape = (33, 47)
    rng = np.random.default_rng(1000 * shape[0] + shape[1])
    labels = S.labels_of(S.GROUPS[0], rng, *shape).copy()
    crops = MR.random_crops(np.random.default_rng(12), 3, *shape)
    bank = R.random_bank(np.random.default_rng(13), 2, *shape)
    lm = (np.zeros((1, 5, 2), np.float32), np.array(["a"]))
    kw = dict(output_size=(shape[1], shape[0]), landmarks=lm, det_threshold=None, device="cuda:0", weights={"bisenet": "generated"},
              background_image=[bank[0], bank[1]])
    feathered = CR.feathered(labels, S.DEFAULT_BITS, 7)
    # explicit picks and the default, i % K
    c = Cropper(feather=7, **kw)
    assert c.par_model is not None and tuple(c._pictures_dev.shape) == (2, *shape, 3) and c._pictures_dev.device.type == "cuda"
    assert np.array_equal(c._pictures_dev.cpu().numpy(), bank)
    for picks, used in (([1, 1, 0], [1, 1, 0]), (None, [0, 1, 0]), (np.array([0, 0, 0]), [0, 0, 0])):
        out, alpha = c.matte(crops, labels, picks)
        assert out.shape == crops.shape and np.array_equal(alpha, feathered)
        assert np.array_equal(out, R.composite(crops, feathered, bank, used)), picks
    with pytest.raises(ValueError, match="picks"):
        c.matte(crops, labels, [0, 1, 2])
    with pytest.raises(ValueError, match="output size"):
        c.matte(crops[:, :, :40], labels[:, :, :40])
    out, alpha = c.matte(crops[:0], labels[:0])
    assert out.shape == (0, *shape, 3) and alpha.shape == (0, *shape)
    # with refine: the guided filter's plane
    want_a = RF.alpha_of(crops, labels, S.DEFAULT_BITS, 4, 64)
    assert ((want_a > 0) & (want_a < 255)).any()
    out, alpha = Cropper(refine=4, **kw).matte(crops, labels, [1, 0, 1])
    assert np.array_equal(alpha, want_a) and np.array_equal(out, R.composite(crops, want_a, bank, [1, 0, 1]))
    # with subject and edge_shift: the cleaned and moved mask under the feather
    moved = MS.shift_mask(S.subject_mask(labels, S.DEFAULT_BITS, True, 0), S.SUBJECT_BITS, -1)
    want_a = CR.feathered(moved, S.SUBJECT_BITS, 5)
    out, alpha = Cropper(subject="largest", edge_shift=-1, **kw).matte(crops, labels)
    assert np.array_equal(alpha, want_a) and np.array_equal(out, R.composite(crops, want_a, bank, [0, 1, 0]))
    # with decontaminate: the subject's colour over the picture, through the feather and through the refined plane
    out, alpha = Cropper(feather=7, decontaminate=2, **kw).matte(crops, labels, [1, 0, 1])
    assert np.array_equal(alpha, feathered) and np.array_equal(out, R.composite(crops, feathered, bank, [1, 0, 1], _taps(2)))
    want_a = RF.alpha_of(crops, labels, S.DEFAULT_BITS, 4, 64)
    out, alpha = Cropper(refine=4, decontaminate=4, **kw).matte(crops, labels)
    assert np.array_equal(alpha, want_a) and np.array_equal(out, R.composite(crops, want_a, bank, [0, 1, 0], _taps(4)))


# ---- end to end: process_dir
def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for n in files:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _decode(file):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(file)))


@pytest.fixture(scope="module")
def photos(tmp_path_factory):
    """Three generated files (one of them a JPEG), a landmark table for them and two pictures of the output size."""
    from PIL import Image
    d = tmp_path_factory.mktemp("matte_image_in")
    rng = np.random.default_rng(31)
    imgs = {"a.png": P.smooth(240, 320), "b.jpg": P.smooth(300, 260)[:, ::-1].copy(),
            "c.png": rng.integers(0, 256, (200, 220, 3), dtype=np.uint8)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name)
    size = (96, 80)
    tgt = A.landmarks_target(size, 0.65)
    rows, names = [], []
    for name, scale, shift in (("a.png", 1.3, (100.0, 60.0)), ("b.jpg", 1.6, (40.0, 90.0)), ("c.png", 1.1, (50.0, 40.0))):
        rows.append(tgt * scale + np.array(shift, np.float32))
        names.append(name)
    bank = np.stack([P.smooth(80, 96)[::-1].copy(), rng.integers(0, 256, (80, 96, 3), dtype=np.uint8)])
    return d, (np.stack(rows).astype(np.float32), np.array(names)), size, bank


def _cropper(photos, batch_size=3, **kw):
    """The generated parser gives these photos the classes 12 and 17 and a few pixels of 6, 9, 14 and 15, never 0: with
    class 17 as the subject a third to two thirds of every crop is background, so the pictures show."""
    from face_crop_plus_amd import Cropper
    d, landmarks, size, bank = photos
    return Cropper(output_size=size, landmarks=landmarks, device="cuda:0", padding="reflect_101", batch_size=batch_size,
                   weights={"bisenet": "generated"}, foreground=[17], **kw)


class _Spy:
    """Cropper._matte_device replaced by a wrapper that records what the matte step saw and returned."""

    def __enter__(self):
        from face_crop_plus_amd import cropper as CR
        self.cls, self.real, self.seen = CR.Cropper, CR.Cropper._matte_device, []
        real, seen = self.real, self.seen

        def spy(self, crops_dev, labels_dev, with_alpha=False, picks=None):
            out, alpha = real(self, crops_dev, labels_dev, with_alpha=True, picks=picks)
            seen.append((crops_dev.cpu().numpy(), alpha.cpu().numpy(), out.cpu().numpy(), None if picks is None else list(picks)))
            return out, (alpha if with_alpha else None)
        self.cls._matte_device = spy
        return self.seen

    def __exit__(self, *exc):
        self.cls._matte_device = self.real


def test_process_dir_composites_over_the_picked_pictures(device, photos, tmp_path):
    """PNG: the written pixels are the reference composite of what the matte step saw, over the pictures that
    ``pick_pictures`` gives the written names; the tree does not depend on the batch size.  With strategy "all" the
    written names, and with them the picks, carry "_<k>"."""
    from face_crop_plus_amd import matte as M
    bank = photos[3]
    for strategy, names in (("largest", ["a.png", "b.png", "c.png"]), ("all", ["a_0.png", "b_0.png", "c_0.png"])):
        with _Spy() as seen:
            c = _cropper(photos, background_image=list(bank), output_format="png", strategy=strategy)
            c.process_dir(str(photos[0]), str(tmp_path / strategy), desc=None)
        tree = _tree(tmp_path / strategy)
        assert sorted(tree) == names
        (crops, alpha, out, picks), = seen                           # one batch of three
        assert picks == M.pick_pictures(names, 2) == M.pick_pictures([str(tmp_path / strategy / n) for n in names], 2)
        assert out.shape == (3, 80, 96, 3) and np.array_equal(out, R.composite(crops, alpha, bank, picks))
        assert ((alpha > 0) & (alpha < 255)).any() and (alpha == 0).any()
        for i, n in enumerate(names):
            assert np.array_equal(_decode(tree[n]), out[i]), n
    # three batches of one write the tree that one batch of three wrote
    c = _cropper(photos, batch_size=1, background_image=list(bank), output_format="png", strategy="all")
    c.process_dir(str(photos[0]), str(tmp_path / "all1"), desc=None)
    assert _tree(tmp_path / "all1") == tree
    assert M.pick_pictures(["a.png", "b.png", "c.png"], 2) == [1, 1, 1] and set(M.pick_pictures(names, 2)) == {0, 1}   # both pictures were used


def test_process_dir_jpeg_through_both_encoders(device, photos, tmp_path):
    """JPEG: the host and the device encoder write the same bytes, of the reference composite, with decontaminate on."""
    bank = photos[3]
    trees = {}
    with _Spy() as seen:
        for enc in ("host", "device"):
            c = _cropper(photos, batch_size=2, background_image=list(bank), output_format="jpg", encoder=enc, decontaminate=4,
                         strategy="all")
            c.process_dir(str(photos[0]), str(tmp_path / enc), desc=None)
            trees[enc] = _tree(tmp_path / enc)
    assert sorted(trees["host"]) == ["a_0.jpg", "b_0.jpg", "c_0.jpg"] and trees["host"] == trees["device"]
    assert all(_decode(v).shape == (80, 96, 3) for v in trees["host"].values())
    assert len(seen) == 4 and sorted(len(s[3]) for s in seen) == [1, 1, 2, 2]
    assert all(((a > 0) & (a < 255)).any() and (a == 0).any() for _, a, _, _ in seen)       # an edge to estimate at, a picture to show
    from face_crop_plus_amd import Cropper
    encode = Cropper(output_size=48, det_threshold=None, device="cuda:0").encode_jpeg
    written = set(trees["host"].values())
    for crops, alpha, out, picks in seen:
        assert np.array_equal(out, R.composite(crops, alpha, bank, picks, _taps(4)))
        assert set(encode(out)) <= written                          # the files are the encodings of exactly those pixels


def test_process_dir_without_pictures_launches_nothing_new(device, photos, tmp_path, monkeypatch):
    from face_crop_plus_amd import matte as M
    calls = []
    for name in ("matte_image", "cutout_image", "pick_pictures"):
        monkeypatch.setattr(M, name, lambda *a, _n=name, **k: calls.append(_n) or (_ for _ in ()).throw(AssertionError(_n)))
    with _Spy() as seen:
        for more in ({}, {"decontaminate": 4}):
            c = _cropper(photos, background=FILL, output_format="png", **more)
            assert c.background_image is None and c._pictures_dev is None
            c.process_dir(str(photos[0]), str(tmp_path / f"fill{len(more)}"), desc=None)
    assert calls == [] and [s[3] for s in seen] == [None, None]       # picks= is not passed without pictures
    crops, alpha, out, _ = seen[0]
    tree = _tree(tmp_path / "fill0")
    assert sorted(tree) == ["a.png", "b.png", "c.png"] and np.array_equal(out, MR.composite(crops, alpha, FILL))
    assert all(np.array_equal(_decode(tree[n]), out[i]) for i, n in enumerate(sorted(tree)))
