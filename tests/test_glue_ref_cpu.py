"""The glue-kernel references of tests/glue_ref.py, checked on the host.

Each float64 reference agrees with ``torch.nn.functional`` in float64; each float32 restatement of a kernel's operation order
lies within its derived bound of the float64 reference on the inputs tests/test_glue_kernels_gpu.py uses; and every bound
rejects a planted mistake on those inputs (a tolerance that accepts one is too loose to catch a subtly wrong kernel)."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _load():
    spec = importlib.util.spec_from_file_location("_glue_ref", os.path.join(os.path.dirname(__file__), "glue_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()


# ------------------------------------------------------------------------------------ float64 references vs torch
@pytest.mark.parametrize("align_corners", [False, True])
@pytest.mark.parametrize("h,w,oh,ow", [(1, 1, 5, 3), (1, 37, 16, 16), (41, 1, 16, 9), (100, 72, 512, 512),
                                       (700, 900, 512, 512), (64, 64, 64, 64), (8, 8, 61, 64)])
def test_bilinear_ref_vs_interpolate(h, w, oh, ow, align_corners):
    faces = R.faces_u8(2, h, w, 100 + h)
    ref = R.preprocess_ref64(faces, oh, ow, (0, 0, 0), (1, 1, 1), align_corners)
    x = torch.from_numpy(faces).permute(0, 3, 1, 2)
    # float64: torch computes its indices in float64 and the reference in float32 (as torch does for float32 tensors).  A
    # source index differs by <= 3u (|src| + 1) (scale, product, offset), and a pixel step is <= 1: <= 6u (max(h, w) + 1)
    t64 = F.interpolate(x.double() / 255, (oh, ow), mode="bilinear", align_corners=align_corners).permute(0, 2, 3, 1).numpy()
    assert np.abs(ref - t64).max() <= R.SLACK * 6 * R.U * (max(h, w) + 1)
    # float32: the same float32 indices and weights; only torch's float32 arithmetic differs (a few roundings of values <= 1)
    t32 = F.interpolate(x.float() / 255, (oh, ow), mode="bilinear", align_corners=align_corners).permute(0, 2, 3, 1).numpy()
    assert np.abs(ref - t32).max() <= 8 * R.U


@pytest.mark.parametrize("inp,out", [(512, 1), (512, 37), (512, 64), (512, 255), (512, 256), (512, 512), (512, 1024),
                                     (512, 257), (300, 29), (300, 600), (300, 300), (7, 1024)])
def test_nearest_idx_vs_interpolate(inp, out):
    x = torch.arange(inp, dtype=torch.float64)[None, None, :, None]
    t = F.interpolate(x, (out, 1), mode="nearest")[0, 0, :, 0].long().numpy()
    assert np.array_equal(R.nearest_idx(inp, out), t)
    # the parse kernel's single formula gives ATen's integers, out == in and out == 2 * in included
    assert np.array_equal(R.nearest_idx_kernel(inp, out), t)


def test_preprocess_ref_applies_mean_std():
    faces = R.faces_u8(1, 100, 72, 1)
    ref = R.preprocess_ref64(faces, 512, 512)
    x = F.interpolate(torch.from_numpy(faces).permute(0, 3, 1, 2).double() / 255, (512, 512), mode="bilinear",
                      align_corners=False)
    m = torch.tensor(R.BISE_MEAN, dtype=torch.float32).double().view(1, 3, 1, 1)
    s = torch.tensor(R.BISE_STD, dtype=torch.float32).double().view(1, 3, 1, 1)
    t = ((x - m) / s).permute(0, 2, 3, 1).numpy()
    assert np.abs(ref - t).max() <= R.SLACK * 6 * R.U * 101 / min(R.BISE_STD)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (17, 17), (20, 24)])
def test_bicubic_ref_vs_interpolate(h, w):
    x4 = R.bicubic_input(h, w, 4, 7)
    ref = R.bicubic_ref64(x4, h, w)
    t = F.interpolate(torch.from_numpy(x4[..., :3]).permute(2, 0, 1)[None].double(), (h, w), mode="bicubic",
                      align_corners=False)[0].permute(1, 2, 0).numpy()
    assert np.abs(ref - t).max() <= 1e-14
    t25 = F.interpolate(torch.from_numpy(x4[..., :3]).permute(2, 0, 1)[None].double(), None, 0.25, mode="bicubic")
    assert np.abs(ref - t25[0].permute(1, 2, 0).numpy()).max() <= 1e-14


@pytest.mark.parametrize("hw,c,ld", [(1, 4, 4), (3, 19, 32), (125, 65, 68), (256, 512, 512)])
def test_avgpool_ref_vs_avg_pool2d(hw, c, ld):
    x = R.avgpool_input(2, hw, ld, hw)
    t = F.avg_pool2d(torch.from_numpy(x[:, :, :c]).double().permute(0, 2, 1)[..., None], (hw, 1)).flatten(1).numpy()
    assert np.abs(R.avgpool_ref64(x, c) - t).max() <= 1e-14


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("has_scale,has_shift", [(False, False), (True, False), (False, True), (True, True)])
def test_fc_ref_vs_linear(act, has_scale, has_shift):
    x, w, sc, sh = R.fc_input(3, 65, 19, 5)
    sc, sh = (sc if has_scale else None), (sh if has_shift else None)
    t = torch.from_numpy(x).double() @ torch.from_numpy(w).double().t()
    if sc is not None:
        t = t * torch.from_numpy(sc).double()
    if sh is not None:
        t = t + torch.from_numpy(sh).double()
    t = F.relu(t) if act == 1 else torch.sigmoid(t) if act == 2 else t
    assert np.abs(R.fc_ref64(x, w, sc, sh, act) - t.numpy()).max() <= 1e-14
    lin = F.linear(torch.from_numpy(x).double(), torch.from_numpy(w).double()).numpy()
    assert np.abs(R.fc_ref64(x, w, None, None, 0) - lin).max() <= 1e-14


def test_first_argmax_vs_torch_argmax():
    v = np.array([[1, 3, 3, 2], [np.nan, 1, np.nan, 5], [1, 2, np.nan, 9], [-np.inf] * 4, [0, 0, 0, 0],
                  [np.inf, np.inf, 1, np.nan]], np.float64)
    assert np.array_equal(R.first_argmax(v), torch.argmax(torch.from_numpy(v), -1).numpy())
    g = np.random.default_rng(0)
    v = g.integers(0, 3, (4096, 19)).astype(np.float32)          # many exact ties
    v[g.random(v.shape) < 0.01] = np.nan
    assert np.array_equal(R.first_argmax(v), torch.argmax(torch.from_numpy(v), -1).numpy())


def test_label_mask_and_counts_vs_torch():
    lab = np.arange(32, dtype=np.uint8).repeat(3)
    for bits in (0, 1, 1 << 31, 0xFFFFFFFF, 0x9E3779B9, (1 << 17) | (1 << 14)):
        exp = np.array([255 if (bits >> int(l)) & 1 else 0 for l in lab], np.uint8)
        assert np.array_equal(R.label_mask(lab, bits), exp)
    assert np.array_equal(R.label_counts(lab.reshape(2, 48), 32)[0], torch.bincount(torch.from_numpy(lab[:48]).long(),
                                                                                     minlength=32).numpy())


# --------------------------------------------------------------------- float32 restatements within their bounds
def _ratio(err, bound):
    return float((np.abs(err) / bound).max())


@pytest.mark.parametrize("h,w", R.PREPROCESS_SIZES)
def test_preprocess_f32_within_bound_and_planted_rejected(h, w):
    faces = R.faces_u8(1, h, w, h * 7 + w)
    ref = R.preprocess_ref64(faces, 512, 512)
    bound = R.preprocess_bound(ref)
    assert _ratio(R.preprocess_f32(faces, 512, 512) - ref, bound) <= 1
    if (h, w) in R.PREPROCESS_RESIZED:
        assert _ratio(R.preprocess_f32(faces, 512, 512, align_corners=True) - ref, bound) > 1


@pytest.mark.parametrize("hw", R.AVGPOOL_HW)
def test_avgpool_f32_within_bound_and_planted_rejected(hw):
    for c in R.AVGPOOL_C:
        for ld in (c, c + 3):
            x = R.avgpool_input(2, hw, ld, hw * 1000 + c)
            ref = R.avgpool_ref64(x, c)
            bound = R.avgpool_bound(x, c, ref)
            assert _ratio(R.avgpool_f32(x, c) - ref, bound) <= 1, (hw, c, ld)
            assert _ratio(R.avgpool_f32(x, c, drop_last=True) - ref, bound) > 1, (hw, c, ld)


@pytest.mark.parametrize("cin", R.FC_CIN)
def test_fc_f32_within_bound_and_planted_rejected(cin):
    for cout in R.FC_COUT:
        for n in R.FC_N:
            x, w, sc, sh = R.fc_input(n, cin, cout, cin * 100 + cout + n)
            for act in (0, 1, 2):
                for s_, t_ in ((None, None), (sc, None), (None, sh), (sc, sh)):
                    ref = R.fc_ref64(x, w, s_, t_, act)
                    bound = R.fc_bound(x, w, s_, t_, act, ref)
                    assert _ratio(R.fc_f32(x, w, s_, t_, act) - ref, bound) <= 1, (cin, cout, n, act)
                    if act != 1 or cout * n >= 19:       # ReLU may zero every output that the skipped k changes
                        assert _ratio(R.fc_f32(x, w, s_, t_, act, skip_last=True) - ref, bound) > 1, (cin, cout, n, act)


def test_scale_add_f32_within_bound():
    g = R.gen(3)
    x, addt = torch.randn(2, 64, 512, generator=g).numpy(), torch.randn(2, 64, 512, generator=g).numpy()
    s, addv = torch.rand(2, 512, generator=g).numpy(), torch.randn(2, 512, generator=g).numpy()
    for av, at in ((None, None), (addv, None), (None, addt), (addv, addt)):
        ref = R.scale_add_ref64(x, s, av, at)
        assert _ratio(R.scale_add_f32(x, s, av, at) - ref, R.scale_add_bound(x, s, av, at)) <= 1


PARSE_CPU = [(1, 64, 64, 19, 19, 512, 512, o) for o in R.PARSE_OUT] + [
    (2, 64, 64, 20, 19, 512, 512, (37, 29)), (1, 64, 64, 32, 32, 512, 512, (255, 257)), (1, 64, 64, 19, 1, 512, 512, (64, 64)),
    (1, 64, 64, 32, 19, 300, 200, (255, 257)), (1, 64, 64, 19, 19, 300, 200, (600, 400))]


@pytest.mark.parametrize("f,lh,lw,ld,ncls,mh,mw,out", PARSE_CPU)
def test_parse_tail_f32_within_bound_and_planted_rejected(f, lh, lw, ld, ncls, mh, mw, out):
    lg = R.pad_logits(R.logits_input(f, lh, lw, ld, ld * 10 + ncls), ncls)
    lab = R.parse_tail_f32(lg, ncls, mh, mw, *out)
    assert not R.parse_label_violations(lab, lg, ncls, mh, mw, *out).any()
    if ncls > 1 and out[0] * out[1] > 1:
        wrong = R.parse_tail_f32(lg, ncls, mh, mw, *out, align_corners=False)
        assert R.parse_label_violations(wrong, lg, ncls, mh, mw, *out).any()


def test_parse_tail_ties_and_nan_references():
    lg = R.pad_logits(R.logits_input(1, 64, 64, 20, 4, ties=(2, 5), nan_at=(0, 10, 20, 7)), 19)
    lab = R.parse_tail_f32(lg, 19, 512, 512, 512, 512)
    assert (lab == 2).mean() > 0.5 and not (lab == 5).any()
    # a NaN logit reaches every output pixel whose bilinear footprint holds it (0 * NaN is NaN): the first NaN class wins
    rows = (np.arange(512) * np.float32(63 / 511)).astype(np.int64)
    hit = np.isin(rows, (9, 10))[:, None] & np.isin((np.arange(512) * np.float32(63 / 511)).astype(np.int64), (19, 20))[None]
    assert (lab[0][hit] == 7).all() and hit.sum() > 0
    assert not R.parse_label_violations(lab, lg, 19, 512, 512, 512, 512).any()
    bad = lab.copy()
    bad[0][hit] = 8
    assert R.parse_label_violations(bad, lg, 19, 512, 512, 512, 512).any()


@pytest.mark.parametrize("h,w", R.BICUBIC_HW)
@pytest.mark.parametrize("ld", R.BICUBIC_LD)
def test_bicubic_f32_within_window_and_planted_rejected(h, w, ld):
    x4 = R.bicubic_input(h, w, ld, h * 31 + w + ld)
    ref = R.bicubic_ref64(x4, h, w)
    win = R.bicubic_window(x4)
    assert not R.bicubic_violations(R.bicubic_f32(x4, h, w), ref, win).any()
    assert R.bicubic_violations(R.bicubic_f32(x4, h, w, shift=1), ref, win).any()
    assert ((ref > 1).any() and (ref < 0).any()) or h * w == 1      # both clamps fire


def test_absmax_planted_rejected():
    g = R.gen(9)
    x = torch.randn(100, 40, generator=g).numpy()
    x[-1, 5] = 7.0
    assert R.absmax_ref(x) == np.float32(7.0) and R.absmax_ref(x[:-1]) < 7.0
    x[-1, 5] = 1.0
    x[20, -1] = -9.0
    assert R.absmax_ref(x) == np.float32(9.0) and R.absmax_ref(x[:, :-1]) < 9.0
    x[3, 3] = np.nan
    assert R.absmax_ref(x) == np.float32(np.inf)
    assert R.absmax_ref(np.zeros((4, 8), np.float32)) == 0 and R.absmax_ref(np.full((4, 8), -0.0, np.float32)) == 0


def test_split32_decode_matches_audit_decoder():
    spec = importlib.util.spec_from_file_location("_conv_audit", os.path.join(os.path.dirname(__file__), "conv_audit.py"))
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    v = torch.randn(5, 64, generator=R.gen(4)) * 100
    raw = A.encode(v)
    assert np.array_equal(R.split32_decode(raw.numpy()), A.decode(raw, 1).float().numpy())


def test_u8_to_nhwc4_restatement():
    img = np.arange(256, dtype=np.uint8).repeat(3).reshape(-1, 3)
    out = R.u8_to_nhwc4_f32(img, (104.0, 117.0, 123.0), 1.0)
    assert np.array_equal(out[:, :3], img.astype(np.float32) - np.array([104, 117, 123], np.float32)) and not out[:, 3].any()
    out = R.u8_to_nhwc4_f32(img, (0, 0, 0), 255.0)
    assert np.array_equal(out[:, :3], (torch.from_numpy(img).float() / 255).numpy())
