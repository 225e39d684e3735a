"""The RetinaFace post-processing references of tests/retina_post_ref.py, checked on the host.

Each float64 reference is checked against a float64 ``torch`` evaluation of the reference's formulas and the float32
oracle (``oracle.retinaface_ref``) against it within the derived bound; then every bound and audit is shown to reject a
planted mistake on the very inputs the GPU audit (tests/test_retina_post_audit_gpu.py) uses."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import retinaface_ref as R


def _load_ref():
    spec = importlib.util.spec_from_file_location("_retina_post_ref", os.path.join(os.path.dirname(__file__),
                                                                                   "retina_post_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _load_ref()
f32 = np.float32
SHAPES = [(100, 75), (257, 191), (640, 640), (33, 1)]


def _torch_decode64(loc, ldm, h, w):
    """The reference's decode_bboxes / decode_landms + scaling, in torch float64 over torch-built priors."""
    pri = []
    for s, ms in zip((8, 16, 32), ((16, 32), (64, 128), (256, 512))):
        fh, fw = -(-h // s), -(-w // s)
        i, j, a = torch.meshgrid(torch.arange(fh, dtype=torch.float64), torch.arange(fw, dtype=torch.float64),
                                 torch.tensor(ms, dtype=torch.float64), indexing="ij")
        pri.append(torch.stack([(j + 0.5) * s / w, (i + 0.5) * s / h, a / w, a / h], -1).reshape(-1, 4))
    pri = torch.cat(pri)
    loc, ldm = torch.from_numpy(loc).double(), torch.from_numpy(ldm).double()
    v = (float(f32(0.1)), float(f32(0.2)))
    b = torch.cat((pri[:, :2] + loc[..., :2] * v[0] * pri[:, 2:], pri[:, 2:] * torch.exp(loc[..., 2:] * v[1])), -1)
    b[..., :2] -= b[..., 2:] / 2
    b[..., 2:] += b[..., :2]
    lm = torch.cat([pri[:, :2] + ldm[..., 2 * k:2 * k + 2] * v[0] * pri[:, 2:] for k in range(5)], -1)
    return pri.numpy(), (b * torch.tensor([w, h, w, h], dtype=torch.float64)).numpy(), \
        (lm * torch.tensor([w, h] * 5, dtype=torch.float64)).numpy()


@pytest.mark.parametrize("h,w", SHAPES)
def test_decode64_matches_torch_float64_and_bounds_hold_for_the_oracle(h, w):
    logits, loc, ldm = P.head_inputs(2, h, w, h * 7 + w)
    pri = P.priors64(h, w)
    tp, tb, tl = _torch_decode64(loc, ldm, h, w)
    assert np.array_equal(pri, tp)
    b64, l64 = P.decode64(loc, ldm, pri, h, w)
    fin = np.isfinite(tb)
    assert np.array_equal(fin, np.isfinite(b64))
    np.testing.assert_allclose(b64[fin], tb[fin], rtol=1e-14, atol=1e-9)
    np.testing.assert_allclose(l64, tl, rtol=1e-14, atol=1e-9)
    s64 = P.score64(logits)
    np.testing.assert_allclose(s64, torch.softmax(torch.from_numpy(logits).double(), -1)[..., 1].numpy(), rtol=1e-14,
                               atol=1e-300)
    # the float32 oracle stays within the derived bounds
    pri32 = R.prior_box(h, w)
    assert np.all(np.abs(pri32 - pri) <= P.U * np.abs(pri))
    ob, ol = R.decode(None, loc, ldm, pri32, h, w)
    bb, lb = P.decode_bound(loc, ldm, pri, h, w)
    assert P.err_ratio(ob, b64, bb) <= 1.0
    assert P.err_ratio(ol, l64, lb) <= 1.0
    os32 = torch.softmax(torch.from_numpy(logits), -1)[..., 1].numpy()
    assert P.err_ratio(os32, s64, P.score_bound(logits)) <= 1.0
    # outputs the bound cannot speak for (expf overflow in float32) are exactly the planted overflow rows
    assert np.array_equal(~P.auditable(b64, bb), ~np.isfinite(ob) | (np.abs(b64) >= 1e37))


def test_scores_exactly_at_the_threshold_have_zero_bound():
    logits, *_ = P.head_inputs(1, 64, 64, 5)
    eq = logits[..., 0] == logits[..., 1]
    assert eq.sum() == 2
    assert np.all(P.score64(logits)[eq] == 0.5) and np.all(P.score_bound(logits)[eq] == 0)
    s32 = torch.softmax(torch.from_numpy(logits), -1)[..., 1].numpy()
    assert np.all(s32[eq] == f32(0.5))


@pytest.mark.parametrize("h,w", SHAPES[:2])
def test_decode_bounds_reject_planted_mistakes(h, w):
    logits, loc, ldm = P.head_inputs(1, h, w, 11)
    pri = P.priors64(h, w)
    b64, l64 = P.decode64(loc, ldm, pri, h, w)
    bb, lb = P.decode_bound(loc, ldm, pri, h, w)
    no_half = P.priors64(h, w, centre=0.0).astype(f32)                     # prior centre without +0.5
    ob, ol = R.decode(None, loc, ldm, no_half, h, w)
    assert P.err_ratio(ob, b64, bb) > 1e3 and P.err_ratio(ol, l64, lb) > 1e3
    ob, ol = R.decode(None, loc, ldm, R.prior_box(h, w), h, w, variance=(0.2, 0.1))    # var0 / var1 swapped
    assert P.err_ratio(ob, b64, bb) > 1e3 and P.err_ratio(ol, l64, lb) > 1e3


def test_threshold_audit_accepts_strict_and_rejects_ge():
    for vis in (0.5, 1 - 2.0 ** -23, 0.6):
        logits, *_ = P.head_inputs(1, 64, 48, 3)
        s32 = torch.softmax(torch.from_numpy(logits), -1)[..., 1].numpy()[0]
        s64, sb = P.score64(logits)[0], P.score_bound(logits)[0]
        good = P.threshold_audit(s32 > f32(vis), s64, sb, vis, s32, s32)
        assert good["bad"].size == 0
        if vis == 0.5:
            bad = P.threshold_audit(s32 >= f32(vis), s64, sb, vis, s32, s32)
            assert bad["bad"].size == 2
    # the 1 - 2^-23 rows land exactly on the threshold in float32 (robust to an ulp of expf either side)
    logits, *_ = P.head_inputs(1, 64, 48, 3)
    s32 = torch.softmax(torch.from_numpy(logits), -1)[..., 1].numpy()[0]
    assert (s32 == f32(1 - 2.0 ** -23)).sum() >= 1


def test_nms_audit_accepts_the_oracle_and_rejects_planted_mistakes():
    b, s = P.iou_edge_boxes()
    keep = R.nms_single(b, s, 0.4)
    assert keep == P.nms_f32(b, s) == [0, 1, 3, 5, 7]           # IoU exactly 0.4 survives; ties by position
    assert P.nms_audit(b, s, keep) == []
    assert P.nms_audit(b, s, P.nms_f32(b, s, le=False))           # '<' instead of '<='
    assert P.nms_audit(b, s, P.nms_f32(b, s, one=0.0))            # area without +1
    assert P.nms_audit(b, s, P.nms_f32(b, s, desc_pos=True))      # ties by descending position
    cb, cs = P.cluster_boxes(20000, 150, 1)
    keep = R.nms_single(cb, cs, 0.4)
    assert 100 < len(keep) < 400
    assert P.nms_f32(cb, cs) == keep and P.nms_audit(cb, cs, keep) == []
    assert P.nms_audit(cb, cs, P.nms_f32(cb, cs, desc_pos=True))
    assert P.nms_audit(cb, cs, keep[:-1]) and P.nms_audit(cb, cs, keep + [int(np.setdiff1d(np.arange(20000), keep)[0])])
    gb, gs = P.grid_boxes(30, 40, 2)
    keep = R.nms_single(gb, gs, 0.4)
    assert len(keep) == 1200 and P.nms_audit(gb, gs, keep) == []


def test_iou_delta_is_zero_for_integer_boxes_and_covers_the_float32_formula():
    b, _ = P.iou_edge_boxes()
    iou, d = P.iou_delta(b[0][None], b)
    assert np.all(d < 1e-15) and iou[1] == 0.4              # only the float64 quotient's own rounding
    rng = np.random.default_rng(4)
    x = rng.uniform(0, 3000, (4000, 2)).astype(f32)
    s = rng.uniform(1, 80, (4000, 2)).astype(f32)
    bb = np.concatenate([x, x + s], -1).astype(f32)
    kb, ob = bb[:2000], bb[2000:] + rng.normal(0, 5, (2000, 4)).astype(f32)
    iou, d = P.iou_delta(kb, ob)
    one = f32(1)
    xx1 = np.maximum(kb[:, 0], ob[:, 0]); yy1 = np.maximum(kb[:, 1], ob[:, 1])
    xx2 = np.minimum(kb[:, 2], ob[:, 2]); yy2 = np.minimum(kb[:, 3], ob[:, 3])
    a = np.maximum(f32(0), xx2 - xx1 + one) * np.maximum(f32(0), yy2 - yy1 + one)
    ka = (kb[:, 2] - kb[:, 0] + one) * (kb[:, 3] - kb[:, 1] + one)
    oa = (ob[:, 2] - ob[:, 0] + one) * (ob[:, 3] - ob[:, 1] + one)
    q = a.astype(np.float64) / (ka + oa - a).astype(np.float64)         # unrounded quotient of the float32 operands
    fin = np.isfinite(d)
    assert fin.mean() > 0.99
    assert np.all(np.abs(q - iou)[fin] <= d[fin])


def test_largest_is_torch_argmax_of_plus_one_areas():
    kb = np.array([[0, 0, 4, 4], [0, 0, 1, 13], [5, 5, 8, 8]], f32)   # 25 vs 28 with +1, 16 vs 13 without
    assert P.largest_ref(kb) == 1 and P.largest_ref(kb, one=0.0) == 0
    _, sidx, sel = R.take_by_strategy(np.zeros((3, 10), f32), kb, [0, 0, 0], "largest")
    assert sel == [P.largest_ref(kb)]
    tie = np.array([[0, 0, 4, 4], [1, 1, 5, 5], [2, 2, 6, 6]], f32)
    assert P.largest_ref(tie) == 0                                    # equal areas: the first maximum
    nan = np.array([[0, 0, 9, 9], [0, 0, np.nan, 3], [0, 0, 50, 50], [np.inf, 0, np.inf, 1]], f32)
    assert P.largest_ref(nan) == 1                                    # NaN is maximal, the first one wins
    _, _, sel = R.take_by_strategy(np.zeros((4, 10), f32), nan, [0] * 4, "largest")
    assert sel == [1]
