"""RetinaFace decode / NMS / strategy / gather kernels (fcp_retina_post.hip) against tests/retina_post_ref.py.

Decode outputs are held to the float64 references within the bounds derived from the kernel's op order (the worst
err/bound of every output is printed); the threshold decision to the float64 score and its bound; NMS keep lists are
bit-exact against the float32 oracle (the reference's own semantics) and pass the independent float64 audit; the
"best" / "largest" selections match ``torch.argmax`` on CPU.  Inputs are synthetic head maps (packed like the detector's
fused 32-channel maps) and, where noted, the detector itself with the generated weights.  Every case runs once."""
import importlib.util
import os
import time

import numpy as np
import pytest
import torch

from oracle import retinaface_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32


def _load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(__file__), file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


P = _load("_retina_post_ref", "retina_post_ref.py")
_post = _load("_retina_post_gpu_helpers", "test_retina_post_gpu.py")
_heads_from_raw, _decode = _post._heads_from_raw, _post._decode
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.time()
    yield
    print(f"\nretina post audit: {time.time() - t0:.1f} s, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")
    for k, v in sorted(WORST.items()):
        print(f"  worst err/bound {k}: {v:.3g}")


def _raw_from_heads(heads):
    """The detector's three (n, h, w, 32) head maps -> reference-order (logits, loc, ldm) float32 numpy arrays."""
    lg, lc, lm = [], [], []
    for hd in heads:
        t = (hd.buf if hasattr(hd, "buf") else hd).float().cpu().numpy()
        n = t.shape[0]
        lg.append(t[..., 0:4].reshape(n, -1, 2)); lc.append(t[..., 4:12].reshape(n, -1, 4))
        lm.append(t[..., 12:32].reshape(n, -1, 10))
    return np.concatenate(lg, 1), np.concatenate(lc, 1), np.concatenate(lm, 1)


def _audit_decode(tag, logits, loc, ldm, h, w, vis, out):
    """Dense decode within the float64 bounds, threshold decisions, compaction (ascending prior order, bit-exact copies of
    the dense values).  ``out``: the ``_decode`` tuple.  Returns the per-image candidate positions."""
    cs, cb, cl, cp, cc, ds, db, dl = [t.cpu().numpy() for t in out]
    n = logits.shape[0]
    pri = P.priors64(h, w)
    s64, sb = P.score64(logits), P.score_bound(logits)
    b64, l64 = P.decode64(loc, ldm, pri, h, w)
    bb, lb = P.decode_bound(loc, ldm, pri, h, w)
    r = {"score": P.err_ratio(ds, s64, sb)}
    for k, nm in enumerate(("x1", "y1", "x2", "y2")):
        r[nm] = P.err_ratio(db[..., k], b64[..., k], bb[..., k])
    r["landmarks"] = P.err_ratio(dl, l64, lb)
    for k, v in r.items():
        WORST[f"{tag} {k}"] = max(WORST.get(f"{tag} {k}", 0.0), v)
    assert max(r.values()) <= 1.0, (tag, r)
    # what the bound cannot speak for (float32 expf overflow) equals the oracle bit for bit
    ob, ol = R.decode(None, loc, ldm, R.prior_box(h, w), h, w)
    na = ~P.auditable(b64, bb)
    assert np.array_equal(db[na], ob[na], equal_nan=True)
    o32 = torch.softmax(torch.from_numpy(logits), -1)[..., 1].numpy()
    idxs = []
    for i in range(n):
        k = int(cc[i])
        idx = cp[i, :k]
        cand = np.zeros(s64.shape[1], bool)
        cand[idx] = True
        assert np.all(np.diff(idx) > 0)
        a = P.threshold_audit(cand, s64[i], sb[i], vis, ds[i], o32[i])
        assert a["bad"].size == 0, (tag, i, a["bad"][:10], a)
        assert np.array_equal(cs[i, :k], ds[i, idx])
        assert np.array_equal(cb[i, :k], db[i, idx], equal_nan=True)
        assert np.array_equal(cl[i, :k], dl[i, idx])
        idxs.append(idx)
    return idxs


def _nms_all_strategies(cs, cb, cc, device, thr=0.4):
    """One nms_select launch per strategy on the same device candidates -> numpy dicts."""
    from face_crop_plus_amd.retinaface import nms_select
    outs = {}
    for st in ("all", "best", "largest"):
        o = nms_select(cs, cb, cc, thr, st)
        torch.cuda.synchronize()
        outs[st] = {k: v.cpu().numpy() for k, v in o.items()}
    return outs


def _check_nms(boxes, scores, outs, i, audit=True, thr=0.4):
    """Image i: keep list bit-exact vs the oracle, float64 audit, "all" / "best" / "largest" selections."""
    keep = R.nms_single(boxes, scores, thr)
    kc = int(outs["all"]["keep_count"][i])
    got = outs["all"]["keep_pos"][i, :kc].tolist()
    assert got == keep, (i, kc, len(keep))
    if audit:
        errs = P.nms_audit(boxes, scores, got, thr)
        assert errs == [], errs
    for st in ("best", "largest"):
        assert outs[st]["keep_count"][i] == kc and outs[st]["keep_pos"][i, :kc].tolist() == keep
    assert outs["all"]["sel_count"][i] == kc and outs["all"]["sel_pos"][i, :kc].tolist() == keep
    if kc == 0:
        assert outs["best"]["sel_count"][i] == 0 and outs["largest"]["sel_count"][i] == 0
        return keep
    assert outs["best"]["sel_count"][i] == 1 and outs["best"]["sel_pos"][i, 0] == keep[0]
    assert outs["largest"]["sel_count"][i] == 1
    assert outs["largest"]["sel_pos"][i, 0] == keep[P.largest_ref(boxes[keep])]
    return keep


def _gather(cand_ldm, sel_pos, sel_count, n, cap, pads, max_faces, device):
    from face_crop_plus_amd import _native as N
    off = torch.full((n + 1,), -7, dtype=torch.int32, device=device)
    out_l = torch.full((max_faces, 5, 2), float("nan"), device=device)
    out_i = torch.full((max_faces,), -7, dtype=torch.int32, device=device)
    d_pad = None if pads is None else torch.from_numpy(pads).to(device)
    N.check(N.lib().fcp_retina_gather_faces(N.ptr(cand_ldm), N.ptr(sel_pos), N.ptr(sel_count), n, cap, N.ptr(d_pad),
                                            max_faces, N.ptr(off), N.ptr(out_l), N.ptr(out_i), N.stream_ptr()))
    torch.cuda.synchronize()
    return off.cpu().numpy(), out_l.cpu().numpy(), out_i.cpu().numpy()


def _gather_ref(cand_ldm, sels, pads, max_faces):
    """Image-major selected landmarks minus (left, top) padding, truncated at max_faces, zero tail."""
    n = len(sels)
    exp_l = np.zeros((max_faces, 5, 2), f32)
    exp_i = np.zeros((max_faces,), np.int32)
    f = 0
    for i in range(n):
        for p in sels[i]:
            if f < max_faces:
                v = cand_ldm[i, p].reshape(5, 2)
                exp_l[f] = v - pads[i, [2, 0]].astype(f32) if pads is not None else v
                exp_i[f] = i
            f += 1
    off = np.concatenate([[0], np.cumsum([len(s) for s in sels])]).astype(np.int32)
    return off, exp_l, exp_i


# ------------------------------------------------------------------------------------------------ shipped shapes
@pytest.mark.parametrize("n,size", [(32, 1024), (64, 640), (8, 1024)])
def test_shipped_shapes_detector(n, size, device):
    """The detector with the generated weights at the shipped batch / size: dense decode of its own head maps within the
    float64 bounds, threshold and compaction, NMS + all three strategies, and gather with truncation and paddings."""
    from face_crop_plus_amd import weights
    from face_crop_plus_amd.retinaface import RetinaFace
    g = torch.Generator(device=device).manual_seed(n + size)
    imgs = torch.randint(0, 256, (n, size, size, 3), generator=g, dtype=torch.uint8, device=device)
    det = RetinaFace("all", 0.6).load(device, weights.generate_state_dict("retinaface"))
    res = det.detect(imgs, want_dense=True)
    torch.cuda.synchronize()
    logits, loc, ldm = _raw_from_heads(res["heads"])
    out = (res["cand_score"], res["cand_box"], res["cand_ldm"], res["cand_prior"], res["cand_count"]) + res["dense"]
    idxs = _audit_decode(f"{n}@{size}", logits, loc, ldm, size, size, 0.6, out)
    outs = _nms_all_strategies(res["cand_score"], res["cand_box"], res["cand_count"], device)
    cs, cb = res["cand_score"].cpu().numpy(), res["cand_box"].cpu().numpy()
    sels = []
    for i in range(n):
        k = len(idxs[i])
        sels.append(_check_nms(cb[i, :k], cs[i, :k], outs, i))
    assert sum(map(len, sels)) > n
    # the product's own selection and gather
    kc = res["keep_count"].cpu().numpy()
    assert [res["keep_pos"][i, :kc[i]].cpu().tolist() for i in range(n)] == sels
    cl = res["cand_ldm"].cpu().numpy()
    total = sum(map(len, sels))
    _, el, ei = _gather_ref(cl, sels, None, total)
    assert np.array_equal(res["landmarks"].cpu().numpy(), el) and np.array_equal(res["img_idx"].cpu().numpy(), ei)
    pads = np.random.default_rng(size).integers(0, 300, (n, 4)).astype(np.int32)
    sel_pos = torch.from_numpy(outs["all"]["sel_pos"]).to(device)
    sel_cnt = torch.from_numpy(outs["all"]["sel_count"]).to(device)
    P_ = cs.shape[1]
    for mf in (total - 3, total, total + 5):
        got = _gather(res["cand_ldm"], sel_pos, sel_cnt, n, P_, pads, max(mf, 1), device)
        exp = _gather_ref(cl, sels, pads, max(mf, 1))
        assert all(np.array_equal(a, b) for a, b in zip(got, exp)), mf


# ------------------------------------------------------------------------------------------------------ frame sizes
_R32 = [0, 1, 8, 9, 16, 17, 24, 25]
FRAMES = [(96 + a, 96 + b) for a, b in zip(_R32, _R32[::-1])] + [(1, 1), (8, 8), (7, 300), (985, 1601), (745, 2113)]


def test_frame_sizes_decode(device):
    """Every residue of h and w mod 32 that changes ceil(h / s) for s = 8, 16, 32, 1x1, 8x8, non-square frames, and
    frames whose prior count is 2 below / above the 65 536-prior decode span (985x1601: 65 534, 745x2113: 65 538)."""
    assert P.prior_count(985, 1601) == 65534 and P.prior_count(745, 2113) == 65538
    for k, (h, w) in enumerate(FRAMES):
        n = 2 if P.prior_count(h, w) < 20000 else 1
        logits, loc, ldm = P.head_inputs(n, h, w, 100 + k)
        heads = _heads_from_raw(logits, loc, ldm, h, w, device)
        out = _decode(heads, n, h, w, 0.6, device)
        _audit_decode("frames", logits, loc, ldm, h, w, 0.6, out)


@pytest.mark.parametrize("vis", [0.5, 1 - 2.0 ** -23, 0.0, 1e-30])
def test_threshold_edges(vis, device):
    """Scores exactly at vis in float32 (equal logits give 1/2; l0 - l1 = ln 2^-23 gives 1 - 2^-23): strict '>' drops
    them.  vis 0 and 1e-30: every prior whose score is not 0 is a candidate; with unsaturated logits, every prior."""
    h, w = 200, 136
    logits, loc, ldm = P.head_inputs(2, h, w, 7)
    heads = _heads_from_raw(logits, loc, ldm, h, w, device)
    out = _decode(heads, 2, h, w, vis, device)
    idxs = _audit_decode("threshold", logits, loc, ldm, h, w, vis, out)
    ds = out[5].cpu().numpy()
    for i in range(2):
        assert np.array_equal(idxs[i], np.flatnonzero(ds[i] > f32(vis)))
    if vis == 0.5:
        eq = logits[..., 0] == logits[..., 1]
        assert np.all(ds[eq] == f32(0.5)) and not any(np.isin(idxs[i], np.flatnonzero(eq[i])).any() for i in range(2))
    if vis < 1e-20:
        lg = np.clip(logits, -20, 20)
        heads = _heads_from_raw(lg, loc, ldm, h, w, device)
        out = _decode(heads, 2, h, w, vis, device)
        Pn = P.prior_count(h, w)
        assert out[4].tolist() == [Pn, Pn]
        assert np.array_equal(out[3].cpu().numpy(), np.tile(np.arange(Pn, dtype=np.int32), (2, 1)))


def test_inf_nan_boxes_through_nms_and_largest(device):
    """loc whose expf overflows: inf widths, NaN right edges (inf + -inf), candidates of top score; the decode kernel's
    own candidates through NMS (a NaN box suppresses everything after it) and "largest" (NaN is maximal)."""
    h, w = 160, 224
    logits, loc, ldm = P.head_inputs(3, h, w, 21)
    rng = np.random.default_rng(5)
    for i in range(3):
        r = rng.choice(logits.shape[1], 6, replace=False)
        logits[i, r] = (-9.0, 9.0)
        loc[i, r[:2], 2] = 480.0
        loc[i, r[2:4], 2:] = -700.0
    heads = _heads_from_raw(logits, loc, ldm, h, w, device)
    out = _decode(heads, 3, h, w, 0.6, device)
    idxs = _audit_decode("inf/nan", logits, loc, ldm, h, w, 0.6, out)
    cs, cb, cc = out[0], out[1], out[4]
    outs = _nms_all_strategies(cs, cb, cc, device)
    csn, cbn = cs.cpu().numpy(), cb.cpu().numpy()
    for i in range(3):
        k = len(idxs[i])
        assert not np.isfinite(cbn[i, :k]).all()
        keep = _check_nms(cbn[i, :k], csn[i, :k], outs, i)
        assert len(keep) >= 1


def test_iou_exactly_at_threshold_from_integer_boxes(device):
    b, s = P.iou_edge_boxes()
    cs, cb = torch.from_numpy(s[None]).to(device), torch.from_numpy(b[None]).to(device)
    cc = torch.tensor([len(s)], dtype=torch.int32, device=device)
    outs = _nms_all_strategies(cs, cb, cc, device)
    assert _check_nms(b, s, outs, 0) == [0, 1, 3, 5, 7]


# ------------------------------------------------------------------------------------- sort and capacity edges
def _launch(cases, cap, device):
    """cases: list of (boxes, scores) per image (may be empty) -> padded device candidates + the three launches."""
    n = len(cases)
    cs = np.zeros((n, cap), f32); cb = np.zeros((n, cap, 4), f32); cc = np.zeros((n,), np.int32)
    for i, (b, s) in enumerate(cases):
        cs[i, :len(s)] = s; cb[i, :len(s)] = b; cc[i] = len(s)
        cs[i, len(s):] = 2.0                            # garbage beyond K must never be read
        cb[i, len(s):] = np.nan
    d = [torch.from_numpy(a).to(device) for a in (cs, cb, cc)]
    return _nms_all_strategies(*d, device)


@pytest.mark.parametrize("K", [1, 63, 64, 65, 8191, 8192, 8193, 16384, 65536, 300_007, 507_871, 507_904])
def test_sort_and_capacity_edges(K, device):
    """Sizes at the wave tile (64), the LDS sort (8192 keys), 2 / 8 / 64 LDS chunks per merge stage, and the alive
    bitmap at its 7 936-word LDS limit (507 871: last word partial; 507 904 = 64 * 7 936, the old capacity)."""
    b, s = P.cluster_boxes(K, min(K, 250 if K < 300_000 else 120), K)   # the oracle's greedy loop costs O(kept * K)
    outs = _launch([(b, s)], K, device)
    keep = _check_nms(b, s, outs, 0)
    assert len(keep) >= min(K, 30)


def test_mixed_k_in_one_launch(device):
    """Images of K = 0, 1, 8 193 and 100 000 in one launch: each chooses its own sort path and bitmap size."""
    cases = [(np.zeros((0, 4), f32), np.zeros((0,), f32)), P.cluster_boxes(1, 1, 3), P.cluster_boxes(8193, 200, 4),
             P.cluster_boxes(100_000, 300, 5)]
    outs = _launch(cases, 100_000, device)
    for i, (b, s) in enumerate(cases):
        _check_nms(b, s, outs, i)


def test_thousands_of_survivors(device):
    """4 800 well separated boxes (every one kept: 75 tiles of kept boxes) plus 1 200 duplicates they suppress."""
    gb, gs = P.grid_boxes(60, 80, 6)
    rng = np.random.default_rng(6)
    dup = rng.choice(len(gs), 1200, replace=False)
    b = np.concatenate([gb, gb[dup] + f32(0.5)])
    s = np.concatenate([gs, gs[dup] * f32(0.999)])
    outs = _launch([(b, s)], 6000, device)
    keep = _check_nms(b, s, outs, 0)
    assert len(keep) == 4800


def test_largest_ties_inf_and_nan_across_waves(device):
    """"largest" reduces 1024 strided ranks per thread, 64 lanes per wave, 16 waves: equal maximal areas at ranks 900
    (wave 14) and 1030 (wave 0, second stride) and 2000 -> rank 900; then infinite areas at ranks 1030 (x2 = inf) and
    900 (y2 = inf: the two intersect in a finite box, so both survive) -> rank 900.  A NaN box is suppressed by any box
    kept before it and suppresses every box after it, so a kept NaN area is alone: at rank 0 it is selected."""
    gb, _ = P.grid_boxes(48, 48, 8)
    s = np.linspace(0.99, 0.61, len(gb)).astype(f32)
    assert np.all(np.diff(s) < 0)
    for r in (900, 1030, 2000):
        gb[r, 2:] = gb[r, :2] + f32(34.0)
    outs = _launch([(gb, s)], len(s), device)
    keep = _check_nms(gb, s, outs, 0)
    assert len(keep) == len(s) and outs["largest"]["sel_pos"][0, 0] == 900
    gb[1030, 2] = np.inf
    gb[900, 3] = np.inf
    outs = _launch([(gb, s)], len(s), device)
    keep = _check_nms(gb, s, outs, 0)
    assert len(keep) == len(s) and outs["largest"]["sel_pos"][0, 0] == 900
    gb[0, 2] = np.nan
    outs = _launch([(gb, s)], len(s), device)
    keep = _check_nms(gb, s, outs, 0)
    assert keep == [0] and outs["largest"]["sel_pos"][0, 0] == 0


# ---------------------------------------------------------------------------------------- above the old capacity
def test_nms_above_507904_candidates(device):
    """cap 700 000 with K = 650 000 > 507 904: the alive bitmap no longer fits in LDS (10 157 words)."""
    b, s = P.cluster_boxes(650_000, 120, 9)
    outs = _launch([(b, s)], 700_000, device)
    keep = _check_nms(b, s, outs, 0)
    assert len(keep) >= 100


@pytest.mark.parametrize("size", [4096, 3513])
def test_detect_frames_above_507904_priors(size, device):
    """RetinaFace.detect on one 4096^2 (688 128 priors) and one 3513^2 (508 200) frame against the oracle's decode, NMS and
    gather run on the detector's own head maps (res["heads"]; the conv audit covers those maps)."""
    from face_crop_plus_amd import weights
    from face_crop_plus_amd.retinaface import RetinaFace
    assert P.prior_count(size, size) > 507_904
    g = torch.Generator(device=device).manual_seed(size)
    img = torch.randint(0, 256, (1, size, size, 3), generator=g, dtype=torch.uint8, device=device)
    det = RetinaFace("all", 0.6).load(device, weights.generate_state_dict("retinaface"))
    res = det.detect(img)
    torch.cuda.synchronize()
    logits, loc, ldm = _raw_from_heads(res["heads"])
    pri32 = R.prior_box(size, size)
    o32 = torch.softmax(torch.from_numpy(logits), -1)[..., 1].numpy()[0]
    ob, ol = R.decode(None, loc, ldm, pri32, size, size)
    k = int(res["cand_count"][0])
    idx = res["cand_prior"][0, :k].cpu().numpy()
    cand = np.zeros(len(o32), bool)
    cand[idx] = True
    s64, sb = P.score64(logits)[0], P.score_bound(logits)[0]
    cs = res["cand_score"][0, :k].cpu().numpy()
    k32 = o32.copy()
    k32[idx] = cs                                        # the kernel's float32 scores where it wrote them
    a = P.threshold_audit(cand, s64, sb, 0.6, k32, o32)
    assert a["bad"].size == 0 and k > 100, a
    assert np.all(np.abs(cs.astype(np.float64) - s64[idx]) <= sb[idx])
    cb = res["cand_box"][0, :k].cpu().numpy()
    bb, lb = P.decode_bound(loc[:, idx], ldm[:, idx], P.priors64(size, size)[idx], size, size)
    b64, l64 = P.decode64(loc[:, idx], ldm[:, idx], P.priors64(size, size)[idx], size, size)
    assert P.err_ratio(cb[None], b64, bb) <= 1.0
    keep = R.nms_single(cb, cs, 0.4)
    kc = int(res["keep_count"][0])
    assert res["keep_pos"][0, :kc].cpu().tolist() == keep
    nf = int(res["face_offset"][-1])
    assert nf == len(keep)
    cl = res["cand_ldm"][0, :k].cpu().numpy()
    assert np.array_equal(res["landmarks"][:nf].cpu().numpy(), cl[keep].reshape(-1, 5, 2))
    assert P.err_ratio(cl[None], l64, lb) <= 1.0
    # the oracle's own float32 path agrees wherever its candidates are the kernel's
    oc = np.flatnonzero(o32 > f32(0.6))
    if np.array_equal(oc, idx):
        assert R.nms_single(ob[0, oc], o32[oc], 0.4) == keep
        assert np.allclose(ol[0, oc][keep], cl[keep], rtol=0, atol=1e-2)
