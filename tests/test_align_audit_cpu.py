"""The references and bounds of tests/align_audit_ref.py, proven without a GPU on the inputs the GPU audit uses: the
transform bound holds for the kernel's operation order and rejects two planted mistakes; the warp edge list catches a
planted off-by-one in the border index and in the all-constant early-out of every family; the area references stay within
the box filter's bound and catch a wrongly taken integral fast path."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import align_ref as A, batch_ref as B


def _load():
    spec = importlib.util.spec_from_file_location("_align_audit_ref", os.path.join(os.path.dirname(__file__),
                                                                                   "align_audit_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
SKEW = (False, True)


def _worst(mat, name, skew, rows=None):
    exact, accept, bound, _ = R.transform_expected(name, skew)
    sel = accept if rows is None else accept & rows
    return float((np.abs(mat - exact) / bound)[sel].max()) if sel.any() else 0.0


# ------------------------------------------------------------------------------------------------------ transforms
def test_kernel_order_is_within_the_bound_of_the_exact_transform():
    worst, accepted = 0.0, 0
    for name, src, dst in R.transform_cases():
        for skew in SKEW:
            exact, accept, bound, _ = R.transform_expected(name, skew)
            m, ok = R.kernel_order_f64(src, dst, skew)
            assert np.array_equal(ok != 0, accept), (name, skew)
            assert not m[~accept].any()
            r = _worst(m, name, skew)
            assert r <= 1, (name, skew, r)
            worst, accepted = max(worst, r), accepted + int(accept.sum())
    print(f"\nkernel_order_f64 vs exact_transform: worst err / bound {worst:.4f} over {accepted} accepted faces")
    assert accepted > 500


def test_cases_sit_clear_of_the_acceptance_threshold():
    seen = []
    for name, src, dst in R.transform_cases():
        _, accept, _, ratios = R.transform_expected(name, True)
        for i, r in enumerate(ratios):
            if r is not None:
                assert r > R.DET_THRESHOLD * R.RATIO_MARGIN or r < R.DET_THRESHOLD / R.RATIO_MARGIN, (name, i, r)
                seen.append(r)
    special = R.transform_expected("special", True)
    sim = R.transform_expected("special", False)
    # rows: exactly collinear, ratios ~2.9e-6, ~1.8e-10, ~1.1e-14, NaN, +inf, -inf, ordinary
    assert special[1].tolist() == [False, True, True, False, False, False, False, True]
    assert sim[1].tolist() == [True, True, True, True, False, False, False, True]
    r = special[3]
    assert r[0] == 0.0 and 1e-6 < r[1] < 1e-5 and 1e-10 < r[2] < 1e-9 and 1e-15 < r[3] < 1e-13
    # the rejected near-line row: the kernel's order computes the same decision, with the margin the reference module states
    src, dst = next((s, d) for n, s, d in R.transform_cases() if n == "special")
    _, ok = R.kernel_order_f64(src, dst, True)
    assert ok[3] == 0 and ok[2] == 1 and ok[1] == 1
    s = src[3].astype(np.float64)
    x, y = s[:, 0] - s[:, 0].mean(), s[:, 1] - s[:, 1].mean()
    sxx, syy, sxy = (x * x).sum(), (y * y).sum(), (x * y).sum()
    det_err = 2 * R.U * (sxx * syy + sxy * sxy)
    assert abs(sxx * syy - sxy * sxy) + det_err < 0.05 * R.DET_THRESHOLD * sxx * syy
    # k = 2: distinct points are a valid similarity and a singular affine, identical points are rejected by both
    k2s, k2a = R.transform_expected("k2", False)[1], R.transform_expected("k2", True)[1]
    assert k2s.tolist() == [True, True, True, False, True, True, True, True] and not k2a.any()
    assert min(seen) == 0.0 and max(seen) > 0.1


@pytest.mark.parametrize("plant,names", [("float32_sums", None), ("uncentred", ("full_res", "full_res_small"))])
def test_planted_mistakes_exceed_the_bound(plant, names):
    hit = []
    for name, src, dst in R.transform_cases():
        if names is not None and name not in names:
            continue
        for skew in SKEW:
            if plant == "float32_sums":
                m, ok = R.kernel_order_f64(src, dst, skew, centred_dtype=np.float32)
            else:
                m, ok = R.kernel_order_f64(src, dst, skew, centre=False)
            r = _worst(m, name, skew, rows=ok != 0)
            hit.append((name, skew, r))
    print("\n" + plant + ": " + ", ".join(f"{n}/{int(s)} {r:.3g}" for n, s, r in hit))
    if plant == "uncentred":
        assert all(r > 1 for _, _, r in hit), hit           # coordinates around 30000, both forms
    else:
        assert all(r > 1 for n, s, r in hit if not (n == "k2" and s)), hit


def test_oracle_estimate_transform_agrees_within_the_bound():
    worst = 0.0
    for name, src, dst in R.transform_cases():
        for skew in SKEW:
            exact, accept, bound, _ = R.transform_expected(name, skew)
            for i in range(len(src)):
                m = A.estimate_transform(src[i], dst, skew)
                assert (m is not None) == bool(accept[i]), (name, skew, i)
                if m is not None:
                    r = float((np.abs(m.reshape(6) - exact[i]) / bound[i]).max())
                    assert r <= 1, (name, skew, i, r)
                    worst = max(worst, r)
    print(f"\noracle.align_ref.estimate_transform vs exact_transform: worst err / bound {worst:.4f}")


# ----------------------------------------------------------------------------------------------------------- warps
def test_edge_list_has_the_listed_shapes():
    for family in R.FAMILIES:
        L = R.warp_launches(family)
        assert {wh for _, wh, *_ in L} >= set(R.OUT_SIZES)
        assert {len(i) for _, _, i, _, _ in L} >= {1, 9} and max(len(i) for _, _, i, _, _ in L) <= 48
        assert any(ok is None for *_, ok in L) and any(ok is not None and 0 in ok and 1 in ok for *_, ok in L)
        finite = all(np.isfinite(m[ok != 0] if ok is not None else m).all() for _, _, _, m, ok in L)
        assert finite == (family == "float32")
    shapes = {sl.shape[:2] for sl in R.scene_slices(*R.warp_scenes()[0][1:])}
    assert shapes == {(40, 52), (1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (7, 9)}
    ends, offs, rows = set(), set(), set()
    for name, batch, pads in R.warp_scenes():
        blob, srcs = R.ragged_blob(batch, pads)
        assert srcs[-1, 0] + srcs[-1, 1] * srcs[-1, 2] * 3 == blob.size        # the last image ends the blob
        ends.add(blob.size % 4); ends.add(batch.size % 4 + 4)
        offs |= {int(o) % 2 for o in srcs[:, 0]}
        rows |= {int(w) * 3 % 4 for w in srcs[:, 2]} | {batch.shape[2] * 3 % 4 + 4}
    assert ends == set(range(8)) and offs == {0, 1} and rows == set(range(8))


@pytest.mark.parametrize("border", list(R.BORDERS))
@pytest.mark.parametrize("family", R.FAMILIES)
def test_restatement_equals_the_oracles_and_planted_mistakes_change_bytes(family, border):
    """``warp_any`` un-planted is the oracle on every launch (so it is the same function, int32 wrap-around and cvRound of
    non-finite values included); with a planted off-by-one in the border index, or in the all-constant early-out of the
    constant border, at least one byte of the edge list changes."""
    b = R.BORDERS[border]
    scenes = {n: R.scene_slices(bt, p) for n, bt, p in R.warp_scenes()}
    ref = R.warp_reference(family, b)
    for (name, wh, idx, mats, ok), want in zip(R.warp_launches(family), ref):
        got = R.launch_reference(scenes[name], wh, idx, mats, ok, b, family, R.warp_any)
        assert np.array_equal(got, want), (name, wh)
    for plant in ("border",) + (("early_out",) if b == 0 else ()):
        changed = 0
        for (name, wh, idx, mats, ok), want in zip(R.warp_launches(family), ref):
            got = R.launch_reference(scenes[name], wh, idx, mats, ok, b, family,
                                     lambda *a: R.warp_any(*a, plant=plant))
            changed += int((got != want).sum())
            if changed:
                break
        assert changed > 0, (family, border, plant)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_reference_interior_is_close_to_float64_resampling(family):
    """Interior pixels of the ordinary (48, 64) faces against float64 resampling of the float64 inverse map.  Linear: one
    rounding level plus the 1/32-pixel coordinate quantisation times the steepest gradient on each axis (the bound of
    tests/test_align_oracle.py, with both axes); cubic / Lanczos-4: one level from the float64 kernel at the same
    1/32-pixel coordinates (the bound of tests/test_warp_interp_cpu.py)."""
    slices = R.scene_slices(*R.warp_scenes()[0][1:])
    K = R.TAPS[family]
    checked = 0
    for name, wh, idx, mats, ok in R.warp_launches(family):
        if name != "main" or wh != (48, 64) or ok is None:
            continue
        for j in range(len(idx)):
            img = slices[idx[j]]
            if not ok[j] or img.shape[0] < 40 or abs(mats[j, 0] * mats[j, 4] - mats[j, 1] * mats[j, 3]) < 0.01:
                continue
            out = R.oracle_warp(img, mats[j], wh, 1, family).astype(np.float64)
            f = img.astype(np.float64)
            if K == 2:
                want, sx, sy = R.resample_f64(img, mats[j], wh, family)
                inner = (sx >= 0) & (sx <= img.shape[1] - 1) & (sy >= 0) & (sy <= img.shape[0] - 1)
                g = np.abs(np.diff(f, axis=1)).max() + np.abs(np.diff(f, axis=0)).max()
                tol = 1.0 + 2 * g / 32 + 1e-9
            else:
                X, Y = R.W.source_coords(mats[j].reshape(2, 3), wh)
                Mq = np.array([1, 0, 0, 0, 1, 0], np.float64)           # resample at the quantised coordinates
                sx, sy = X / 32.0, Y / 32.0
                want = _resample_at(f, sx, sy, family)
                x0, y0 = (X >> 5) - (K // 2 - 1), (Y >> 5) - (K // 2 - 1)
                inner = (x0 >= 0) & (x0 <= img.shape[1] - K) & (y0 >= 0) & (y0 <= img.shape[0] - K)
                want, tol = np.clip(np.rint(want), 0, 255), 1.0
            if inner.sum() == 0:
                continue
            assert np.abs(out - want)[inner].max() <= tol, (family, j)
            checked += int(inner.sum())
    assert checked > 3000, checked


def _resample_at(f, sx, sy, family):
    K = R.TAPS[family]
    taps = np.arange(K) - (K // 2 - 1)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    wx = R.W.kernel_f64(R.W.INTERP[family], (sx - x0)[..., None] - taps)
    wy = R.W.kernel_f64(R.W.INTERP[family], (sy - y0)[..., None] - taps)
    wx /= wx.sum(-1, keepdims=True); wy /= wy.sum(-1, keepdims=True)
    acc = np.zeros(sx.shape + (3,))
    for r in range(K):
        for k in range(K):
            v = f[np.clip(y0 + taps[r], 0, f.shape[0] - 1), np.clip(x0 + taps[k], 0, f.shape[1] - 1)]
            acc += v * (wy[..., r] * wx[..., k])[..., None]
    return acc


# ------------------------------------------------------------------------------------- batch builder, level builder
def test_level_cases_cover_the_listed_geometries():
    dws = {dw for _, (dw, dh) in R.LEVEL_CASES}
    assert {1, 2, 3, 5} <= dws
    assert {(dw * dh) % 4 for _, (dw, dh) in R.LEVEL_CASES if dw in (1, 2, 3, 5)} == {0, 1, 2, 3}
    blob, levels, dst_bytes, exp = R.level_plan()
    assert levels[-1, 0] + levels[-1, 1] * levels[-1, 2] * 3 == blob.size
    assert (levels[:, 3] % 4 == 0).all() and {int(o) % 2 for o in levels[:, 0]} == {0, 1}
    ends = levels[:, 3] + levels[:, 4] * levels[:, 5] * 3
    assert (levels[1:, 3] - ends[:-1] >= 16).all() and levels[0, 3] >= 16 and dst_bytes - ends[-1] >= 16
    for name, W_, H_, imgs, items in R.batch_scenes():
        assert len(items) >= 9 and max(im.shape[0] for im in imgs) <= 240 and max(im.shape[1] for im in imgs) <= 135
        assert {it[6] for it in items} == ({0, 1} if name.startswith("slot") else {1})
        assert any(it[2] == 1 or it[3] == 1 for it in items)


@pytest.mark.parametrize("case", R.MIXED_AND_CLIPPED)
def test_area_reference_is_within_the_box_filter_bound_and_catches_the_fast_path(case):
    (sw, sh), (dw, dh) = case
    img = R.level_image(R.LEVEL_CASES.index(case))
    exact = R.exact_area(img, dw, dh)
    got = B.resize_area_u8(img, dw, dh)
    err = np.abs(got.astype(np.float64) - exact).max()
    print(f"\n{case}: reference |err| {err:.4f} (bound {R.AREA_BOUND})")
    assert err <= R.AREA_BOUND
    if case != ((100, 37), (33, 17)):                     # one axis integral: the planted fast path must be caught
        planted = R.planted_area_fast_path(img, dw, dh)
        assert np.abs(planted.astype(np.float64) - exact).max() > R.AREA_BOUND
        assert not np.array_equal(planted, got)


def test_batch_expected_places_every_item():
    for name, W_, H_, imgs, items in R.batch_scenes():
        for mode in ("constant", "reflect_101"):
            out = R.batch_expected(W_, H_, imgs, items, mode)
            for i, (sw, sh, dw, dh, top, left, interp) in enumerate(items):
                inner = out[i, top:top + dh, left:left + dw]
                assert np.array_equal(inner, B.resize_u8(imgs[i], dw, dh, "area" if interp else "cubic"))
                if mode == "constant":
                    assert out[i].sum() == inner.sum()
