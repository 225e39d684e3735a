"""The align, warp and batch-builder kernels at their edges, against tests/align_audit_ref.py.

fcp_estimate_transform(_counted): every row's accept / reject and matrix against the exact rational reference within the
derived float64 bound, and bit for bit against the numpy restatement of the kernel's operation order; sentinel tails
behind ``mat`` and ``ok``.  The eight warp kernels (fixed, float32, cubic, Lanczos-4 x batch, ragged) see one edge list,
byte for byte against the oracles, every output carved out of a sentinel-filled buffer.  The batch builder and the ragged
level builder byte for byte against oracle/batch_ref.py, outputs between guard bytes.  Both boundaries (C ABI through
ctypes, torch.ops.fcp) are used for every export touched.  tests/test_align_audit_cpu.py proves the references."""
import importlib.util
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _load():
    spec = importlib.util.spec_from_file_location("_align_audit_ref", os.path.join(os.path.dirname(__file__),
                                                                                   "align_audit_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
WORST = {}          # kernel -> worst |device - exact| / bound over the file
BITS = {}           # kernel -> every bit comparison with the float64 restatement held
GUARD = 64          # sentinel bytes before and after every output (keeps the output 4-byte aligned)
SENT = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _file_budget():
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    print(f"\nalign audit file: {time.time() - t0:.1f} s, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 2**20:.1f} MiB; worst err/bound vs the exact reference: "
          + ", ".join(f"{k} {v:.4f}" for k, v in sorted(WORST.items()))
          + "; bit-equal to kernel_order_f64: " + ", ".join(f"{k} {'yes' if v else 'NO'}" for k, v in sorted(BITS.items())))


def N():
    from face_crop_plus_amd import _native
    return _native


def T():
    from face_crop_plus_amd import torch_ops
    if not os.path.isfile(torch_ops.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    return torch_ops


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _carve(nbytes, device):
    """(buffer, output view): ``nbytes`` bytes between two guards of a sentinel-filled uint8 buffer."""
    buf = torch.full((nbytes + 2 * GUARD,), SENT, dtype=torch.uint8, device=device)
    out = buf[GUARD:GUARD + nbytes]
    assert out.data_ptr() % 4 == 0
    return buf, out


def _guards_ok(buf, nbytes):
    return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + nbytes:] == SENT).all())


# ------------------------------------------------------------------------------------------------------ transforms
MAT_SENT, OK_SENT, TAIL = 0x7FF8DEADBEEF0001, 0x5A5A5A5A, 16


def _estimate_c(device, src_d, dst_d, f, k, skew, face_count=None, valid_total=None, counted=True):
    """The C export with sentinel tails behind mat and ok -> (mat (f,6) float64, ok (f,) int32) on the host."""
    nat = N()
    mat = torch.full((f * 6 + TAIL,), MAT_SENT, dtype=torch.int64, device=device)
    ok = torch.full((f + TAIL,), OK_SENT, dtype=torch.int32, device=device)
    if counted:
        rc = nat.lib().fcp_estimate_transform_counted(nat.ptr(src_d), nat.ptr(dst_d), f, k, int(skew), nat.ptr(face_count),
                                                      nat.ptr(mat), nat.ptr(ok), nat.ptr(valid_total), nat.stream_ptr())
    else:
        rc = nat.lib().fcp_estimate_transform(nat.ptr(src_d), nat.ptr(dst_d), f, k, int(skew), nat.ptr(mat), nat.ptr(ok),
                                              nat.stream_ptr())
    nat.check(rc, "fcp_estimate_transform")
    assert bool((mat[f * 6:] == MAT_SENT).all()) and bool((ok[f:] == OK_SENT).all()), "sentinel tail overwritten"
    return mat[:f * 6].view(torch.float64).view(f, 6).cpu().numpy(), ok[:f].cpu().numpy()


def _estimate_op(monkeypatch, src_d, dst_d, skew, face_count=None, valid_total=None):
    from face_crop_plus_amd import align
    monkeypatch.setattr(T(), "ENABLED", True)
    mat, ok = align.estimate_transform(src_d, dst_d, skew, face_count, valid_total)
    return mat.cpu().numpy(), ok.cpu().numpy()


def _check_transform(name, skew, mat, ok, live=None):
    """ok and matrices of one launch against the exact reference (rows >= live are padding) and the restatement."""
    src, dst = next((s, d) for n, s, d in R.transform_cases() if n == name)
    exact, accept, bound, _ = R.transform_expected(name, skew)
    if live is not None:
        accept = accept & (np.arange(len(accept)) < live)
    assert np.array_equal(ok, accept.astype(np.int32)), (name, skew, np.flatnonzero(ok != accept))
    assert not mat[~accept].any() and not np.signbit(mat[~accept]).any(), "rejected rows must be all-zero matrices"
    if accept.any():
        r = float((np.abs(mat - exact) / bound)[accept].max())
        key = "estimate_transform"
        WORST[key] = max(WORST.get(key, 0.0), r)
        print(f"{name} allow_skew={int(skew)}: worst err / bound {r:.4f} over {int(accept.sum())} accepted rows")
        assert r <= 1, f"{name}: error {r:.3g}x the float64 bound"
    want, _ = R.kernel_order_f64(src, dst, skew)
    same = np.array_equal(mat[accept].view(np.uint64), want[accept].view(np.uint64))
    BITS["estimate_transform"] = BITS.get("estimate_transform", True) and same
    return same


@pytest.mark.parametrize("skew", [False, True])
@pytest.mark.parametrize("name", [n for n, _, _ in R.transform_cases()])
def test_estimate_transform_against_the_exact_reference(name, skew, device, monkeypatch):
    """Expected: bit equality with ``kernel_order_f64`` (the library is built with -ffp-contract=off; double addition,
    multiplication and division are IEEE operations on the device)."""
    src, dst = next((s, d) for n, s, d in R.transform_cases() if n == name)
    f, k = src.shape[:2]
    src_d, dst_d = _dev(src, device), _dev(dst, device)
    accept = R.transform_expected(name, skew)[1]
    mat, ok = _estimate_c(device, src_d, dst_d, f, k, skew, counted=False)
    same = _check_transform(name, skew, mat, ok)
    total = torch.tensor([7], dtype=torch.int64, device=device)              # preset, no face_count: one atomic per wave
    mat2, ok2 = _estimate_c(device, src_d, dst_d, f, k, skew, None, total)
    assert np.array_equal(mat2.view(np.uint64), mat.view(np.uint64)) and np.array_equal(ok2, ok)
    assert int(total.item()) == 7 + int(accept.sum()) == 7 + int(ok.sum())
    mat3, ok3 = _estimate_op(monkeypatch, src_d, dst_d, skew)
    assert np.array_equal(mat3.view(np.uint64), mat.view(np.uint64)) and np.array_equal(ok3, ok)
    assert same, f"{name}: accepted matrices differ in bits from kernel_order_f64"


@pytest.mark.parametrize("boundary", ["c_abi", "torch_ops"])
@pytest.mark.parametrize("skew", [False, True])
def test_estimate_transform_counted(skew, boundary, device, monkeypatch):
    name = "f65"
    src, dst = next((s, d) for n, s, d in R.transform_cases() if n == name)
    f, k = src.shape[:2]
    src_d, dst_d = _dev(src, device), _dev(dst, device)
    accept = R.transform_expected(name, skew)[1]

    def run(fc, vt):
        if boundary == "c_abi":
            return _estimate_c(device, src_d, dst_d, f, k, skew, fc, vt)
        return _estimate_op(monkeypatch, src_d, dst_d, skew, fc, vt)

    total = torch.tensor([1000], dtype=torch.int64, device=device)           # preset; every launch adds to it
    want = 1000
    for count in (0, 1, f - 1, f, f + 7, -3):
        fc = torch.tensor([count], dtype=torch.int32, device=device)
        live = max(min(count, f), 0)
        mat, ok = run(fc, total)
        _check_transform(name, skew, mat, ok, live)
        want += int(accept[:live].sum())
        assert int(total.item()) == want, (count, int(total.item()), want)
    fc = torch.tensor([f - 1], dtype=torch.int32, device=device)
    mat, ok = run(fc, None)                                                  # face_count without an accumulator
    _check_transform(name, skew, mat, ok, f - 1)
    assert int(total.item()) == want
    mat, ok = run(None, total)                                               # an accumulator without face_count
    _check_transform(name, skew, mat, ok)
    assert int(total.item()) == want + int(accept.sum())


# ----------------------------------------------------------------------------------------------------------- warps
_C_BATCH = {"fixed": "fcp_warp_affine_u8", "float32": "fcp_warp_affine_u8_float", "cubic": "fcp_warp_affine_u8_interp",
            "lanczos4": "fcp_warp_affine_u8_interp"}
_C_RAGGED = {"fixed": "fcp_warp_affine_u8_ragged", "float32": "fcp_warp_affine_u8_float_ragged",
             "cubic": "fcp_warp_affine_u8_interp_ragged", "lanczos4": "fcp_warp_affine_u8_interp_ragged"}


def _warp_c(device, family, source, scene, idx, mats, ok, wh, border):
    """One launch through the C ABI into a carved output -> (f, h, w, 3) uint8 on the host."""
    nat = N()
    f, (ow, oh) = len(idx), wh
    buf, out = _carve(f * oh * ow * 3, device)
    mat_d = _dev(mats, device)
    ok_d = None if ok is None else _dev(ok, device)
    interp = [R.W.INTERP[family]] if family in R.W.INTERP else []
    if source == "batch":
        images, pads = scene["images"], scene["pads"]
        n, h, w, _ = images.shape
        idx_d = _dev(idx, device)
        rc = getattr(nat.lib(), _C_BATCH[family])(nat.ptr(images), n, h, w, nat.ptr(idx_d), nat.ptr(mat_d), nat.ptr(ok_d),
                                                  nat.ptr(pads), f, oh, ow, border, *interp, nat.ptr(out), nat.stream_ptr())
    else:
        from face_crop_plus_amd.align import WARP_SRC_DTYPE
        rec = np.zeros(f, WARP_SRC_DTYPE)
        srcs = scene["srcs"][idx]
        rec["off"], rec["h"], rec["w"] = srcs[:, 0], srcs[:, 1], srcs[:, 2]
        rec_d = _dev(rec.view(np.uint8), device)
        blob = scene["blob"]
        rc = getattr(nat.lib(), _C_RAGGED[family])(nat.ptr(blob), blob.numel(), rec.ctypes.data, nat.ptr(rec_d),
                                                   nat.ptr(mat_d), nat.ptr(ok_d), f, oh, ow, border, *interp, nat.ptr(out),
                                                   nat.stream_ptr())
    nat.check(rc, _C_BATCH[family])
    got = out.view(f, oh, ow, 3).cpu().numpy()
    assert _guards_ok(buf, f * oh * ow * 3), "guard bytes around the crops were overwritten"
    return got


def _warp_op(device, family, source, scene, idx, mats, ok, wh, border):
    """The same launch through torch.ops.fcp (``torch_ops.ENABLED`` set by the caller)."""
    from face_crop_plus_amd import align
    mat_d = _dev(mats, device)
    ok_d = None if ok is None else _dev(ok, device)
    kw = {"interpolation": family} if family in R.W.INTERP else {"family": family}
    if source == "batch":
        return align.warp_affine(scene["images"], _dev(idx, device), mat_d, ok_d, scene["pads"], wh, border, **kw).cpu().numpy()
    return align.warp_affine_ragged(scene["blob"], scene["srcs"][idx], mat_d, ok_d, wh, border, **kw).cpu().numpy()


@pytest.fixture(scope="module")
def warp_scenes(device):
    out = {}
    for name, batch, pads in R.warp_scenes():
        blob, srcs = R.ragged_blob(batch, pads)
        blob_d = _dev(blob, device)
        assert blob_d.numel() == srcs[-1, 0] + srcs[-1, 1] * srcs[-1, 2] * 3 and blob_d.data_ptr() % 4 == 0
        out[name] = {"images": _dev(batch, device), "pads": _dev(pads, device), "blob": blob_d, "srcs": srcs}
    return out


@pytest.mark.parametrize("border", list(R.BORDERS))
@pytest.mark.parametrize("source", ["batch", "ragged"])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_warp_edge_list(family, source, border, device, warp_scenes, monkeypatch):
    """Every launch of the edge list through the C ABI with guard bytes, every fourth one through torch.ops.fcp as well."""
    b = R.BORDERS[border]
    ref = R.warp_reference(family, b)
    monkeypatch.setattr(T(), "ENABLED", True)
    for j, ((name, wh, idx, mats, ok), want) in enumerate(zip(R.warp_launches(family), ref)):
        got = _warp_c(device, family, source, warp_scenes[name], idx, mats, ok, wh, b)
        for q in range(len(idx)):
            assert np.array_equal(got[q], want[q]), (name, wh, int(idx[q]), mats[q].tolist(), None if ok is None else int(ok[q]),
                                                     int(np.abs(got[q].astype(int) - want[q]).max()))
        if j % 4 == 0:
            assert np.array_equal(_warp_op(device, family, source, warp_scenes[name], idx, mats, ok, wh, b), want), (name, wh)


def test_batch_warps_refuse_sources_above_the_short_range(device):
    nat = N()
    imgs = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=device)
    idx = torch.zeros(1, dtype=torch.int32, device=device)
    mat = _dev(np.eye(2, 3).reshape(1, 6), device)
    out = torch.empty((1, 4, 4, 3), dtype=torch.uint8, device=device)
    for h, w in ((32768, 1), (1, 32768)):
        for fn, extra in (("fcp_warp_affine_u8", []), ("fcp_warp_affine_u8_float", []), ("fcp_warp_affine_u8_interp", [2])):
            rc = getattr(nat.lib(), fn)(nat.ptr(imgs), 1, h, w, nat.ptr(idx), nat.ptr(mat), None, None, 1, 4, 4, 0, *extra,
                                        nat.ptr(out), nat.stream_ptr())
            assert rc < 0 and b"32767" in nat.lib().fcp_last_error(), (fn, h, w)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------- batch builder, level builder
@pytest.mark.parametrize("boundary", ["c_abi", "torch_ops"])
def test_level_builder_all_geometries_in_one_launch(boundary, device, monkeypatch):
    from face_crop_plus_amd import align
    blob, levels, dst_bytes, exp = R.level_plan()
    src = _dev(blob, device)
    dst = torch.full((dst_bytes,), SENT, dtype=torch.uint8, device=device)
    assert dst.data_ptr() % 4 == 0
    monkeypatch.setattr(T(), "ENABLED", boundary == "torch_ops")
    align.resize_area_ragged(src, levels, dst)
    got = dst.cpu().numpy()
    guard = np.ones(dst_bytes, bool)
    for k, (off, want) in enumerate(exp):
        guard[off:off + want.size] = False
        assert np.array_equal(got[off:off + want.size].reshape(want.shape), want), (k, R.LEVEL_CASES[k])
    assert (got[guard] == SENT).all(), "guard bytes between the levels were overwritten"
    assert guard.sum() >= 16 * (len(exp) + 1)


@pytest.mark.parametrize("border", ["constant", "replicate", "reflect", "wrap", "reflect_101"])
@pytest.mark.parametrize("scene", [s[0] for s in R.batch_scenes()])
def test_batch_builder_geometries(scene, border, device):
    from face_crop_plus_amd.batch import ITEM_DTYPE
    nat = N()
    _, W_, H_, imgs, geo = next(s for s in R.batch_scenes() if s[0] == scene)
    n = len(imgs)
    items = np.zeros(n, ITEM_DTYPE)
    parts, off = [np.array([3], np.uint8)], 1                    # one odd byte in front: odd image offsets
    for i, (img, (sw, sh, dw, dh, top, left, interp)) in enumerate(zip(imgs, geo)):
        items[i] = (off, sh, sw, dh, dw, top, left, interp, 0)
        parts.append(img.reshape(-1))
        off += img.size
    blob = _dev(np.concatenate(parts), device)
    assert blob.numel() == off and {int(o) % 2 for o in items["src_off"]} == {0, 1}     # the last image ends the blob
    items_d = _dev(items.view(np.uint8), device)
    buf, out = _carve(n * H_ * W_ * 3, device)
    nat.check(nat.lib().fcp_build_batch_u8(nat.ptr(blob), blob.numel(), items.ctypes.data, nat.ptr(items_d), n, H_, W_,
                                           R.BORDERS[border], nat.ptr(out), nat.stream_ptr()), "fcp_build_batch_u8")
    got = out.view(n, H_, W_, 3).cpu().numpy()
    assert _guards_ok(buf, n * H_ * W_ * 3), "guard bytes around the batch were overwritten"
    want = R.batch_expected(W_, H_, imgs, geo, border)
    for i in range(n):
        assert np.array_equal(got[i], want[i]), (i, geo[i], int(np.abs(got[i].astype(int) - want[i]).max()))
