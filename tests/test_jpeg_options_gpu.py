"""Cropper(jpeg_quality=, jpeg_subsampling=, jpeg_optimize=) on the GPU: lengths, bytes between guard bytes and Huffman table
records of ``fcp_jpeg_encode_ex_u8`` against the restatement tests/jpeg_options_ref.py, the recorded fixture and Pillow at
run time, through both boundaries; per-face tables in batches; libjpeg's limit of the code lengths on the device; slots
that overflow and the host fallback; determinism; refusals; the old entry point's bytes; process_dir end to end, device
against host, file by file.

Every test fails without the feature: the entry points, the ops and the keywords do not exist there."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from oracle import align_ref as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def _load():
    spec = importlib.util.spec_from_file_location("_jpeg_options_ref", os.path.join(os.path.dirname(__file__), "jpeg_options_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


O = _load()
R = O.R
SHAPES = [(h, w, ch, ss) for h, w in O.GPU_SIZES for ch, ss in O.MODES]


def _turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_options.npz"))


@pytest.fixture(scope="module")
def reference():
    """(h, w, channels, subsampling, optimize, quality) -> (kinds, batch, scans, table records or None), computed once."""
    cache = {}

    def get(h, w, ch, ss, opt, q):
        key = (h, w, ch, ss, opt, q)
        if key not in cache:
            imgs = np.stack([R.content(k, h, w, ch) for k in R.CONTENTS])
            scans, records = [], []
            for im in imgs:
                tables = O.tables_of(im, q, ss, opt)
                scans.append(O.encode_scan(im, q, ss, opt, tables))
                records.append(b"".join(O.table_record(t) for t in tables))
            cache[key] = (list(R.CONTENTS), imgs, scans, records if opt else None)
        return cache[key]
    return get


def _encode(device, imgs, capacity, boundary, quality=95, subsampling="4:2:0", optimize=False):
    """One call between guard bytes -> (lengths (F,) host, slots (F, capacity) host, the whole guarded buffer (host), the
    table records (F, 4, 272) host or None, the guarded table buffer)."""
    from face_crop_plus_amd import jpegenc
    from face_crop_plus_amd import torch_ops as T
    f = imgs.shape[0]
    buf = torch.full((f, capacity + 2 * GUARD), 0xA5, dtype=torch.uint8, device=device)
    out = buf[:, GUARD:GUARD + capacity]
    tbuf = torch.full((f + 2, 4, 272), 0xA5, dtype=torch.uint8, device=device) if optimize else None
    old = T.ENABLED
    T.ENABLED = boundary == "op"
    try:
        lengths = jpegenc.encode_scans(torch.from_numpy(imgs).to(device), out, quality, subsampling=subsampling,
                                       tables=tbuf[1:f + 1] if optimize else None)
    finally:
        T.ENABLED = old
    assert lengths.dtype == torch.int32 and tuple(lengths.shape) == (f,) and lengths.device.type == "cuda"
    host = buf.cpu().numpy()
    thost = tbuf.cpu().numpy() if optimize else None
    return lengths.cpu().numpy(), host[:, GUARD:GUARD + capacity], host, (thost[1:f + 1] if optimize else None), thost


def _check(got, want, records, capacity, what):
    lengths, slots, whole, tables, twhole = got
    assert lengths.tolist() == [len(s) for s in want], what
    for i, s in enumerate(want):
        n = min(len(s), capacity)
        assert slots[i, :n].tobytes() == s[:n], (what, i)
        assert (slots[i, n:] == 0xA5).all(), (what, i, "bytes written past the stream")
    assert (whole[:, :GUARD] == 0xA5).all() and (whole[:, GUARD + capacity:] == 0xA5).all(), (what, "guard bytes")
    if records is not None:
        for i, rec in enumerate(records):
            assert tables[i].tobytes() == rec, (what, i, "table records")
        assert (twhole[0] == 0xA5).all() and (twhole[-1] == 0xA5).all(), (what, "guard records")
    else:
        assert tables is None


def _golden_equals(golden, case, data):
    import zlib
    key = O.case_key(case)
    if "jpg_" + key in golden:
        return golden["jpg_" + key].tobytes() == data
    return golden["sum_" + key].tolist() == [len(data), zlib.crc32(data)]


@pytest.mark.parametrize("boundary", ["op", "cabi"])
@pytest.mark.parametrize("optimize", [False, True], ids=["std", "opt"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}_{s[3].replace(':', '')}")
def test_kernel_bytes_equal_restatement_pillow_and_fixture(device, reference, golden, shape, optimize, boundary):
    from face_crop_plus_amd import jpegenc
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    h, w, ch, ss = shape
    for q in (95,) + ((1, 100) if (h, w) in O.EXTRA_QUALITY_SIZES else ()):
        kinds, imgs, want, records = reference(h, w, ch, ss, optimize, q)
        capacity = max(len(s) for s in want) + 5             # every stream fits, with room that has to stay untouched
        got = _encode(device, imgs, capacity, boundary, q, ss, optimize)
        print(shape, optimize, boundary, q, "lengths", got[0].tolist(), "reference", [len(s) for s in want])
        _check(got, want, records, capacity, (shape, optimize, boundary, q))
        for i, kind in enumerate(kinds):
            head = jpegenc.jpeg_header(h, w, ch, q, subsampling=ss, tables=got[3][i] if optimize else None)
            data = head + got[1][i, :got[0][i]].tobytes()
            assert _golden_equals(golden, (kind, h, w, ch, ss, optimize, q), data), (shape, kind, q, "fixture")
            if _turbo():
                assert data == O.pillow(imgs[i], q, ss, optimize), (shape, kind, q, "Pillow")


def test_pillow_comparison_ran():
    """The run-time comparison above is skipped only where Pillow is not built on libjpeg-turbo; say so."""
    if not _turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo: compared with the fixture only")


@pytest.mark.parametrize("f", [1, 3, 65])
def test_batch_sizes_with_optimised_tables(device, f):
    """F faces of differing content in one call: every face has its own tables, offsets and length."""
    h, w = 17, 9
    for ch, ss in ((3, "4:4:4"), (3, "4:2:2"), (1, "4:2:0")):
        imgs = np.stack([R.content(R.CONTENTS[i % 5], h, w, ch, seed=i) for i in range(f)])
        tables = [O.tables_of(im, 95, ss, True) for im in imgs]
        want = [O.encode_scan(im, 95, ss, True, t) for im, t in zip(imgs, tables)]
        records = [b"".join(O.table_record(t) for t in ts) for ts in tables]
        assert f == 1 or len(set(records)) > 1
        capacity = max(len(s) for s in want)                 # the longest fits exactly
        for boundary in ("op", "cabi"):
            _check(_encode(device, imgs, capacity, boundary, 95, ss, True), want, records, capacity, (f, ch, ss, boundary))


# ---- the limit of the code lengths to 16 bits
@pytest.mark.parametrize("shift,nsym", [(0, 19), (1, 18)], ids=["issue", "one_chain"])
def test_length_limit_images_on_the_device(device, golden, shift, nsym):
    """tests/test_jpeg_options_cpu.py::test_length_limit_images says which of the two reaches the limit (the second)."""
    from face_crop_plus_amd import jpegenc
    img, _ = O.fibonacci_image(shift, nsym)
    tables = O.tables_of(img, 50, 2, True)
    want = O.encode_scan(img, 50, 2, True, tables)
    record = b"".join(O.table_record(t) for t in tables)
    capacity = len(want) + 7
    got = _encode(device, img[None], capacity, "cabi", 50, "4:2:0", True)
    _check(got, [want], [record], capacity, (shift, nsym))
    data = jpegenc.jpeg_header(840, 840, 1, 50, tables=got[3][0]) + got[1][0, :got[0][0]].tobytes()
    assert data == golden[f"jpg_fibonacci_{shift}_{nsym}"].tobytes()


@pytest.mark.parametrize("boundary", ["op", "cabi"])
def test_huffman_tables_of_given_rows(device, boundary):
    from face_crop_plus_amd import jpegenc
    from face_crop_plus_amd import torch_ops as T
    one, two = np.zeros(256, np.int64), np.zeros(256, np.int64)
    one[7], two[[3, 200]] = 5, 9
    rng = np.random.default_rng(5)
    sparse = np.where(rng.random(256) < 0.4, rng.integers(1, 30000, 256), 0)
    # the rows that aim at the table builder shared with the PNG encoder: every non-zero count in lane 5 of the wave (index
    # % 64), so that both halves of a merge come from one lane's registers; the two smallest counts equal and in lanes 0 and
    # 63, the two ends of the butterfly (the pseudo-symbol, entry 256 with count 1, ties with them from lane 0).
    # fibonacci_row(30) is the row that reaches depth 30 under the arrays' bound of 32
    one_lane, tie = np.zeros(256, np.int64), np.zeros(256, np.int64)
    one_lane[[5, 69, 133, 197]], tie[[0, 63, 130]] = (3, 1, 4, 1), (1, 1, 7)
    rows = [O.fibonacci_row(19), O.fibonacci_row(25), O.fibonacci_row(30), O.fibonacci_row(19, 1), O.fibonacci_row(25, 1),
            O.fibonacci_row(30, 1), np.ones(256, np.int64), one, two, np.zeros(256, np.int64), sparse,
            np.full(256, 36000, np.int64), one_lane, tie]
    depths = []
    for r in rows:
        info = {}
        O.gen_optimal_table(r, info)
        depths.append(info["depth"])
        assert int(r.sum()) < O.FIB35 - 1
    assert max(depths) == 30 and sum(d > 16 for d in depths) >= 3          # the limiting loop runs, up to 14 levels of it
    want = [O.gen_optimal_table(r) for r in rows]
    freq = torch.from_numpy(np.stack(rows).astype(np.int32)).to(device)
    old = T.ENABLED
    T.ENABLED = boundary == "op"
    try:
        tables, codes = jpegenc.huffman_tables(freq, with_codes=True)
        only = jpegenc.huffman_tables(freq)
    finally:
        T.ENABLED = old
    assert tuple(tables.shape) == (len(rows), 272) and tables.dtype == torch.uint8
    assert tuple(codes.shape) == (len(rows), 256) and codes.dtype == torch.int32
    tables, codes = tables.cpu().numpy(), codes.cpu().numpy().view(np.uint32)
    assert np.array_equal(only.cpu().numpy(), tables)
    for i, t in enumerate(want):
        assert tables[i].tobytes() == O.table_record(t), i
        assert np.array_equal(codes[i], O.code_words(t)), i
    assert not tables[9].any() and not codes[9].any()                       # the all-zero row


# ---- slots that overflow
def test_overflowing_slots_fall_back_to_the_host(device):
    from face_crop_plus_amd import Cropper
    from face_crop_plus_amd import jpegenc
    noise = R.content("noise", 256, 256, 3)
    ramp = R.content("ramp", 256, 256, 3)
    raw = noise.size
    want = O.encode(noise, 100, "4:4:4", False)
    assert raw == 196608 and len(want) == 269731
    c = Cropper(output_size=48, det_threshold=None, device="cuda:0", jpeg_quality=100, jpeg_subsampling="4:4:4")
    files = c.encode_jpeg(np.stack([noise, ramp]))
    assert files[0] == want and files[1] == O.encode(ramp, 100, "4:4:4", False) and len(files[1]) < raw
    if _turbo():
        assert files[0] == O.pillow(noise, 100, "4:4:4", False)
    # with optimised tables and an explicit small slot
    want = O.encode(noise, 100, "4:4:4", True)
    files = jpegenc.encode_jpeg(torch.from_numpy(np.stack([ramp, noise])).to(device), 100, 4096, subsampling="4:4:4", optimize=True)
    assert files == [O.encode(ramp, 100, "4:4:4", True), want]
    assert len(files[0]) > 4096                                              # both fell back
    # at the kernel boundary: the true length, nothing past the slot
    small = R.content("noise", 37, 53, 3)
    for opt in (False, True):
        tables = O.tables_of(small, 100, "4:4:4", opt)
        scan = O.encode_scan(small, 100, "4:4:4", opt, tables)
        record = [b"".join(O.table_record(t) for t in tables)] if opt else None
        assert len(scan) > small.size
        for capacity in (small.size, 1, 0, len(scan) - 1):
            for boundary in ("op", "cabi"):
                _check(_encode(device, small[None], capacity, boundary, 100, "4:4:4", opt), [scan], record, capacity,
                       (opt, capacity, boundary))


def test_two_runs_give_identical_bytes(device, reference):
    for h, w, ch, ss in ((37, 53, 3, "4:4:4"), (37, 53, 3, "4:2:2"), (24, 40, 1, "4:2:0")):
        _, imgs, want, _ = reference(h, w, ch, ss, True, 95)
        capacity = max(len(s) for s in want)
        a = _encode(device, imgs, capacity, "cabi", 95, ss, True)
        b = _encode(device, imgs, capacity, "cabi", 95, ss, True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4])


def test_default_settings_through_the_new_entry_point_equal_the_old_one(device, reference):
    from face_crop_plus_amd import _native as N
    lib = N.lib()
    for h, w, ch in ((37, 53, 3), (17, 9, 3), (24, 40, 1)):
        _, imgs, want, _ = reference(h, w, ch, "4:2:0", False, 95)
        f, capacity = len(imgs), max(len(s) for s in want) + 3
        crops = torch.from_numpy(imgs).to(device)
        need = lib.fcp_jpeg_workspace_bytes(f, h, w, ch)
        assert need == lib.fcp_jpeg_workspace_bytes_ex(f, h, w, ch, 2, 0)
        res = []
        for new in (False, True):
            out = torch.full((f, capacity), 0xA5, dtype=torch.uint8, device=device)
            lengths = torch.full((f,), -1, dtype=torch.int32, device=device)
            work = torch.empty((need,), dtype=torch.uint8, device=device)
            if new:
                rc = lib.fcp_jpeg_encode_ex_u8(N.ptr(crops), f, h, w, ch, 95, 2, 0, N.ptr(out), capacity, capacity, N.ptr(lengths),
                                               None, N.ptr(work), need, N.stream_ptr())
            else:
                rc = lib.fcp_jpeg_encode_u8(N.ptr(crops), f, h, w, ch, 95, 2, N.ptr(out), capacity, capacity, N.ptr(lengths),
                                            N.ptr(work), need, N.stream_ptr())
            assert rc == 0, lib.fcp_last_error()
            torch.cuda.synchronize()
            res.append((lengths.cpu().numpy(), out.cpu().numpy()))
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        assert res[0][0].tolist() == [len(s) for s in want]


def test_refusals_launch_nothing(device):
    from face_crop_plus_amd import _native as N
    from face_crop_plus_amd import torch_ops as T
    crops = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=device)
    out = torch.full((1, 64), 7, dtype=torch.uint8, device=device)
    lengths = torch.full((1,), -5, dtype=torch.int32, device=device)
    tables = torch.full((1, 4, 272), 9, dtype=torch.uint8, device=device)
    lib = N.lib()
    need = lib.fcp_jpeg_workspace_bytes_ex(1, 8, 8, 3, 0, 1)
    work = torch.empty((need,), dtype=torch.uint8, device=device)

    def call(h=8, w=8, c=3, q=95, ss=0, opt=1, cap=64, wsb=need, ws=work, tb=tables, off=0):
        return lib.fcp_jpeg_encode_ex_u8(N.ptr(crops), 1, h, w, c, q, ss, opt, N.ptr(out), 64, cap, N.ptr(lengths), N.ptr(tb),
                                         N.ptr(ws, off), wsb, N.stream_ptr())
    for kw, word in ((dict(h=0), b"bad sizes"), (dict(c=2), b"channels"), (dict(q=0), b"quality"), (dict(ss=3), b"subsampling"),
                     (dict(ss=-1), b"subsampling"), (dict(opt=2), b"optimize"), (dict(tb=None), b"tables"),
                     (dict(cap=65), b"capacity"), (dict(wsb=need - 1), b"workspace"), (dict(w=8193), b"8192"),
                     (dict(off=4), b"aligned"), (dict(h=8192, w=8192, opt=0), b"32-bit bit offsets"),
                     (dict(h=1760, w=1760), b"optimised tables")):
        assert call(**kw) < 0, kw
        assert word in lib.fcp_last_error(), (kw, lib.fcp_last_error())
    torch.cuda.synchronize()
    assert (out.cpu() == 7).all() and lengths.cpu().tolist() == [-5] and (tables.cpu() == 9).all()      # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    img = np.zeros((8, 8, 3), np.uint8)
    ts = O.tables_of(img, 95, 0, True)
    want = O.encode_scan(img, 95, 0, True, ts)
    assert lengths.cpu().tolist() == [len(want)] and out.cpu().numpy()[0, :len(want)].tobytes() == want
    assert tables.cpu().numpy().tobytes() == b"".join(O.table_record(t) for t in ts)
    ops = T.load()
    with pytest.raises(RuntimeError, match="quality"):
        ops.jpeg_encode_ex(crops, 0, 0, out, None)
    with pytest.raises(RuntimeError, match="subsampling"):
        ops.jpeg_encode_ex(crops, 95, 3, out, None)
    with pytest.raises(RuntimeError, match="tables"):
        ops.jpeg_encode_ex(crops, 95, 0, out, tables[:, :2])
    with pytest.raises(RuntimeError):
        ops.jpeg_huffman_tables(torch.zeros((1, 255), dtype=torch.int32, device=device), False)


# ---- end to end: process_dir, device against host
def _noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def _smooth(h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([127.5 + 100 * np.sin(xx / 30.0 + 0.4 * c) * np.cos(yy / 20.0 - 0.3 * c) for c in range(3)],
                    -1).round().astype(np.uint8)


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for n in files:
            p = os.path.join(d, n)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def photos(tmp_path_factory):
    """Three generated files (one of them a JPEG, one with two faces) and a landmark table for them."""
    from PIL import Image
    d = tmp_path_factory.mktemp("jpeg_options_in")
    rng = np.random.default_rng(31)
    imgs = {"a.png": _smooth(240, 320), "b.jpg": _smooth(300, 260)[:, ::-1].copy(), "c.png": _noise(rng, 200, 220)}
    for name, img in imgs.items():
        Image.fromarray(img).save(d / name)
    size = (96, 80)
    tgt = A.landmarks_target(size, 0.65)
    rows, names = [], []
    for name, scale, shift in (("a.png", 1.3, (100.0, 60.0)), ("a.png", 0.9, (30.0, 20.0)), ("b.jpg", 1.6, (40.0, 90.0)),
                               ("c.png", 1.1, (50.0, 40.0))):
        rows.append(tgt * scale + np.array(shift, np.float32))
        names.append(name)
    return d, (np.stack(rows).astype(np.float32), np.array(names)), size


def _run(photos, out, **kw):
    from face_crop_plus_amd import Cropper
    d, landmarks, size = photos
    if kw.get("strategy") != "all":              # one face per file: two would race for the same file name
        first = [list(landmarks[1]).index(n) for n in sorted(set(landmarks[1]))]
        landmarks = (landmarks[0][first], landmarks[1][first])
    c = Cropper(output_size=size, landmarks=landmarks, device="cuda:0", padding="reflect_101", batch_size=2, **kw)
    c.process_dir(str(d), str(out), desc=None)
    return _tree(out)


def _decodes(tree):
    from PIL import Image
    for n, data in tree.items():
        im = Image.open(io.BytesIO(data))
        im.load()
        assert im.size == (96, 80)[::-1] or im.size == (96, 80), n


def test_process_dir_444_optimised_with_mask_groups(device, photos, tmp_path):
    kw = dict(output_format="jpg", strategy="all", mask_groups={"all": list(range(19)), "low": list(range(10))},
              attr_groups=None, weights={"bisenet": "generated"}, jpeg_subsampling="4:4:4", jpeg_quality=90, jpeg_optimize=True)
    host = _run(photos, tmp_path / "host", encoder="host", **kw)
    dev = _run(photos, tmp_path / "dev", encoder="device", **kw)
    assert sorted(host) and sorted(dev) == sorted(host)
    assert any(os.sep + "all_mask" + os.sep in os.sep + n for n in host) and any(n.endswith("a_1.jpg") for n in host)
    for n in host:
        assert dev[n] == host[n], n
    _decodes(dev)
    crops = [n for n in host if "_mask" not in n]
    masks = [n for n in host if "_mask" in n]
    assert crops and masks
    for n in crops:                              # 4:4:4 frames with tables of their own
        at = host[n].index(b"\xff\xc0")
        assert host[n][at + 9] == 3 and host[n][at + 11] == 0x11
    for n in masks:                              # gray: one component whose sampling byte follows the setting
        at = host[n].index(b"\xff\xc0")
        assert host[n][at + 9] == 1 and host[n][at + 11] == 0x11
    plain = _run(photos, tmp_path / "plain", encoder="device", **{k: v for k, v in kw.items() if not k.startswith("jpeg_")})
    assert sorted(plain) == sorted(dev) and all(plain[n] != dev[n] for n in dev)


def test_process_dir_422(device, photos, tmp_path):
    kw = dict(output_format="jpg", jpeg_subsampling="4:2:2")
    host = _run(photos, tmp_path / "host", encoder="host", **kw)
    dev = _run(photos, tmp_path / "dev", encoder="device", **kw)
    assert sorted(host) == ["a.jpg", "b.jpg", "c.jpg"] and sorted(dev) == sorted(host)
    for n in host:
        assert dev[n] == host[n], n
        at = host[n].index(b"\xff\xc0")
        assert host[n][at + 11] == 0x21
    _decodes(dev)
