"""The device encoders at full size and at their edges (tests/encoder_audit_cases.py; tests/test_encoder_audit_cpu.py
asserts from the references alone that every case exercises what it is here for).

PNG: ``pngenc.encode_streams`` between guard bytes, through both boundaries, against ``png_ref.encode_stream`` byte for
byte; and the device's own stream inflated by zlib (an inflater this project did not write, which also verifies the
Adler-32) against ``png_ref.filter_rows``.  JPEG: ``jpegenc.encode_scans`` between guard bytes against the restatement
(jpeg_options_ref), Pillow where it is built on libjpeg-turbo, and the recorded fixture tests/golden/encoder_audit.npz;
every face stays inside a slot of h * w * c bytes, i.e. on the device."""
import importlib.util
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def _load():
    spec = importlib.util.spec_from_file_location("_encoder_audit_cases", os.path.join(os.path.dirname(__file__), "encoder_audit_cases.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


C = _load()
P, O = C.P, C.O


def _turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


# ---------------------------------------------------------------------------------------------------------- PNG
@pytest.fixture(scope="module")
def png_reference():
    """name -> (image, reference stream) of every case, computed once."""
    return {name: (img, P.encode_stream(img)) for name, img in C.png_small_cases() + [C.png_big_case()]}


def _png_encode(device, img, capacity, boundary):
    """One face between guard bytes -> (length, slot (capacity,) host, the whole guarded buffer (host))."""
    from face_crop_plus_amd import pngenc
    from face_crop_plus_amd import torch_ops as T
    px = img[..., 0] if img.shape[-1] == 1 else img
    buf = torch.full((1, capacity + 2 * GUARD), 0xA5, dtype=torch.uint8, device=device)
    old = T.ENABLED
    T.ENABLED = boundary == "op"
    try:
        lengths = pngenc.encode_streams(torch.from_numpy(np.ascontiguousarray(px[None])).to(device), buf[:, GUARD:GUARD + capacity])
    finally:
        T.ENABLED = old
    assert lengths.dtype == torch.int32 and tuple(lengths.shape) == (1,)
    host = buf.cpu().numpy()[0]
    return int(lengths.cpu()[0]), host[GUARD:GUARD + capacity], host


def _png_check(device, name, img, want):
    capacity = len(want) + 5                                   # the stream fits, with room that has to stay untouched
    for boundary in ("op", "cabi"):
        length, slot, whole = _png_encode(device, img, capacity, boundary)
        assert length == len(want), (name, boundary, length, len(want))
        assert slot[:length].tobytes() == want, (name, boundary)
        assert (slot[length:] == 0xA5).all(), (name, boundary, "bytes written past the stream")
        assert (whole[:GUARD] == 0xA5).all() and (whole[GUARD + capacity:] == 0xA5).all(), (name, boundary, "guard bytes")
        assert zlib.decompress(slot[:length].tobytes()) == P.filter_rows(img).tobytes(), (name, boundary, "zlib")


PNG_GROUPS = {"fullsize": [n for n, _ in C.png_fullsize_cases()], "big": [C.png_big_case()[0]],
              "tall": [n for n, _ in C.png_tall_cases()], "runs": [n for n, _, _ in C.png_run_boundary_cases()],
              "header": [n for n, _, _ in C.png_header_cases()]}


@pytest.mark.parametrize("group", sorted(PNG_GROUPS))
def test_png_bytes_equal_the_definition_and_inflate(device, png_reference, group):
    from face_crop_plus_amd import torch_ops as T
    if not os.path.isfile(T.LIB_PATH):
        pytest.fail("the torch.ops.fcp veneer was not built")
    for name in PNG_GROUPS[group]:
        img, want = png_reference[name]
        print(name, img.shape, "reference", len(want), "bytes")
        _png_check(device, name, img, want)


# ---------------------------------------------------------------------------------------------------------- JPEG
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "encoder_audit.npz"))


@pytest.fixture(scope="module")
def restated():
    """(h, w, channels, subsampling) -> [``encoder_audit_cases.restate`` of each face]: standard and optimised from one
    pass over the coefficients, computed once for the two groups that need it."""
    cache = {}

    def get(h, w, ch, ss):
        if (h, w, ch, ss) not in cache:
            cache[(h, w, ch, ss)] = [C.restate(img, C.QUALITY, ss) for img in C.jpeg_faces(h, w, ch)[1]]
        return cache[(h, w, ch, ss)]
    return get


def _jpeg_encode(device, imgs, capacity, boundary, subsampling, optimize):
    """tests/test_jpeg_options_gpu.py's ``_encode`` at the audit's quality."""
    from face_crop_plus_amd import jpegenc
    from face_crop_plus_amd import torch_ops as T
    f = imgs.shape[0]
    buf = torch.full((f, capacity + 2 * GUARD), 0xA5, dtype=torch.uint8, device=device)
    tbuf = torch.full((f + 2, 4, 272), 0xA5, dtype=torch.uint8, device=device) if optimize else None
    old = T.ENABLED
    T.ENABLED = boundary == "op"
    try:
        lengths = jpegenc.encode_scans(torch.from_numpy(imgs).to(device), buf[:, GUARD:GUARD + capacity], C.QUALITY,
                                       subsampling=subsampling, tables=tbuf[1:f + 1] if optimize else None)
    finally:
        T.ENABLED = old
    assert lengths.dtype == torch.int32 and tuple(lengths.shape) == (f,)
    host = buf.cpu().numpy()
    thost = tbuf.cpu().numpy() if optimize else None
    return lengths.cpu().numpy(), host[:, GUARD:GUARD + capacity], host, thost


@pytest.mark.parametrize("group", C.jpeg_groups(), ids=lambda g: g[0])
def test_jpeg_bytes_equal_restatement_pillow_and_fixture(device, golden, restated, group):
    from face_crop_plus_amd import jpegenc
    name, h, w, ch, ss, opt, restate = group
    kinds, imgs = C.jpeg_faces(h, w, ch)
    capacity = -(-h // 8) * -(-w // 8) * 64 * ch               # the default slot h * w * c; the slivers': their whole blocks
    want = restated(h, w, ch, ss) if restate else None
    for boundary in ("op", "cabi"):
        lengths, slots, whole, tables = _jpeg_encode(device, imgs, capacity, boundary, ss, opt)
        print(name, boundary, "lengths", lengths.tolist(), "capacity", capacity)
        assert (lengths <= capacity).all(), (name, boundary, "a face would fall back to the host")
        assert (whole[:, :GUARD] == 0xA5).all() and (whole[:, GUARD + capacity:] == 0xA5).all(), (name, boundary, "guard bytes")
        if opt:
            assert (tables[0] == 0xA5).all() and (tables[-1] == 0xA5).all(), (name, boundary, "guard records")
            assert len({tables[1 + i].tobytes() for i in range(3)}) == 3, (name, "every face has tables of its own")
        for i, kind in enumerate(kinds):
            n = int(lengths[i])
            scan = slots[i, :n].tobytes()
            assert (slots[i, n:] == 0xA5).all(), (name, boundary, kind, "bytes written past the stream")
            if restate:
                assert n == len(want[i][opt][0]) and scan == want[i][opt][0], (name, boundary, kind, "restatement")
                if opt:
                    assert tables[1 + i].tobytes() == want[i][True][1], (name, boundary, kind, "table records")
            data = jpegenc.jpeg_header(h, w, ch, C.QUALITY, subsampling=ss, tables=tables[1 + i] if opt else None) + scan
            assert golden[C.fixture_key(name, kind)].tolist() == [len(data), zlib.crc32(data)], (name, boundary, kind, "fixture")
            if _turbo():
                assert data == O.pillow(imgs[i], C.QUALITY, ss, opt), (name, boundary, kind, "Pillow")


def test_three_differing_faces_in_one_call_equal_three_calls(device):
    """256 x 256 at 4:4:4 with optimised tables, f = 3: each face has its own histogram, tables and offsets, so the batch
    gives every face the bytes and the records it gets alone."""
    kinds, imgs = C.jpeg_faces(256, 256, 3)
    capacity = imgs[0].size
    together = _jpeg_encode(device, imgs, capacity, "cabi", "4:4:4", True)
    assert len(set(together[0].tolist())) == 3
    for i in range(3):
        alone = _jpeg_encode(device, imgs[i:i + 1], capacity, "cabi", "4:4:4", True)
        assert alone[0][0] == together[0][i] and np.array_equal(alone[1][0], together[1][i]), kinds[i]
        assert np.array_equal(alone[3][1], together[3][1 + i]), kinds[i]
