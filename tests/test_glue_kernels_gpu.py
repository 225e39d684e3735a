"""The BiSeNet / RRDB / input glue kernels against tests/glue_ref.py, at the shapes and edges where they can go wrong.

Every launch is checked twice: bit for bit against the float32 restatement of the kernel's documented operation order, and
against the float64 reference of the documented op within the bound derived from that order (tests/test_glue_ref_cpu.py
shows each bound rejects a planted mistake on these same inputs).  Output buffers carry guard regions (padding channels,
bytes past the end) filled with a sentinel that must survive the launch.  Last, two integration checks: RRDBNet.predict on
batches whose images do not start on 4-byte boundaries, and BiSeNet.parse across sub-batches of odd-sized faces."""
import ctypes as C
import importlib.util
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _load():
    spec = importlib.util.spec_from_file_location("_glue_ref", os.path.join(os.path.dirname(__file__), "glue_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load()
WORST = {}          # kernel -> worst |device - ref64| / bound over the file


def _note(kernel, err, bound):
    r = float((np.abs(err) / bound).max())
    WORST[kernel] = max(WORST.get(kernel, 0.0), r)
    assert r <= 1, f"{kernel}: error {r:.3g}x its float64 bound"


@pytest.fixture(scope="module", autouse=True)
def _file_budget():
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    print(f"\nglue kernels file: {time.time() - t0:.1f} s, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 2**30:.2f} GiB; worst err/bound vs float64: "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def N():
    from face_crop_plus_amd import _native
    return _native


def _call(fn, *args):
    """Launch export `fn`: a tensor argument becomes its device pointer, (tensor, byte offset) an offset pointer, None NULL.
    The tensors stay referenced here until the launch is queued (a temporary freed earlier could hand its memory to the
    next argument's upload)."""
    nat = N()
    ptrs = [nat.ptr(*a) if isinstance(a, tuple) else nat.ptr(a) if a is None or isinstance(a, torch.Tensor) else a
            for a in args]
    nat.check(getattr(nat.lib(), fn)(*ptrs, nat.stream_ptr()), fn)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits_equal(got: np.ndarray, exp: np.ndarray) -> bool:
    return got.shape == exp.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32),
                                                     np.ascontiguousarray(exp, np.float32).view(np.uint32))


SENT = 0x7FC0DEAD          # bit pattern of a NaN no kernel produces


def _sent(shape, device) -> torch.Tensor:
    """float32 buffer filled with the SENT pattern (made from int32: a float fill need not keep a NaN's payload)."""
    return torch.full(shape, SENT, dtype=torch.int32, device=device).view(torch.float32)


def _sentinel_ok(t: torch.Tensor) -> bool:
    return bool((t.contiguous().view(torch.int32) == SENT).all())


# ------------------------------------------------------------------------------------------------------ preprocess
def _preprocess(faces, oh, ow, device):
    f, h, w, _ = faces.shape
    out = _sent((f * oh * ow * 4 + 64,), device)
    mean, std = (C.c_float * 3)(*R.BISE_MEAN), (C.c_float * 3)(*R.BISE_STD)
    _call("fcp_bise_preprocess_u8", _dev(faces, device), f, h, w, out, oh, ow, mean, std)
    assert _sentinel_ok(out[f * oh * ow * 4:])
    return out[:f * oh * ow * 4].view(f, oh, ow, 4).cpu().numpy()


@pytest.mark.parametrize("h,w", R.PREPROCESS_SIZES)
def test_preprocess_bits_and_fp64(h, w, device):
    f = 3 if h * w <= 512 * 512 else 1
    faces = R.faces_u8(f, h, w, h * 7 + w)
    got = _preprocess(faces, 512, 512, device)
    assert not got[..., 3].any()
    assert _bits_equal(got[..., :3], R.preprocess_f32(faces, 512, 512)), (h, w)
    ref = R.preprocess_ref64(faces, 512, 512)
    _note("preprocess", got[..., :3] - ref, R.preprocess_bound(ref))


def test_preprocess_32_faces_past_the_grid_cap(device):
    """32 x 512^2 outputs = 32768 blocks of 256 > the 16384-block grid: faces 16..31 come from the second grid-stride pass."""
    faces = R.faces_u8(32, 512, 512, 32)
    got = _preprocess(faces, 512, 512, device)
    assert not got[..., 3].any()
    for i in range(32):
        assert _bits_equal(got[i, ..., :3], R.preprocess_f32(faces[i:i + 1], 512, 512)[0]), i
    for i in (0, 15, 16, 31):
        ref = R.preprocess_ref64(faces[i:i + 1], 512, 512)[0]
        _note("preprocess", got[i, ..., :3] - ref, R.preprocess_bound(ref))


def test_preprocess_odd_output_size(device):
    faces = R.faces_u8(2, 100, 72, 5)
    got = _preprocess(faces, 37, 29, device)
    assert _bits_equal(got[..., :3], R.preprocess_f32(faces, 37, 29))


# --------------------------------------------------------------------------------------------------------- avgpool
def _avgpool(x, c, c0, device):
    n, hw, ld = x.shape
    out = _sent((n * c + 16,), device)
    _call("fcp_avgpool_nhwc_f32", (_dev(x, device), 4 * c0), n, hw, c, ld, out)
    assert _sentinel_ok(out[n * c:])
    return out[:n * c].view(n, c).cpu().numpy()


@pytest.mark.parametrize("hw", R.AVGPOOL_HW)
def test_avgpool_bits_and_fp64(hw, device):
    for c in R.AVGPOOL_C:
        for c0, ld in ((0, c), (3, c + 5)):              # dense, and a channel slice of a wider tensor
            x = R.avgpool_input(2, hw, ld, hw * 1000 + c)
            got = _avgpool(x, c, c0, device)
            xs = x[:, :, c0:]
            assert _bits_equal(got, R.avgpool_f32(xs, c)), (hw, c, ld)
            ref = R.avgpool_ref64(xs, c)
            _note("avgpool", got - ref, R.avgpool_bound(xs, c, ref))


@pytest.mark.parametrize("hw,c", R.AVGPOOL_SHIPPED)
def test_avgpool_shipped_shapes(hw, c, device):
    x = R.avgpool_input(8, hw, c, hw + c)
    got = _avgpool(x, c, 0, device)
    assert _bits_equal(got, R.avgpool_f32(x, c))
    ref = R.avgpool_ref64(x, c)
    _note("avgpool", got - ref, R.avgpool_bound(x, c, ref))


# -------------------------------------------------------------------------------------------------------------- fc
@pytest.mark.parametrize("cin", R.FC_CIN)
def test_fc_bits_and_fp64(cin, device):
    for cout in R.FC_COUT:
        for n in R.FC_N:
            x, w, sc, sh = R.fc_input(n, cin, cout, cin * 100 + cout + n)
            xd, wd, scd, shd = (_dev(a, device) for a in (x, w, sc, sh))
            runs = []
            for act in (0, 1, 2):
                for s_, t_ in ((None, None), (sc, None), (None, sh), (sc, sh)):
                    out = _sent((n * cout + 16,), device)
                    _call("fcp_fc_f32", xd, wd, scd if s_ is not None else None, shd if t_ is not None else None,
                          n, cin, cout, act, out)
                    runs.append((act, s_, t_, out))
            for act, s_, t_, out in runs:
                what = (cin, cout, n, act, s_ is not None, t_ is not None)
                assert _sentinel_ok(out[n * cout:]), what
                got = out[:n * cout].view(n, cout).cpu().numpy()
                exp = R.fc_f32(x, w, s_, t_, act)
                if act == 2:        # expf / np.exp: EXP_ULP ulp each way
                    d = np.abs(got.view(np.int32).astype(np.int64) - exp.view(np.int32).astype(np.int64))
                    assert d.max() <= R.EXP_ULP, what
                else:
                    assert _bits_equal(got, exp), what
                ref = R.fc_ref64(x, w, s_, t_, act)
                _note(f"fc act{act}", got - ref, R.fc_bound(x, w, s_, t_, act, ref))


# ------------------------------------------------------------------------------------------------------- scale_add
@pytest.mark.parametrize("c", [4, 512])
@pytest.mark.parametrize("addv,addt", [(False, False), (True, False), (False, True), (True, True), (False, "x"),
                                       (True, "x")])
@pytest.mark.parametrize("x_pad,out_pad,t_pad", [(0, 0, 0), (4, 0, 0), (0, 8, 0), (0, 0, 12), (4, 8, 12)])
def test_scale_add_bits_and_fp64(c, addv, addt, x_pad, out_pad, t_pad, device):
    n, hw = 2, 37
    g = R.gen(c + x_pad + out_pad + t_pad)
    xb = torch.randn(n, hw, c + x_pad, generator=g).numpy()
    tb = torch.randn(n, hw, c + t_pad, generator=g).numpy()
    s = torch.rand(n, c, generator=g).numpy()
    av = torch.randn(n, c, generator=g).numpy() if addv else None
    xd = _dev(xb, device)
    if addt == "x":                                     # FFM: feat * atten + feat (add_t is x itself)
        td, t_ld, t_np = xd, c + x_pad, xb[:, :, :c]
    elif addt:
        td, t_ld, t_np = _dev(tb, device), c + t_pad, tb[:, :, :c]
    else:
        td, t_ld, t_np = None, 0, None
    out_ld = c + out_pad
    out = _sent((n, hw, out_ld), device)
    _call("fcp_scale_add_nhwc_f32", xd, c + x_pad, _dev(s, device), _dev(av, device) if av is not None else None, td, t_ld,
          n, hw, c, out, out_ld)
    assert _sentinel_ok(out[..., c:])
    got = out[..., :c].cpu().numpy()
    assert _bits_equal(got, R.scale_add_f32(xb[:, :, :c], s, av, t_np))
    ref = R.scale_add_ref64(xb[:, :, :c], s, av, t_np)
    _note("scale_add", got - ref, R.scale_add_bound(xb[:, :, :c], s, av, t_np))


# ----------------------------------------------------------------------------------------- parse tail + histogram
def _parse(lg, ncls, mh, mw, oh, ow, device, label_off=0):
    f, lh, lw, ld = lg.shape
    hw = oh * ow
    lab = torch.full((f * hw + label_off + 64,), 0xEE, dtype=torch.uint8, device=device)
    cnt = torch.full((f * ncls + 16,), -7, dtype=torch.int32, device=device)
    _call("fcp_parse_tail", _dev(lg, device), f, lh, lw, ld, ncls, mh, mw, oh, ow, (lab, label_off), cnt)
    lab_h, cnt_h = lab.cpu().numpy(), cnt.cpu().numpy()
    assert (lab_h[:label_off] == 0xEE).all() and (lab_h[label_off + f * hw:] == 0xEE).all()
    assert (cnt_h[f * ncls:] == -7).all()
    labels = lab_h[label_off:label_off + f * hw].reshape(f, oh, ow)
    counts = cnt_h[:f * ncls].reshape(f, ncls)
    assert np.array_equal(counts, R.label_counts(labels, ncls)), "class histogram != bincount of the labels"
    return labels


def _check_parse(lg, ncls, mh, mw, out, device, label_off=0):
    labels = _parse(lg, ncls, mh, mw, *out, device, label_off)
    assert np.array_equal(labels, R.parse_tail_f32(lg, ncls, mh, mw, *out))
    bad, worst = R.parse_label_violations(labels, lg, ncls, mh, mw, *out, worst=True)
    assert not bad.any(), f"{int(bad.sum())} labels off the float64 maximum"
    WORST["parse_tail"] = max(WORST.get("parse_tail", 0.0), worst)
    return labels


# every logit layout at the small outputs; the shipped one and the widest at 512^2 and 1024^2
PARSE_MID512 = [(out, ld, ncls) for out in R.PARSE_OUT for ld, ncls in ((19, 19), (20, 19), (32, 19), (19, 1), (32, 32))
                if out[0] * out[1] < 512 * 512 or (ld, ncls) in ((19, 19), (32, 32))]


@pytest.mark.parametrize("out,ld,ncls", PARSE_MID512)
def test_parse_tail_mid512(out, ld, ncls, device):
    lg = R.pad_logits(R.logits_input(1 if out[0] > 512 else 2, 64, 64, ld, ld * 10 + ncls), ncls)
    _check_parse(lg, ncls, 512, 512, out, device)


@pytest.mark.parametrize("out", [(255, 257), (37, 29), (300, 200), (600, 400), (1, 1)])
def test_parse_tail_other_mid(out, device):
    lg = R.pad_logits(R.logits_input(2, 64, 64, 20, 77), 19)
    _check_parse(lg, 19, 300, 200, out, device)


@pytest.mark.parametrize("out,off", [((64, 64), 1), ((64, 64), 2), ((64, 64), 3), ((37, 29), 0), ((37, 29), 2),
                                     ((255, 257), 1)])
def test_parse_hist_unaligned_label_bases(out, off, device):
    """hw % 4 == 0 with a label base 1..3 bytes past a word, and odd hw (face bases then drift through every alignment)."""
    lg = R.pad_logits(R.logits_input(5, 64, 64, 19, 90 + off), 19)
    _check_parse(lg, 19, 512, 512, out, device, label_off=off)


def test_parse_tail_32_faces_past_the_grid_cap(device):
    lg = R.pad_logits(R.logits_input(32, 64, 64, 4, 32), 4)
    labels = _parse(lg, 4, 512, 512, 512, 512, device)
    for i in range(32):
        assert np.array_equal(labels[i], R.parse_tail_f32(lg[i:i + 1], 4, 512, 512, 512, 512)[0]), i
    for i in (0, 31):
        assert not R.parse_label_violations(labels[i:i + 1], lg[i:i + 1], 4, 512, 512, 512, 512).any()


def test_parse_tail_ties_and_nan(device):
    """Class 5 is an exact copy of class 2 (identical interpolated scores): 2 must win every tie.  Two NaN logits (classes 7
    and 8 of one logit pixel) reach every output pixel whose footprint holds them: the first NaN class, 7, wins there."""
    lg = R.pad_logits(R.logits_input(2, 64, 64, 20, 4, ties=(2, 5), nan_at=(1, 10, 20, 7)), 19)
    labels = _check_parse(lg, 19, 512, 512, (512, 512), device)
    assert (labels == 2).mean() > 0.5 and not (labels == 5).any()
    rows = np.isin((np.arange(512) * np.float32(63 / 511)).astype(np.int64), (9, 10))
    cols = np.isin((np.arange(512) * np.float32(63 / 511)).astype(np.int64), (19, 20))
    hit = rows[:, None] & cols[None]
    assert hit.sum() > 0 and (labels[1][hit] == 7).all() and not (labels[0] == 7)[hit].all()


# ------------------------------------------------------------------------------------------------------ label mask
def test_label_mask_every_label_and_bit(device):
    g = R.gen(31)
    total = 16384 * 256 + 4099                              # past the grid cap
    lab = torch.randint(0, 32, (total,), generator=g, dtype=torch.uint8).numpy()
    lab[:32] = np.arange(32)
    ld = _dev(lab, device)
    nat = N()
    for bits in (0, 1, 1 << 31, 0xFFFFFFFF, 0x80000001, (1 << 17) | (1 << 14), 0x9E3779B9,
                 int(torch.randint(0, 2**31, (1,), generator=g)) * 2 + 1):
        mask = torch.full((total + 64,), 0x5A, dtype=torch.uint8, device=device)
        _call("fcp_label_mask_u8", nat.ptr(ld), total, C.c_uint32(bits), nat.ptr(mask))
        m = mask.cpu().numpy()
        assert (m[total:] == 0x5A).all()
        assert np.array_equal(m[:total], R.label_mask(lab, bits)), hex(bits)


# --------------------------------------------------------------------------------------------------- bicubic x0.25
def _bicubic(x4, h, w, device):
    out = torch.full((h * w * 3 + 64,), 0x5A, dtype=torch.uint8, device=device)
    _call("fcp_bicubic_down4_u8", _dev(x4, device), h, w, x4.shape[2], out)
    o = out.cpu().numpy()
    assert (o[h * w * 3:] == 0x5A).all()
    return o[:h * w * 3].reshape(h, w, 3)


@pytest.mark.parametrize("h,w", R.BICUBIC_HW)
@pytest.mark.parametrize("ld", R.BICUBIC_LD)
def test_bicubic_bytes(h, w, ld, device):
    x4 = R.bicubic_input(h, w, ld, h * 31 + w + ld)
    got = _bicubic(x4, h, w, device)
    assert np.array_equal(got, R.bicubic_f32(x4, h, w))
    ref = R.bicubic_ref64(x4, h, w)
    assert not R.bicubic_violations(got, ref, R.bicubic_window(x4)).any()
    assert ((got == 255).any() and (got == 0).any()) or h * w == 1


def test_bicubic_past_the_grid_cap(device):
    """2048 x 2056 outputs (> 16384 blocks of 256 pixels) from an 8192 x 8224 x 3 input (808 MB)."""
    h, w = 2048, 2056
    assert h * w > 16384 * 256
    x4 = R.bicubic_input(h, w, 3, 2048)
    got = _bicubic(x4, h, w, device)
    assert np.array_equal(got, R.bicubic_f32(x4, h, w))
    ref = R.bicubic_ref64(x4, h, w)
    assert not R.bicubic_violations(got, ref, R.bicubic_window(x4)).any()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------- absmax
def _absmax(buf: torch.Tensor, npix, c, ld, fmt, c0=0, init=0.0):
    out = _sent((2,), buf.device)
    out[0] = init
    _call("fcp_absmax_nhwc", N().ptr(buf, 4 * c0), npix, c, ld, fmt, N().ptr(out))
    o = out.cpu().numpy()
    assert _sentinel_ok(out[1:])
    return o[0]


@pytest.mark.parametrize("npix,c,ld,c0", [(1, 8, 8, 0), (1001, 16, 24, 4), (333, 64, 72, 8), (300_000, 64, 64, 0)])
def test_absmax_fp32_exact(npix, c, ld, c0, device):
    """npix * c / 8 = 2.4M lanes in the last case: past the 8192-block grid."""
    g = R.gen(npix + c)
    x = torch.randn(npix, ld, generator=g)
    x[:, :c0] = 1e9                                        # outside the view: never counted
    x[:, c0 + c:] = -1e9
    xd = x.to(device)
    view = lambda a: a[:, c0:c0 + c].numpy()
    assert _absmax(xd, npix, c, ld, 0, c0) == R.absmax_ref(view(x))
    for place in ((0, c0), (npix - 1, c0 + c // 2), (npix // 2, c0 + c - 1), (npix - 1, c0 + c - 1)):
        y = x.clone()
        y[place] = -1000.0                                  # first element, last pixel, last channel
        assert _absmax(y.to(device), npix, c, ld, 0, c0) == np.float32(1000.0), place
    y = x.clone()
    y[npix - 1, c0 + c - 1] = float("nan")
    assert _absmax(y.to(device), npix, c, ld, 0, c0) == np.float32(np.inf)


def test_absmax_special_values(device):
    z = torch.zeros(100, 8, device=device)
    assert _absmax(z, 100, 8, 8, 0) == 0
    assert _absmax(z, 100, 8, 8, 0, init=2.5) == np.float32(2.5)       # the caller's value stays when it is larger
    assert _absmax(torch.full((100, 8), -0.0, device=device), 100, 8, 8, 0) == 0
    sub = torch.zeros(100, 8)
    sub[37, 3] = -float(np.float32(1e-40))                  # subnormal
    sub[99, 7] = float(np.float32(3e-41))
    r = _absmax(sub.to(device), 100, 8, 8, 0)
    assert r == np.float32(1e-40) and r == R.absmax_ref(sub.numpy())
    for v in (float("inf"), -float("inf")):
        t = torch.zeros(100, 8)
        t[50, 5] = v
        assert _absmax(t.to(device), 100, 8, 8, 0) == np.float32(np.inf)


def test_absmax_split32_exact(device):
    """fmt 1 views made by f32_to_split32: a 64-channel tensor and its second 32-channel slice (ld 64 > c 32)."""
    from face_crop_plus_amd import engine as E
    g = R.gen(77)
    npix = 40_000
    x = torch.randn(1, npix, 1, 64, generator=g) * 300
    x[0, npix - 1, 0, 63] = -20000.0
    s = E.f32_to_split32(E.Act(x.to(device)))
    raw = s.buf.reshape(npix, 64).cpu().numpy()
    vals = R.split32_decode(raw)
    assert _absmax(s.buf, npix, 64, 64, 1) == R.absmax_ref(vals) == np.float32(20000.0)
    assert _absmax(s.buf, npix, 32, 64, 1, c0=32) == R.absmax_ref(vals[:, 32:])
    assert _absmax(s.buf, npix, 32, 64, 1, c0=0) == R.absmax_ref(vals[:, :32])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ input converters
SUB_DIV = [((104.0, 117.0, 123.0), 1.0),      # detector: x - mean, no scaling
           ((0.0, 0.0, 0.0), 255.0),          # RRDB: .div(255)
           ((0.5, 1.5, 2.5), 3.0)]


@pytest.mark.parametrize("npix", [1, 2, 3, 4, 1000, 1001, 1002, 1003])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_u8_to_nhwc4_any_input_alignment(npix, off, device):
    g = R.gen(npix * 4 + off)
    buf = torch.randint(0, 256, (npix * 3 + 8,), generator=g, dtype=torch.uint8)
    img = buf[off:off + npix * 3].numpy().reshape(npix, 3)
    bd = buf.to(device)
    for sub, div in SUB_DIV:
        out = _sent((npix * 4 + 16,), device)
        _call("fcp_u8_to_nhwc4_f32", N().ptr(bd, off), N().ptr(out), npix, (C.c_float * 3)(*sub), C.c_float(div))
        assert _sentinel_ok(out[npix * 4:])
        assert _bits_equal(out[:npix * 4].view(npix, 4).cpu().numpy(), R.u8_to_nhwc4_f32(img, sub, div)), (sub, div)


@pytest.mark.parametrize("off", [0, 3])
def test_u8_to_nhwc4_past_the_grid_cap(off, device):
    """8192 blocks x 256 lanes x 4 pixels = 8388608 pixels per grid pass; 4099 more (npix % 4 == 3) need a second pass."""
    npix = 8192 * 256 * 4 + 4099
    g = R.gen(off)
    buf = torch.randint(0, 256, (npix * 3 + 8,), generator=g, dtype=torch.uint8)
    img = buf[off:off + npix * 3].numpy().reshape(npix, 3)
    out = _sent((npix * 4 + 16,), device)
    _call("fcp_u8_to_nhwc4_f32", (buf.to(device), off), out, npix, (C.c_float * 3)(0.0, 0.0, 0.0),
          C.c_float(255.0))
    assert _sentinel_ok(out[npix * 4:])
    assert _bits_equal(out[:npix * 4].view(npix, 4).cpu().numpy(), R.u8_to_nhwc4_f32(img, (0, 0, 0), 255.0))
    del out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (3, 5, 5), (2, 25, 30), (1, 7, 9), (2, 1024, 1024 + 3)])
def test_f32nchw_to_nhwc4(n, h, w, device):
    g = R.gen(n * h * w)
    x = (torch.rand(n, 3, h, w, generator=g) * 255).round()
    x[..., 0, 0] += 0.25                                       # a non-integer value
    for sub, div in SUB_DIV:
        out = _sent((n * h * w * 4 + 16,), device)
        _call("fcp_f32nchw_to_nhwc4_f32", x.to(device), out, n, h, w, (C.c_float * 3)(*sub),
              C.c_float(div))
        assert _sentinel_ok(out[n * h * w * 4:])
        exp = R.u8_to_nhwc4_f32(x.permute(0, 2, 3, 1).reshape(-1, 3).numpy(), sub, div)
        assert _bits_equal(out[:n * h * w * 4].view(-1, 4).cpu().numpy(), exp), (sub, div)


# ------------------------------------------------------------------------------------------------------ integration
@pytest.fixture(scope="module")
def rrdb(device):
    from face_crop_plus_amd import weights
    from face_crop_plus_amd.rrdb import RRDBNet
    return RRDBNet(0.02).load(device, weights.generate_state_dict("rrdb"))


@pytest.mark.parametrize("n,h,w", [(3, 25, 30), (2, 25, 31)])
def test_rrdb_predict_batch_with_unaligned_images(rrdb, n, h, w, device):
    """H * W = 750 puts image 1 at byte 2250 (2 mod 4); 775 (odd) at byte 2325.  Every image is gated in (landmarks=None) and
    must equal the same image enhanced alone, and the float NCHW path."""
    g = R.gen(h * w)
    imgs = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
    batch = rrdb.predict(imgs.clone().to(device), None, None)
    torch.cuda.synchronize()
    assert batch.shape == (n, h, w, 3) and batch.dtype == torch.uint8
    for i in range(n):
        alone = rrdb.predict(imgs[i:i + 1].clone().to(device), None, None)
        assert torch.equal(batch[i], alone[0]), f"image {i} differs from the same image enhanced alone"
        assert not torch.equal(alone[0].cpu(), imgs[i]), f"image {i} was not enhanced"
    flt = rrdb.predict(imgs.permute(0, 3, 1, 2).float().to(device), None, None)
    assert torch.equal(flt, batch.permute(0, 3, 1, 2).float())


def test_bisenet_parse_sub_batches_of_odd_faces(device):
    """5 faces of 37 x 29 with max_batch_size 2 (sub-batches 2, 2, 1; face bases at 3219-byte steps, label bases at 1073):
    every face equals the face parsed alone, and the counts are the bincount of the labels."""
    from face_crop_plus_amd import weights
    from face_crop_plus_amd.bise import BiSeNet
    sd = weights.generate_state_dict("bisenet")
    faces = torch.from_numpy(R.faces_u8(5, 37, 29, 5)).to(device)
    m = BiSeNet(None, None, 2).load(device, sd)
    labels, counts = m.parse(faces)
    lab, cnt = labels.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(cnt, R.label_counts(lab, 19))
    for i in range(5):
        li, ci = m.parse(faces[i:i + 1])
        assert torch.equal(li[0], labels[i]) and torch.equal(ci[0], counts[i]), f"face {i} differs when parsed alone"
