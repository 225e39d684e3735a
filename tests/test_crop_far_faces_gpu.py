"""The crop-stage kernels and the device encoders past 2^31 pixels and 2^32 bytes per call: one test per entry point.

Faces are 250 x 250 (no multiple of any tile, so no face starts on a power of two).  Level P31 is f = 34 400 faces: f h w
passes 2^31, so every per-pixel index passes 31 bits, every one-byte plane 2^31 bytes, the crops and every workspace 2^32
bytes.  Level B32 is f = 22 950: the crops pass 2^32 bytes; it is taken where P31 would need more than 64 GiB of device
memory by the entry point's own ``*_workspace_bytes`` (the test asserts that its level is the one this rule gives; the id
states it).  Both are inside the documented f <= 65535.

The batch is filler made on the device (``torch.randint``); a few probe faces take the content of the feature's own case
generator: face 0, face f - 1, the face that holds byte 2^31 and the face that holds byte 2^32 of every buffer of the call
that grows with f (a workspace counts as f equal shares, and as planes of 4- and 8-byte elements per pixel), and the face
that holds pixel 2^31.  Every boundary lies strictly inside its face.  Every probe's output equals the feature's CPU
reference (tests/*_ref.py) for that face alone, byte for byte; and for every probe that lies at byte offset o >= 2^32 of a
written buffer, the faces around o - 2^32 (where a store whose address lost its upper bits would land) equal the kernel's
own output for that filler face in a batch of one.  Lengths and sharpness sums are checked likewise.

Each test is one call of the kernel-level wrapper plus batches of one, frees what it allocated, and skips only where the
device has less free memory than the call needs (the reason gives both numbers)."""
import gc
import importlib.util
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = W = 250
PX = H * W
FACES = {"P31": 34400, "B32": 22950}
LIMIT = 64 << 30                      # of device memory a P31 call may need; above it the test runs at B32
SLOT = 65000                          # bytes of an encoder's slot: about 64 KiB, no power of two (see the probes)
FILL = (12, 200, 77)


def _load(name):
    spec = importlib.util.spec_from_file_location("_far_" + name, os.path.join(os.path.dirname(__file__), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MR, BR, RR, IR, CR = (_load(n) for n in ("matte_ref", "matte_blur_ref", "matte_refine_ref", "matte_image_ref", "cutout_ref"))
SR, KR, CL, DR, UR, VR = (_load(n) for n in ("subject_ref", "mask_shift_ref", "clahe_ref", "denoise_ref", "sharpen_ref", "sharpness_ref"))
EC = _load("encoder_audit_cases")
BITS = MR.DEFAULT_BITS
TAPS = BR.blur_taps(0.5)              # radius 3, the smallest


@pytest.fixture(scope="module", autouse=True)
def _file_budget():
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    print(f"\nfar faces file: {time.time() - t0:.1f} s, peak device memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


def probe_faces(f, sizes, workspace=0):
    """{face: [what it covers]} for buffers of ``sizes`` {name: bytes per face} and a workspace of ``workspace`` bytes."""
    probes = {0: ["face 0"], f - 1: ["face f - 1"]}

    def cover(name, num, den):                                 # the face that holds byte 2^31 / 2^32 of f faces of num / den bytes
        for bits in (31, 32):
            if f * num > den << bits:
                k, r = divmod(den << bits, num)
                assert 0 < r and k < f, (name, bits, "the boundary lies on the edge of a face")
                probes.setdefault(k, []).append(f"byte 2^{bits} of {name}")
    for name, s in sizes.items():
        cover(name, s, 1)
    if workspace:
        cover("the workspace in f shares", workspace, f)
        cover("a workspace plane of 4-byte elements", 4 * PX, 1)
        cover("a workspace plane of 8-byte elements", 8 * PX, 1)
    if f * PX > 1 << 31:
        k, r = divmod(1 << 31, PX)
        assert 0 < r
        probes.setdefault(k, []).append("pixel 2^31")
    return probes


def victim_faces(f, probes, written):
    """The filler faces around o - 2^32 for every probe at byte offset o >= 2^32 of a written buffer."""
    out = set()
    for s in written.values():
        for p in probes:
            if (p + 1) * s > 1 << 32:
                v = (p * s - (1 << 32)) // s
                out |= {k for k in (v, v + 1) if 0 <= k < f and k not in probes}
    return sorted(out)


def far(device, entry, level, ins, outs, workspace_of, content, run, ref):
    """ins {name: (shape behind (f, H, W), exclusive upper bound of the filler)}; outs {name: bytes per face};
    workspace_of(f) -> bytes; content(i, rng) -> {name: array} for probe number i; run(tensors, first face) -> {name:
    tensor}; ref({name: (1, ...) array}, face) -> {name: (1, ...) array}."""
    f = FACES[level]
    in_bytes = {n: PX * int(np.prod(shape, dtype=np.int64)) for n, (shape, _) in ins.items()}
    need = {lv: FACES[lv] * (sum(in_bytes.values()) + sum(outs.values())) + workspace_of(FACES[lv]) for lv in FACES}
    assert level == ("P31" if need["P31"] <= LIMIT else "B32"), (entry, need)
    gc.collect()
    torch.cuda.empty_cache()                                   # what earlier tests left in the caching allocator is not "in use"
    free, _ = torch.cuda.mem_get_info()
    if free < need[level] + (1 << 30):
        pytest.skip(f"{entry} at {level} needs {need[level] + (1 << 30)} bytes of device memory, the device has {free} free")
    probes = probe_faces(f, {**in_bytes, **outs}, workspace_of(f))
    victims = victim_faces(f, probes, outs)
    rng = np.random.default_rng(31)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t = got = None
    try:
        t = {n: torch.randint(0, high, (f, H, W, *shape), dtype=torch.uint8, device=device) for n, (shape, high) in ins.items()}
        faces = {}
        for i, p in enumerate(sorted(probes)):
            faces[p] = {n: np.ascontiguousarray(v, np.uint8) for n, v in content(i, rng).items()}
            for n, v in faces[p].items():
                t[n][p] = torch.from_numpy(v).to(device)
        torch.cuda.synchronize()
        t0 = time.time()
        got = run(t, 0)
        torch.cuda.synchronize()
        seconds = time.time() - t0
        print(f"\n{entry} {level}: f {f}, need {need[level] / 2**30:.1f} GiB, peak {(torch.cuda.max_memory_allocated() - base) / 2**30:.1f} "
              f"GiB, call {seconds:.2f} s, probes {dict(sorted(probes.items()))}, victims {victims}")
        assert set(got) == set(outs)
        for n, s in outs.items():
            assert got[n].shape[0] == f and got[n][0].numel() * got[n].element_size() == s, (entry, n)
        for p in sorted(probes):
            want = ref({n: v[None] for n, v in faces[p].items()}, p)
            for n, w in want.items():
                assert np.array_equal(got[n][p].cpu().numpy(), np.asarray(w)[0]), (entry, level, "probe", p, probes[p], n)
        for v in victims:
            alone = run({n: x[v:v + 1].contiguous() for n, x in t.items()}, v)
            for n in alone:
                assert torch.equal(alone[n][0], got[n][v]), (entry, level, "victim", v, n)
    finally:
        del t, got
        gc.collect()
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------- contents
def _labels(i, rng):
    kinds = (lambda: MR.random_labels(rng, 1, H, W)[0], lambda: MR.checker_labels(1, H, W)[0], lambda: MR.corner_labels(1, H, W)[0])
    return kinds[i % 3]()


def _crops_labels(i, rng):
    return {"crops": MR.random_crops(rng, 1, H, W)[0], "labels": _labels(i, rng)}


def _crops_alpha(i, rng):
    kind = CR.ALPHAS[i % len(CR.ALPHAS)]
    return {"crops": MR.random_crops(rng, 1, H, W)[0], "alpha": CR.alpha_of(kind, rng, 1, H, W)[0]}


def _four(i, rng):
    """The contents of the denoise and sharpen tests: uniform noise, a gradient under noise, the 0 / 255 checkerboard of
    period 1 (maximal patch distances; both clamps of the sharpened value), constant 255 (every weight at its maximum)."""
    y, x = np.mgrid[0:H, 0:W]
    if i % 4 == 0:
        return {"crops": rng.integers(0, 256, (H, W, 3), dtype=np.uint8)}
    if i % 4 == 1:
        ramp = np.stack([30 + 180 * x / (W - 1), 200 - 150 * y / (H - 1), 60 + 60 * (x + y) / (H + W - 2)], -1)
        return {"crops": np.clip(np.rint(ramp + rng.normal(0, 6, (H, W, 3))), 0, 255).astype(np.uint8)}
    if i % 4 == 2:
        return {"crops": np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, -1)}
    return {"crops": np.full((H, W, 3), 255, np.uint8)}


CROPS = {"crops": ((3,), 256)}
CROPS_LABELS = {"crops": ((3,), 256), "labels": ((), 19)}
CROPS_ALPHA = {"crops": ((3,), 256), "alpha": ((), 256)}
LABELS = {"labels": ((), 19)}
BANK = IR.random_bank(np.random.default_rng(5), IR.K, H, W)


def _picks(first, n):
    return [(first + i) % IR.K for i in range(n)]


def _lib():
    from face_crop_plus_amd import _native as N
    return N.lib()


# ---------------------------------------------------------------------------------------------------------- the matte family
def test_matte_P31(device):
    from face_crop_plus_amd import matte as M

    def run(t, first):
        out, alpha = M.matte(t["crops"], t["labels"], BITS, 3, FILL, with_alpha=True)
        return {"out": out, "alpha": alpha}
    far(device, "fcp_matte_u8", "P31", CROPS_LABELS, {"out": 3 * PX, "alpha": PX}, lambda f: 0, _crops_labels, run,
        lambda x, p: dict(zip(("out", "alpha"), MR.matte(x["crops"], x["labels"], BITS, 3, FILL))))


def test_matte_alpha_P31(device):
    from face_crop_plus_amd import matte as M
    far(device, "fcp_matte_alpha_u8", "P31", CROPS_ALPHA, {"out": 3 * PX}, lambda f: 0, _crops_alpha,
        lambda t, first: {"out": M.matte(t["crops"], t["alpha"], BITS, 0, FILL, alpha=t["alpha"])[0]},
        lambda x, p: {"out": MR.composite(x["crops"], x["alpha"], FILL)})


def test_matte_blur_P31(device):
    from face_crop_plus_amd import matte as M

    def run(t, first):
        out, alpha = M.matte_blur(t["crops"], t["labels"], BITS, 3, TAPS, with_alpha=True)
        return {"out": out, "alpha": alpha}
    far(device, "fcp_matte_blur_u8", "P31", CROPS_LABELS, {"out": 3 * PX, "alpha": PX},
        lambda f: _lib().fcp_matte_blur_workspace_bytes(f, H, W), _crops_labels, run,
        lambda x, p: dict(zip(("out", "alpha"), BR.matte_blur(x["crops"], x["labels"], BITS, 3, TAPS))))


def test_matte_blur_alpha_P31(device):
    from face_crop_plus_amd import matte as M
    ins = {**CROPS_LABELS, "alpha": ((), 256)}

    def content(i, rng):
        return {**_crops_labels(i, rng), "alpha": _crops_alpha(i, rng)["alpha"]}
    far(device, "fcp_matte_blur_alpha_u8", "P31", ins, {"out": 3 * PX}, lambda f: _lib().fcp_matte_blur_workspace_bytes(f, H, W),
        content, lambda t, first: {"out": M.matte_blur(t["crops"], t["labels"], BITS, 0, TAPS, alpha=t["alpha"])[0]},
        lambda x, p: {"out": BR.over(x["crops"], x["alpha"], BR.background(x["crops"], x["labels"], BITS, TAPS)[0])})


def test_matte_refine_P31(device):
    from face_crop_plus_amd import matte as M

    def content(i, rng):                                       # the stripes that expose a narrow accumulator, and noise
        if i % 2 == 0:
            crops, labels = RR.stripe_inputs(1, H, W, 1)
            return {"crops": np.roll(crops[0], i, 1), "labels": np.roll(labels[0], i, 1)}
        return {"crops": MR.random_crops(rng, 1, H, W)[0], "labels": rng.integers(0, 2, (H, W), dtype=np.uint8)}
    far(device, "fcp_matte_refine_u8", "P31", {"crops": ((3,), 256), "labels": ((), 2)}, {"alpha": PX},
        lambda f: _lib().fcp_matte_refine_workspace_bytes(f, H, W), content,
        lambda t, first: {"alpha": M.refine_alpha(t["crops"], t["labels"], 1 << 1, 1, 64)},
        lambda x, p: {"alpha": RR.alpha_of(x["crops"], x["labels"], 1 << 1, 1, 64)})


def test_matte_image_P31(device):
    from face_crop_plus_amd import matte as M
    bank = torch.from_numpy(BANK).to(device)

    def run(t, first):
        out, alpha = M.matte_image(t["crops"], t["labels"], BITS, 3, bank, _picks(first, len(t["crops"])), with_alpha=True)
        return {"out": out, "alpha": alpha}
    far(device, "fcp_matte_image_u8", "P31", CROPS_LABELS, {"out": 3 * PX, "alpha": PX}, lambda f: 0, _crops_labels, run,
        lambda x, p: dict(zip(("out", "alpha"), IR.matte_image(x["crops"], x["labels"], BITS, 3, BANK, _picks(p, 1)))))


def test_matte_image_alpha_P31(device):
    from face_crop_plus_amd import matte as M
    bank = torch.from_numpy(BANK).to(device)
    far(device, "fcp_matte_image_alpha_u8", "P31", CROPS_ALPHA, {"out": 3 * PX}, lambda f: 0, _crops_alpha,
        lambda t, first: {"out": M.matte_image(t["crops"], t["alpha"], BITS, 0, bank, _picks(first, len(t["crops"])), alpha=t["alpha"])[0]},
        lambda x, p: {"out": IR.composite(x["crops"], x["alpha"], BANK, _picks(p, 1))})


def test_cutout_B32(device):
    from face_crop_plus_amd import matte as M
    far(device, "fcp_cutout_u8", "B32", CROPS_ALPHA, {"out": 4 * PX}, lambda f: _lib().fcp_cutout_workspace_bytes(f, H, W),
        _crops_alpha, lambda t, first: {"out": M.cutout(t["crops"], t["alpha"], None, TAPS)},
        lambda x, p: {"out": CR.rgba(x["crops"], x["alpha"], TAPS)})


def test_cutout_image_B32(device):
    from face_crop_plus_amd import matte as M
    bank = torch.from_numpy(BANK).to(device)
    far(device, "fcp_cutout_image_u8", "B32", CROPS_ALPHA, {"out": 3 * PX}, lambda f: _lib().fcp_cutout_workspace_bytes(f, H, W),
        _crops_alpha, lambda t, first: {"out": M.cutout_image(t["crops"], t["alpha"], bank, _picks(first, len(t["crops"])), TAPS)},
        lambda x, p: {"out": IR.composite(x["crops"], x["alpha"], BANK, _picks(p, 1), TAPS)})


def test_subject_mask_P31(device):
    from face_crop_plus_amd import matte as M
    patterns = [p for group in SR.GROUPS for p in group]

    def content(i, rng):
        return {"labels": SR.PATTERNS[patterns[(5 * i) % len(patterns)]](rng, H, W)}
    far(device, "fcp_subject_mask_u8", "P31", LABELS, {"out": PX}, lambda f: _lib().fcp_subject_mask_workspace_bytes(f, H, W),
        content, lambda t, first: {"out": M.subject_mask(t["labels"], BITS, True, 64)},
        lambda x, p: {"out": SR.subject_mask(x["labels"], BITS, True, 64)})


def test_mask_shift_P31(device):
    from face_crop_plus_amd import matte as M
    patterns = [p for group in KR.GROUPS for p in group]

    def content(i, rng):
        return {"labels": KR.PATTERNS[patterns[(4 * i) % len(patterns)]](rng, H, W)}
    far(device, "fcp_mask_shift_u8", "P31", LABELS, {"out": PX}, lambda f: 0, content,
        lambda t, first: {"out": M.shift_mask(t["labels"], BITS, 2)}, lambda x, p: {"out": KR.shift_mask(x["labels"], BITS, 2)})


def test_feather_alpha_P31(device):
    from face_crop_plus_amd import matte as M
    far(device, "fcp_feather_alpha_u8", "P31", LABELS, {"alpha": PX}, lambda f: 0, lambda i, rng: {"labels": _labels(i, rng)},
        lambda t, first: {"alpha": M.feather_alpha(t["labels"], BITS, 3)}, lambda x, p: {"alpha": BR.alpha_of(x["labels"], BITS, 3)})


# ---------------------------------------------------------------------------------------------------------- the crop filters
def test_clahe_P31(device):
    from face_crop_plus_amd import clahe as C
    far(device, "fcp_clahe_u8", "P31", CROPS, {"out": 3 * PX}, lambda f: f * 8 * 8 * 256,
        lambda i, rng: {"crops": CL.smooth_crops(100 + i, 1, H, W)[0]},
        lambda t, first: {"out": C.clahe(t["crops"], 2.0, 8)}, lambda x, p: {"out": CL.clahe(x["crops"], 2.0, 8)})


def test_nlm_denoise_P31(device):
    from face_crop_plus_amd import denoise as D
    lut, shift = D.weight_lut(8)
    lut_dev = torch.from_numpy(lut).to(device)
    far(device, "fcp_nlm_denoise_u8", "P31", CROPS, {"out": 3 * PX}, lambda f: 0, _four,
        lambda t, first: {"out": D.nlm(t["crops"], lut_dev, shift)}, lambda x, p: {"out": DR.nlm(x["crops"], lut, shift)})


def test_unsharp_P31(device):
    from face_crop_plus_amd import sharpen as S
    far(device, "fcp_unsharp_u8", "P31", CROPS, {"out": 3 * PX}, lambda f: 0, _four,
        lambda t, first: {"out": S.unsharp(t["crops"], TAPS, 1024, 0)}, lambda x, p: {"out": UR.unsharp(x["crops"], TAPS, 1024, 0)})


def test_crop_sharpness_P31(device):
    from face_crop_plus_amd import align
    far(device, "fcp_crop_sharpness_u8", "P31", CROPS, {"sums": 16}, lambda f: 0, _four,
        lambda t, first: {"sums": align.sharpness_sums(t["crops"])},
        lambda x, p: {"sums": np.array([VR.sums(x["crops"][0])], np.int64)})


# ---------------------------------------------------------------------------------------------------------- the encoders
ENCODER_INS = {"pixels": ((3,), 4)}                            # low-entropy filler: short streams


def _slot(stream):
    slot = np.full(SLOT, 0xA5, np.uint8)
    n = min(len(stream), SLOT)
    slot[:n] = np.frombuffer(stream[:n], np.uint8)
    return slot[None]


def _jpeg(device, entry, subsampling, optimize):
    from face_crop_plus_amd import jpegenc
    lib = _lib()
    ss = EC.O.sub_index(subsampling)

    def run(t, first):
        n = len(t["pixels"])
        out = torch.full((n, SLOT), 0xA5, dtype=torch.uint8, device=device)
        tables = torch.empty((n, 4, 272), dtype=torch.uint8, device=device) if optimize else None
        lengths = jpegenc.encode_scans(t["pixels"], out, 90, subsampling=subsampling, tables=tables)
        return {"out": out, "lengths": lengths, **({"tables": tables} if optimize else {})}

    def ref(x, p):
        scan, records = EC.restate(x["pixels"][0], 90, subsampling)[optimize]
        want = {"out": _slot(scan), "lengths": np.array([len(scan)], np.int32)}
        if optimize:
            want["tables"] = np.frombuffer(records, np.uint8).reshape(1, 4, 272)
        return want
    outs = {"out": SLOT, "lengths": 4, **({"tables": 4 * 272} if optimize else {})}
    far(device, entry, "P31", ENCODER_INS, outs,
        lambda f: lib.fcp_jpeg_workspace_bytes_ex(f, H, W, 3, ss, int(optimize)) if optimize or ss != 2 else lib.fcp_jpeg_workspace_bytes(f, H, W, 3),
        lambda i, rng: {"pixels": EC.J.content(EC.J.CONTENTS[i % 5], H, W, 3, seed=i)}, run, ref)


def test_jpeg_encode_P31(device):
    _jpeg(device, "fcp_jpeg_encode_u8", "4:2:0", False)


def test_jpeg_encode_ex_P31(device):
    _jpeg(device, "fcp_jpeg_encode_ex_u8", "4:4:4", True)


def test_png_encode_P31(device):
    from face_crop_plus_amd import pngenc

    def run(t, first):
        out = torch.full((len(t["pixels"]), SLOT), 0xA5, dtype=torch.uint8, device=device)
        return {"out": out, "lengths": pngenc.encode_streams(t["pixels"], out)}

    def ref(x, p):
        stream = EC.P.encode_stream(x["pixels"][0])
        return {"out": _slot(stream), "lengths": np.array([len(stream)], np.int32)}
    far(device, "fcp_png_encode_u8", "P31", ENCODER_INS, {"out": SLOT, "lengths": 4},
        lambda f: _lib().fcp_png_workspace_bytes(f, H, W, 3),
        lambda i, rng: {"pixels": EC.P.content(EC.P.KINDS[i % 6], H, W, 3, seed=i)}, run, ref)
