"""Every conv-engine launch of the shipped operating points, checked against float64 (tests/conv_audit.py).

Each test loads one network with generated (or trained-like) weights while the auditor records the host-folded filters, then
runs it at a production geometry with every ``conv`` / ``bottleneck_chain`` / stem / max-pool launch synchronised and
compared, on a sample of output pixels and all output channels, with a float64 reference of the documented op.  The tiles
are the ones the product picks (tuned tables, autotuner).  Each test also pins the kernel families its operating point
reaches, so an audit that silently skipped one fails.  Last: a detector batch whose layer-1 tensor passes 4 GiB per
launch, which must give the same bits as the same images detected in two halves."""
import gc
import importlib.util
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu


def _load():
    spec = importlib.util.spec_from_file_location("_conv_audit", os.path.join(os.path.dirname(__file__), "conv_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


A = _load()

# kernel families each operating point reaches (labels of a recorded run; conv_audit.conv_family / chain_family).  A tuple:
# any one of them (shapes the shipped tile tables do not hold are timed by the autotuner, whose pick may vary from run to run).
DET_CHAINS = {"stem + conv1", "chain 3x3", "chain 3x3 out@even", "chain pair", "chain two-source"}
DET_F16X3 = DET_CHAINS | {"conv 128 dma", "conv 256", "conv 256 bal", "conv halo", "conv halo-wide"}


@pytest.fixture(scope="module", autouse=True)
def _file_budget():
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    print(f"\nconv audit file: {time.time() - t0:.1f} s, peak device memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")


@pytest.fixture(scope="module")
def sds():
    from face_crop_plus_amd import weights
    return {k: weights.generate_state_dict(k) for k in ("retinaface", "bisenet", "rrdb")}


def _images(n, h, w, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8, device=device)


def _audit(name, load, run, require, seed=0):
    """load() under the weight recorder, run(model) under the launch audit; every family of ``require`` must be reached
    (an entry that is a tuple: any one of its families)."""
    from face_crop_plus_amd import engine as E
    aud = A.Auditor(E, seed=seed)
    with aud.record():
        model = load()
    t0 = time.time()
    try:
        with torch.no_grad(), aud.audit():
            run(model)
        torch.cuda.synchronize()
    finally:
        del model
        aud.forget_weights()
        gc.collect()
        torch.cuda.empty_cache()
    fams = aud.families()
    print(f"{name}: {len(aud.rows)} checks in {time.time() - t0:.1f} s, worst err/tol {aud.worst():.3g}, families {sorted(fams)}")
    missing = [r for r in require if not (set(r) & fams if isinstance(r, tuple) else r in fams)]
    assert not missing, f"{name}: the audit never reached {missing} (reached {sorted(fams)})"
    assert aud.worst() <= 1.0
    return aud


def _detector(device, sd, precision=None, streams=None):
    from face_crop_plus_amd.retinaface import RetinaFace

    def load():
        det = RetinaFace("largest", 0.6).load(device, sd, precision)
        if streams is not None:
            det.streams = streams
        return det
    return load


def test_audit_detector_batch32_1024_two_streams(device, sds):
    """configs[3]'s headline path: two sub-batches of 16 on two streams, each laid out for half of the CUs."""
    imgs = _images(32, 1024, 1024, device, 1)
    _audit("det 32@1024 x2", _detector(device, sds["retinaface"]), lambda d: d.detect(imgs), DET_F16X3)


def test_audit_detector_batch8_1024(device, sds):
    """The reference's default batch (8 @1024^2): one stream, no split."""
    imgs = _images(8, 1024, 1024, device, 2)
    _audit("det 8@1024", _detector(device, sds["retinaface"]), lambda d: d.detect(imgs), DET_F16X3)


def test_audit_detector_batch64_640(device, sds):
    """configs[1]: batch 64 @640^2."""
    imgs = _images(64, 640, 640, device, 3)
    _audit("det 64@640 x2", _detector(device, sds["retinaface"]), lambda d: d.detect(imgs), DET_F16X3)


def test_audit_detector_batch33_1024_one_stream(device, sds):
    """One stream, 33 images @1024^2: layer 1's 256-channel tensors span 33 * 64 MiB, just past 2^31 bytes."""
    assert 33 * 256 * 256 * 256 * 4 > 2**31
    imgs = _images(33, 1024, 1024, device, 4)
    _audit("det 33@1024 x1", _detector(device, sds["retinaface"], streams=1), lambda d: d.detect(imgs),
           DET_CHAINS | {"conv 128 dma", ("conv 256", "conv 256 bal"), ("conv halo", "conv halo-wide")})


def test_audit_detector_trained_like_640(device, sds):
    """In-range trained-like weights (BatchNorm statistics over six decades, heavy tails, residual streams up to 100x)."""
    from face_crop_plus_amd import weights
    sd = weights.trained_like_retinaface(sds["retinaface"], 1)
    imgs = _images(8, 640, 640, device, 5)
    _audit("det trained-like 8@640", _detector(device, sd), lambda d: d.detect(imgs), DET_F16X3)


def test_audit_detector_f32_batch8_1024(device, sds):
    """The exact-fp32 path a checkpoint the split cannot carry falls back to."""
    imgs = _images(8, 1024, 1024, device, 6)
    _audit("det f32 8@1024", _detector(device, sds["retinaface"], "f32"), lambda d: d.detect(imgs), {"conv f32", "maxpool"})


def test_audit_bisenet_32_faces(device, sds):
    """configs[2]'s parse batch: 32 faces in one forward."""
    from face_crop_plus_amd.bise import BiSeNet
    faces = _images(32, 256, 256, device, 7)
    _audit("bisenet 32", lambda: BiSeNet(max_batch_size=32).load(device, sds["bisenet"]), lambda m: m.parse(faces),
           {"stem f32", "conv 128 dma", "conv 128 f16x3", "conv 256", "conv 256 bal", "conv halo", "conv halo-wide"})


def test_audit_rrdb_1024(device, sds):
    """One 1024^2 image: the trunk, the in_up2 convs and the banded x4-resolution tail."""
    from face_crop_plus_amd.rrdb import RRDBNet
    img = _images(1, 1024, 1024, device, 8)
    _audit("rrdb 1024", lambda: RRDBNet(1.0).load(device, sds["rrdb"]), lambda m: m.enhance_u8(img, [0]),
           {"conv 128 f16x3", "conv halo"})


def test_detect_batch_past_4gib_per_launch_matches_two_halves(device, sds):
    """One stream, 65 images @1024^2: layer 1's output of the whole batch would span 65 * 64 MiB >= 4 GiB, past what the
    fp16x3 kernels address.  The detector runs it in chunks; the result equals, bit for bit, the two halves detected alone."""
    from face_crop_plus_amd.retinaface import RetinaFace
    det = RetinaFace("largest", 0.6).load(device, sds["retinaface"])
    det.streams = 1
    n, half = 65, 32
    assert n * 256 * 256 * 256 * 4 >= 2**32 and det._images_per_launch(1024, 1024) < n
    imgs = _images(n, 1024, 1024, device, 9)
    with torch.no_grad():
        full = det.detect(imgs)
        parts = [det.detect(imgs[:half].contiguous()), det.detect(imgs[half:].contiguous())]
    nf = int(full["face_offset"][-1])
    nfs = [int(p["face_offset"][-1]) for p in parts]
    assert nf == sum(nfs) and nf > 0
    lm = torch.cat([p["landmarks"][:k] for p, k in zip(parts, nfs)])
    idx = torch.cat([parts[0]["img_idx"][:nfs[0]], parts[1]["img_idx"][:nfs[1]] + half])
    assert torch.equal(full["landmarks"][:nf], lm)
    assert torch.equal(full["img_idx"][:nf], idx)
    assert torch.equal(full["cand_count"], torch.cat([p["cand_count"] for p in parts]))
    assert torch.equal(full["sel_count"], torch.cat([p["sel_count"] for p in parts]))
    del det, full, parts
    gc.collect()
    torch.cuda.empty_cache()
