"""``ConvStats.replay`` (per-launch relaunch capture) against ``ConvStats.timing``, on both launch boundaries.

tools/launch_ledger.py times a step with per-launch events, captures the same step's relaunch closures and pairs the two lists
position by position; bench.py's launch table reads the timing list alone.  Every accounted launch must therefore be
captured, whichever boundary (registered op or C ABI) it took, and a relaunch must be repeatable without changing what
the step computed."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _images(n, h, w, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8, device=device)


def _detector(device):
    from face_crop_plus_amd import weights
    from face_crop_plus_amd.retinaface import RetinaFace
    det = RetinaFace("largest", 0.6).load(device, weights.generate_state_dict("retinaface"))
    det.streams = 1
    imgs = _images(2, 192, 256, device, 1)
    return lambda: det.detect(imgs)


def _bisenet(device):
    from face_crop_plus_amd import weights
    from face_crop_plus_amd.bise import BiSeNet
    m = BiSeNet(None, None, 2).load(device, weights.generate_state_dict("bisenet"))
    faces = _images(2, 64, 48, device, 2)
    return lambda: m.parse(faces)


def _rrdb(device):
    from face_crop_plus_amd import weights
    from face_crop_plus_amd.rrdb import RRDBNet
    m = RRDBNet(1.0).load(device, weights.generate_state_dict("rrdb"))
    img = _images(1, 24, 32, device, 3)
    return lambda: m.enhance_u8(img.clone(), [0])


@pytest.mark.parametrize("boundary", ["op", "ctypes"])
@pytest.mark.parametrize("model", [_detector, _bisenet, _rrdb], ids=["detector", "bisenet", "rrdb"])
def test_capture_matches_timing(device, model, boundary, monkeypatch):
    """One step timed, the same step captured: equal length, and equal label, FLOP and bytes at every position.  Each
    captured relaunch then runs once (the ledger's first use of it)."""
    from face_crop_plus_amd import engine as E, torch_ops as T
    monkeypatch.setattr(T, "ENABLED", boundary == "op")
    monkeypatch.setattr(E.Autotune, "enabled", False)       # no tuning between the two steps: the same tiles, the same labels
    step = model(device)
    with torch.no_grad():
        step()
        torch.cuda.synchronize()
        try:
            E.ConvStats.timing = []
            step()
            torch.cuda.synchronize()
            timing, E.ConvStats.timing = E.ConvStats.timing, None
            E.ConvStats.replay = []
            step()
            torch.cuda.synchronize()
            replay = E.ConvStats.replay
        finally:
            E.ConvStats.timing = E.ConvStats.replay = None
        assert len(timing) > 0
        assert [(t[3], t[2], t[4]) for t in timing] == [(r[0], r[1], r[2]) for r in replay]
        for r in replay:
            r[3]()
        torch.cuda.synchronize()


@pytest.mark.parametrize("boundary", ["op", "ctypes"])
def test_aliased_relaunch_is_idempotent(device, boundary, monkeypatch):
    """RRDB's last dense-block conv: the output view overlaps the second residual.  Relaunching it must leave the output as the
    live launch wrote it (the relaunch writes a scratch tensor), not add the residual again on every call."""
    from face_crop_plus_amd import engine as E, torch_ops as T
    monkeypatch.setattr(T, "ENABLED", boundary == "op")
    g = torch.Generator().manual_seed(5)
    with E.default_precision("f16x3"):
        pc = E.pack_conv(torch.randn(64, 192, 3, 3, generator=g) * 0.05, torch.randn(64, generator=g) * 0.1, stride=1, pad=1,
                         device=device)
    b = E.f32_to_split32(E.Act(torch.randn(1, 24, 32, 192, generator=g).to(device)))
    nxt = E.f32_to_split32(E.Act(torch.randn(1, 24, 32, 192, generator=g).to(device)))
    try:
        E.ConvStats.replay = []
        E.conv(pc, b, nxt.slice(0, 64), alpha=0.2, res1=b.slice(0, 64), res1_pre=False, res2=nxt.slice(0, 64), alpha2=0.2)
        torch.cuda.synchronize()
        replay = E.ConvStats.replay
    finally:
        E.ConvStats.replay = None
    assert len(replay) == 1
    snap = nxt.buf.clone()
    for _ in range(3):
        replay[0][3]()
    torch.cuda.synchronize()
    assert torch.equal(nxt.buf, snap)
