"""The composite over pictures of `Cropper(background_image=...)` (`fcp_matte_image_u8`) with a bank of K = 1 and of K = 64
pictures, at feather 0 and 5, beside the composite over a colour (`fcp_matte_u8`) on the same crops and labels, the
kernel it is an instantiation of: 64 crops of 256 x 256.  Run it from the repository root:

    python tools/bench_matte_image.py           device events around 20 calls of each, warmed, the six alternating,
                                                7 rounds: microseconds per call, and the picture kernel's time over the
                                                colour kernel's beside 10 / 7, the ratio of the bytes they move at feather 0
    rocprofv3 --kernel-trace --stats -d <dir> -o matte_image -- python tools/bench_matte_image.py --trace
                                                3 warm-up and 20 plain calls of each, no events: read the kernel statistics

The calls go through the C entry points with outputs that exist already: the kernels are timed, not the Python call.
With K = 64 crop i reads picture i, so no two crops share their fill; with K = 1 all read the same.  The crops and the
pictures are seeded noise, the labels an ellipse of class 1; the time of the kernel does not depend on the content.  One
crop of each output is checked against tests/matte_image_ref.py first."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())


def _load(name):
    spec = importlib.util.spec_from_file_location("_" + name, os.path.join("tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load("matte_image_ref")
from face_crop_plus_amd import _native as N  # noqa: E402

F, H, W, CALLS, ROUNDS = 64, 256, 256, 20, 7
BANKS, FEATHERS, BITS, FILL = (1, 64), (0, 5), 1 << 1, (0, 177, 64)
trace = "--trace" in sys.argv
rng = np.random.default_rng(5)
crops = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
labels = R.CR.disc_labels(F, H, W)
bank = rng.integers(0, 256, (max(BANKS), H, W, 3), dtype=np.uint8)
picks = {k: [i % k for i in range(F)] for k in BANKS}
dev, lab, pictures = (torch.from_numpy(a).to("cuda:0") for a in (crops, labels, bank))
picks_dev = {k: torch.tensor(p, dtype=torch.int32, device="cuda:0") for k, p in picks.items()}
out = torch.empty_like(dev)


def image_call(k, feather):
    def call():
        N.check(N.lib().fcp_matte_image_u8(N.ptr(dev), N.ptr(lab), F, H, W, BITS, feather, N.ptr(pictures), k, N.ptr(picks_dev[k]),
                                           N.ptr(out), None, N.stream_ptr()), "fcp_matte_image_u8")
    return call


def colour_call(feather):
    def call():
        N.check(N.lib().fcp_matte_u8(N.ptr(dev), N.ptr(lab), F, H, W, BITS, feather, *FILL, N.ptr(out), None, N.stream_ptr()),
                "fcp_matte_u8")
    return call


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / CALLS          # microseconds per call


calls = {}
for feather in FEATHERS:
    calls[f"colour_feather_{feather}"] = colour_call(feather)
    for k in BANKS:
        calls[f"image_k{k}_feather_{feather}"] = image_call(k, feather)
        calls[f"image_k{k}_feather_{feather}"]()
        want, _ = R.matte_image(crops[-1:], labels[-1:], BITS, feather, bank, picks[k][-1:])
        assert np.array_equal(out[-1:].cpu().numpy(), want), (k, feather)
for _ in range(3):
    for fn in calls.values():
        fn()
torch.cuda.synchronize()
if trace:
    for _ in range(CALLS):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
else:
    t = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, fn in calls.items():
            t[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in t.items()}
    colour = {feather: f"colour_feather_{feather}" for feather in FEATHERS}
    print(json.dumps({
        "crops": [F, H, W], "bytes_per_pixel": {"colour": 7, "image": 10},
        "us_per_call": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1)} for k, v in t.items()},
        # the run-to-run spread of the colour kernel: (max - min) / median over the rounds
        "colour_spread": {f"feather_{f}": round((max(t[c]) - min(t[c])) / med[c], 3) for f, c in colour.items()},
        "ratio_to_colour": {k: round(med[k] / med[colour[int(k.rsplit("_", 1)[1])]], 3) for k in calls if k.startswith("image")},
        "bytes_ratio": round(10 / 7, 3)}), flush=True)
print("bench_matte_image ok", "trace" if trace else "events")
