"""The unsharp-mask launch of `Cropper(sharpen=A)` (`fcp_unsharp_u8`, amount 1.0, threshold 0) at sigma 1.5 (radius 5, the
32 x 64 tiles) and sigma 16 (radius 48, the 48 x 64 tiles), beside the two launches of `clahe` (`fcp_clahe_u8`, grid 8,
clip 2.0), the step it follows, and a device-to-device copy of the same bytes, all on the same 64 crops of 256 x 256
(INTEGRATION.md section 2q).  Run it from the repository root:

    python tools/bench_sharpen.py               device events around 20 calls of each, warmed, the four alternating,
                                                7 rounds: microseconds per call
    rocprofv3 --kernel-trace --stats -d <dir> -o sharpen -- python tools/bench_sharpen.py --trace
                                                3 warm-up and 20 plain calls of each, no events: read the kernel statistics

The calls go through the C entry points with outputs that exist already: the kernels are timed, not the Python call.
The crops are seeded: a smooth gradient plus noise; the time of the kernel does not depend on the content.  One crop of
each output is checked against tests/sharpen_ref.py first."""
import ctypes
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


R = _load("sharpen_ref")
from face_crop_plus_amd import _native as N  # noqa: E402
from face_crop_plus_amd import matte as M  # noqa: E402
from face_crop_plus_amd import sharpen as S  # noqa: E402

F, H, W, AMOUNT, THRESHOLD, GRID, CLIP, CALLS, ROUNDS = 64, 256, 256, 1.0, 0, 8, 2.0, 20, 7
SIGMAS = (1.5, 16)
trace = "--trace" in sys.argv
rng = np.random.default_rng(5)
y, x = np.mgrid[0:H, 0:W]
ramp = np.stack([30 + 180 * x / (W - 1), 200 - 150 * y / (H - 1), 60 + 60 * (x + y) / (H + W - 2)], -1)
crops = np.clip(np.rint(ramp[None] + rng.normal(0, 12, (F, H, W, 3))), 0, 255).astype(np.uint8)
dev = torch.from_numpy(crops).to("cuda:0")
out = torch.empty_like(dev)
eq = torch.empty_like(dev)
copy = torch.empty_like(dev)
luts = torch.empty((F, GRID, GRID, 256), dtype=torch.uint8, device="cuda:0")
taps = {s: M.blur_taps(s) for s in SIGMAS}
taps16 = {s: (ctypes.c_uint16 * len(t))(*t) for s, t in taps.items()}
amount_q = S.amount_q8(AMOUNT)


def unsharp_call(sigma):
    def call():
        N.check(N.lib().fcp_unsharp_u8(N.ptr(dev), F, H, W, taps16[sigma], len(taps[sigma]) - 1, amount_q, THRESHOLD, N.ptr(out),
                                       N.stream_ptr()), "fcp_unsharp_u8")
    return call


def clahe_call():
    N.check(N.lib().fcp_clahe_u8(N.ptr(dev), F, H, W, GRID, CLIP, N.ptr(luts), N.ptr(eq), N.stream_ptr()), "fcp_clahe_u8")


def copy_call():
    copy.copy_(dev)


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / CALLS          # microseconds per call


calls = {f"unsharp_sigma_{s:g}": unsharp_call(s) for s in SIGMAS}
calls.update({"clahe": clahe_call, "copy": copy_call})
for s in SIGMAS:
    calls[f"unsharp_sigma_{s:g}"]()
    assert np.array_equal(out[:1].cpu().numpy(), R.unsharp(crops[:1], taps[s], amount_q, THRESHOLD)), s
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
    print(json.dumps({"crops": [F, H, W], "bytes_moved": 2 * dev.numel(), "radius": {f"{s:g}": len(taps[s]) - 1 for s in SIGMAS},
                      "us_per_call": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1)} for k, v in t.items()},
                      "ratio_to_copy": {k: round(med[k] / med["copy"], 2) for k in calls if k != "copy"}}), flush=True)
print("bench_sharpen ok", "trace" if trace else "events")
