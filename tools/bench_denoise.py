"""The non-local-means launch of `Cropper(denoise=H)` (`fcp_nlm_denoise_u8`, H = 8) beside the two launches of `clahe`
(`fcp_clahe_u8`, grid 8, clip 2.0), the step it precedes, on the same 64 crops of 256 x 256.
Run it from the repository root:

    python tools/bench_denoise.py               device events around 10 calls of each, warmed, the two alternating, 7 rounds:
                                                microseconds per call
    rocprofv3 --kernel-trace --stats -d <dir> -o denoise -- python tools/bench_denoise.py --trace
                                                3 warm-up and 10 plain calls of each, no events: read the kernel statistics

The calls go through the C entry points with outputs that exist already: the kernels are timed, not the Python call.
The crops are the synthetic scene of tests/denoise_ref.py, tiled and with seeded Gaussian noise of sigma 10; the time of
the non-local-means kernel does not depend on the content (every offset of every pixel is visited).  One crop of the output
is checked against tests/denoise_ref.py first."""
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


R = _load("denoise_ref")
from face_crop_plus_amd import _native as N  # noqa: E402
from face_crop_plus_amd import denoise as D  # noqa: E402

F, H, W, STRENGTH, GRID, CLIP, CALLS, ROUNDS = 64, 256, 256, 8, 8, 2.0, 10, 7
trace = "--trace" in sys.argv
clean = R.scene(H, W)
crops = np.stack([R.noisy(clean, 10.0, seed) for seed in range(F)])
dev = torch.from_numpy(crops).to("cuda:0")
lut, shift = D.weight_lut(STRENGTH)
lut_dev = torch.from_numpy(lut).to("cuda:0")
out = torch.empty_like(dev)
eq = torch.empty_like(dev)
luts = torch.empty((F, GRID, GRID, 256), dtype=torch.uint8, device="cuda:0")


def denoise_call():
    N.check(N.lib().fcp_nlm_denoise_u8(N.ptr(dev), F, H, W, N.ptr(lut_dev), len(lut), shift, N.ptr(out), N.stream_ptr()),
            "fcp_nlm_denoise_u8")


def clahe_call():
    N.check(N.lib().fcp_clahe_u8(N.ptr(dev), F, H, W, GRID, CLIP, N.ptr(luts), N.ptr(eq), N.stream_ptr()), "fcp_clahe_u8")


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / CALLS          # microseconds per call


calls = {"nlm_denoise": denoise_call, "clahe": clahe_call}
denoise_call()
assert np.array_equal(out[:1].cpu().numpy(), R.nlm(crops[:1], lut, shift))
print(json.dumps({"psnr_db": {"noisy": round(R.psnr(crops[0], clean), 1), "denoised": round(R.psnr(out[0].cpu().numpy(), clean), 1)}}),
      flush=True)
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
    print(json.dumps({"crops": [F, H, W], "strength": STRENGTH,
                      "us_per_call": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1)} for k, v in t.items()},
                      "ratio_of_medians": round(med["nlm_denoise"] / med["clahe"], 1)}), flush=True)
print("bench_denoise ok", "trace" if trace else "events")
