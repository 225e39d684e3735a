"""The skin-smoothing launch of `Cropper(smooth_skin=S)` (`fcp_skin_smooth_u8`, S = 10, amount 1.0) at sigma 3 (radius 9, the
default) and sigma 8 (radius 24, the largest) beside the non-local-means launch of `denoise` (`fcp_nlm_denoise_u8`, H = 8),
the step before it, and the two launches of `clahe` (`fcp_clahe_u8`, grid 8, clip 2.0), the step after it, on the same 64
crops of 256 x 256.  Run it from the repository root:

    python tools/bench_skin.py                  device events around 10 calls of each, warmed, the calls alternating, 7 rounds:
                                                microseconds per call
    rocprofv3 --kernel-trace --stats -d <dir> -o skin -- python tools/bench_skin.py --trace
                                                3 warm-up and 10 plain calls of each, no events: read the kernel statistics

The calls go through the C entry points with outputs that exist already: the kernels are timed, not the Python call.
The crops are the synthetic portrait of tests/skin_ref.py with seeded Gaussian noise of sigma 6, and the label maps are
its own: the face ellipse is skin, hair and background are not.  Unlike the non-local-means kernel this one's time depends
on the label map: tiles without skin are copied, runs of 8 pixels without skin skip the window.  So the launch is timed a
second time with every pixel labelled skin, the most it can cost.  One crop of the output is checked against
tests/skin_ref.py first."""
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


R = _load("skin_ref")
from face_crop_plus_amd import _native as N  # noqa: E402
from face_crop_plus_amd import denoise as D  # noqa: E402
from face_crop_plus_amd import skin as S  # noqa: E402

F, H, W, STRENGTH, SIGMAS, NLM, GRID, CLIP, CALLS, ROUNDS = 64, 256, 256, 10, (3.0, 8.0), 8, 8, 2.0, 10, 7
trace = "--trace" in sys.argv
scenes = [R.scene(H, W, seed=seed) for seed in range(F)]
crops = np.stack([sc["noisy"] for sc in scenes])
labels = np.stack([sc["labels"] for sc in scenes])
dev = torch.from_numpy(crops).to("cuda:0")
lab = {"portrait": torch.from_numpy(labels).to("cuda:0"), "all skin": torch.ones((F, H, W), dtype=torch.uint8, device="cuda:0")}
bits = S.check_classes(None)
table = torch.from_numpy(S.range_lut(STRENGTH)).to("cuda:0")
taps = {sigma: S.taps_of(sigma) for sigma in SIGMAS}
taps16 = {sigma: (ctypes.c_uint16 * len(t))(*t) for sigma, t in taps.items()}
lut, shift = D.weight_lut(NLM)
lut_dev = torch.from_numpy(lut).to("cuda:0")
out = torch.empty_like(dev)
dn = torch.empty_like(dev)
eq = torch.empty_like(dev)
luts = torch.empty((F, GRID, GRID, 256), dtype=torch.uint8, device="cuda:0")


def skin_call(sigma, which):
    def call():
        N.check(N.lib().fcp_skin_smooth_u8(N.ptr(dev), N.ptr(lab[which]), F, H, W, bits, taps16[sigma], len(taps[sigma]) - 1,
                                           N.ptr(table), 256, N.ptr(out), N.stream_ptr()), "fcp_skin_smooth_u8")
    return call


def denoise_call():
    N.check(N.lib().fcp_nlm_denoise_u8(N.ptr(dev), F, H, W, N.ptr(lut_dev), len(lut), shift, N.ptr(dn), N.stream_ptr()),
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


calls = {f"skin_smooth sigma {sigma:g}, {which}": skin_call(sigma, which) for which in lab for sigma in SIGMAS}
calls.update({"nlm_denoise": denoise_call, "clahe": clahe_call})
for sigma in SIGMAS:
    skin_call(sigma, "portrait")()
    want = R.smooth_skin(crops[:1], labels[:1], STRENGTH, sigma)
    assert np.array_equal(out[:1].cpu().numpy(), want), sigma
print(json.dumps({"skin_share": round(float((labels == 1).mean()), 3)}), flush=True)
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
                      "of_nlm_denoise": {k: round(med[k] / med["nlm_denoise"], 2) for k in calls if k.startswith("skin")}}), flush=True)
print("bench_skin ok", "trace" if trace else "events")
