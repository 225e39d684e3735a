"""The cut-out with the subject-colour estimate (`fcp_cutout_u8`, RGBA) against the background blur it is modelled on
(`fcp_matte_blur_u8`) at the same taps: 64 crops of 256 x 256, sigma 4 and 16.  Run it from
the repository root:

    python tools/bench_cutout.py            device events around groups of 20 warmed calls, the two alternating, 7 groups
    rocprofv3 --kernel-trace --stats -d <dir> -o cutout -- python tools/bench_cutout.py --trace
                                            5 warm-up and 20 calls of each, no events: read the kernel statistics

Two alpha planes: "disc", the feathered (5) mask of an ellipse, what a parsed crop gives (most 128 x 8 tiles hold no
soft pixel and skip their taps), and "noise", uniform random bytes (every tile is an edge tile: the whole workspace is
read).  The blur runs on the ellipse's labels with feather 5 in both cases (its time does not depend on the mask).  One
crop of each output is checked against tests/cutout_ref.py first."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
spec = importlib.util.spec_from_file_location("_cutout_ref", os.path.join("tests", "cutout_ref.py"))
R = importlib.util.module_from_spec(spec)
spec.loader.exec_module(R)
from face_crop_plus_amd import matte as M  # noqa: E402

F, H, W, CALLS, GROUPS = 64, 256, 256, 20, 7
trace = "--trace" in sys.argv
rng = np.random.default_rng(8)
crops = R.MR.random_crops(rng, F, H, W)
labels = R.disc_labels(F, H, W)
bits = 1 << 1
cd, ld = torch.from_numpy(crops).to("cuda:0"), torch.from_numpy(labels).to("cuda:0")
planes = {"disc": M.feather_alpha(ld, bits, 5), "noise": torch.from_numpy(rng.integers(0, 256, (F, H, W), dtype=np.uint8)).to("cuda:0")}
soft = {k: float(((v > 0) & (v < 255)).float().mean().item()) for k, v in planes.items()}


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(CALLS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / CALLS          # microseconds per call


for sigma in (4.0, 16.0):
    taps = M.blur_taps(sigma)
    for kind, plane in planes.items():
        cut = lambda: M.cutout(cd, plane, None, taps)
        blur = lambda: M.matte_blur(cd, ld, bits, 5, taps)
        got = cut()[:1].cpu().numpy()
        assert np.array_equal(got, R.rgba(crops[:1], plane[:1].cpu().numpy(), taps)), (sigma, kind)
        for _ in range(5):
            cut(), blur()
        torch.cuda.synchronize()
        if trace:
            for _ in range(CALLS):
                cut(), blur()
            torch.cuda.synchronize()
            continue
        t = {"cutout": [], "matte_blur": []}
        for _ in range(GROUPS):
            t["cutout"].append(timed(cut))
            t["matte_blur"].append(timed(blur))
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps({"sigma": sigma, "radius": len(taps) - 1, "alpha": kind, "soft_share": round(soft[kind], 4),
                          "us_per_call": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                                          for k, v in t.items()},
                          "ratio_of_medians": round(med["cutout"] / med["matte_blur"], 3)}), flush=True)
print("bench_cutout ok", "trace" if trace else "events")
