"""The matte's grow / shrink (`fcp_mask_shift_u8`) beside the feather it precedes (`fcp_feather_alpha_u8`, feather 5) on
the same label maps: 64 crops of 256 x 256, |shift| 2, 8 and 64 in both directions.  Run it
from the repository root:

    python tools/bench_mask_shift.py            device events around replays of a captured graph of 20 launches, warmed,
                                                the kernels alternating, 9 replays each: microseconds per launch
    rocprofv3 --kernel-trace --stats -d <dir> -o mask_shift -- python tools/bench_mask_shift.py --trace
                                                5 warm-up and 20 plain calls of each, no events: read the kernel statistics

The launches go through the C entry points with outputs that exist already, so a replay holds kernels only: the kernel
is timed, not the Python call.  The label maps are the ellipses of tests/cutout_ref.py, what a parsed crop looks like;
neither kernel's time depends on the mask.  One crop of every output is checked against tests/mask_shift_ref.py first."""
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


R, C = _load("mask_shift_ref"), _load("cutout_ref")
from face_crop_plus_amd import _native as N  # noqa: E402

F, H, W, CALLS, REPLAYS = 64, 256, 256, 20, 9
trace = "--trace" in sys.argv
labels = C.disc_labels(F, H, W)
bits = R.SUBJECT_BITS
ld = torch.from_numpy(labels).to("cuda:0")
out = torch.empty_like(ld)
alpha = torch.empty_like(ld)


def shift_call(shift):
    return lambda: N.check(N.lib().fcp_mask_shift_u8(N.ptr(ld), F, H, W, bits, shift, N.ptr(out), N.stream_ptr()), "fcp_mask_shift_u8")


def feather_call():
    N.check(N.lib().fcp_feather_alpha_u8(N.ptr(ld), F, H, W, bits, 5, N.ptr(alpha), N.stream_ptr()), "fcp_feather_alpha_u8")


def captured(fn):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(CALLS):
            fn()
    return graph


def timed(graph):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    graph.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / CALLS          # microseconds per launch


for shift in (2, -2, 8, -8, 64, -64):
    call = shift_call(shift)
    call()
    assert np.array_equal(out[:1].cpu().numpy(), R.shift_mask(labels[:1], bits, shift)), shift
    for _ in range(5):
        call(), feather_call()
    torch.cuda.synchronize()
    if trace:
        for _ in range(CALLS):
            call(), feather_call()
        torch.cuda.synchronize()
        continue
    graphs = {"mask_shift": captured(call), "feather_alpha": captured(feather_call)}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    t = {k: [] for k in graphs}
    for _ in range(REPLAYS):
        for k, g in graphs.items():
            t[k].append(timed(g))
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps({"shift": shift, "us_per_launch": {k: {"median": round(med[k], 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                                                        for k, v in t.items()},
                      "ratio_of_medians": round(med["mask_shift"] / med["feather_alpha"], 2)}), flush=True)
print("bench_mask_shift ok", "trace" if trace else "events")
