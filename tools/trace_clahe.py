"""The two CLAHE launches at 32 crops of 256 x 256, grid 8, clip 2.0: five warm-up calls, then
20, checked against tests/clahe_ref.py.  Run it from the repository root under a kernel trace of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -o clahe -- python tools/trace_clahe.py

and read clahe_lut_kernel / clahe_apply_kernel from the kernel statistics."""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
spec = importlib.util.spec_from_file_location("_clahe_ref", os.path.join("tests", "clahe_ref.py"))
R = importlib.util.module_from_spec(spec)
spec.loader.exec_module(R)
from face_crop_plus_amd import clahe as C  # noqa: E402

crops = np.concatenate([R.smooth_crops(900 + k, 4, 256, 256) for k in range(8)])
dev = torch.from_numpy(crops).to("cuda:0")
for _ in range(5):
    out = C.clahe(dev, 2.0, 8)
torch.cuda.synchronize()
for _ in range(20):
    out = C.clahe(dev, 2.0, 8)
torch.cuda.synchronize()
want = R.clahe(crops[:2], 2.0, 8)
assert np.array_equal(out[:2].cpu().numpy(), want)
print("trace body ok", tuple(out.shape))
