"""The two background-blur launches and the fill kernel at 32 crops of 256 x 256, sigma 8, feather 5 (INTEGRATION.md
section 2i): five warm-up calls of each, then 20, the blur checked against tests/matte_blur_ref.py on one crop.  Run it
from the repository root under a kernel trace of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -o matte_blur -- python tools/trace_matte_blur.py

and read blur_rows_kernel / blur_cols_kernel / matte_kernel from the kernel statistics."""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
spec = importlib.util.spec_from_file_location("_matte_blur_ref", os.path.join("tests", "matte_blur_ref.py"))
R = importlib.util.module_from_spec(spec)
spec.loader.exec_module(R)
from face_crop_plus_amd import matte as M  # noqa: E402

rng = np.random.default_rng(8)
crops = R.MR.random_crops(rng, 32, 256, 256)
labels = np.zeros((32, 256, 256), np.uint8)
labels[:, 48:224, 64:192] = 1                       # a subject in front of a background, as a parsed crop has
labels[:, :, :] ^= (rng.integers(0, 64, labels.shape) == 0).astype(np.uint8)
bits, taps = R.MR.DEFAULT_BITS, M.blur_taps(8.0)
cd, ld = torch.from_numpy(crops).to("cuda:0"), torch.from_numpy(labels).to("cuda:0")
for n in (5, 20):
    for _ in range(n):
        out, _ = M.matte_blur(cd, ld, bits, 5, taps)
        fill, _ = M.matte(cd, ld, bits, 5, (0, 177, 64))
    torch.cuda.synchronize()
want, _ = R.matte_blur(crops[:1, :40], labels[:1, :40], bits, 5, taps)
# rows 0..15 of the strip see nothing below row 39: they equal the full crop's
assert np.array_equal(out[0, :16].cpu().numpy(), want[0, :16])
print("trace body ok", tuple(out.shape), tuple(fill.shape))
