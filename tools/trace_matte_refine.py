"""The two guided-filter launches and the two composites through their alpha at 32 crops of 256 x 256, r 8, eps 64
(INTEGRATION.md section 2k): five warm-up calls of each, then 20, the alpha checked against tests/matte_refine_ref.py on
one crop.  Run it from the repository root under a kernel trace of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -o matte_refine -- python tools/trace_matte_refine.py

and read refine_ab_kernel / refine_alpha_kernel / matte_kernel<0, true> / blur_cols_kernel<0, true> from the kernel
statistics; tools/trace_matte_blur.py is the step to hold them against."""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
spec = importlib.util.spec_from_file_location("_matte_refine_ref", os.path.join("tests", "matte_refine_ref.py"))
R = importlib.util.module_from_spec(spec)
spec.loader.exec_module(R)
from face_crop_plus_amd import matte as M  # noqa: E402

rng = np.random.default_rng(8)
crops = R.MR.random_crops(rng, 32, 256, 256)
labels = np.zeros((32, 256, 256), np.uint8)
labels[:, 48:224, 64:192] = 1                       # a subject in front of a background, as a parsed crop has
labels[:, :, :] ^= (rng.integers(0, 64, labels.shape) == 0).astype(np.uint8)
bits, radius, eps, taps = R.MR.DEFAULT_BITS, 8, 64, M.blur_taps(8.0)
cd, ld = torch.from_numpy(crops).to("cuda:0"), torch.from_numpy(labels).to("cuda:0")
for n in (5, 20):
    for _ in range(n):
        alpha = M.refine_alpha(cd, ld, bits, radius, eps)
        fill, _ = M.matte(cd, ld, bits, 0, (0, 177, 64), alpha=alpha)
        out, _ = M.matte_blur(cd, ld, bits, 0, taps, alpha=alpha)
    torch.cuda.synchronize()
want = R.alpha_of(crops[:1], labels[:1], bits, radius, eps)
assert np.array_equal(alpha[:1].cpu().numpy(), want)
assert np.array_equal(fill[:1].cpu().numpy(), R.MR.composite(crops[:1], want, (0, 177, 64)))
print("trace body ok", tuple(alpha.shape), tuple(fill.shape), tuple(out.shape))
