"""The connected-component launches of Cropper(subject=, fill_holes=) at 32 crops of 256 x 256 (INTEGRATION.md section
2l): five warm-up calls, then 20, the output checked against tests/subject_ref.py on two crops.  The first argument is the
label map, `random` (foreground at density 0.41, fractal clusters across every seam) or `parser` (what BiSeNet with
generated weights makes of random crops: noisy maps of many components); the second the options, `su` (subject="largest"),
`fh` (fill_holes=64) or `both`.  Run it from the repository root under a kernel trace of its own, one run per pair, since
the passes share kernels:

    rocprofv3 --kernel-trace --stats -d <dir> -o subject -- python tools/trace_subject.py random both

and read tile_kernel / seam_kernel / flatten_kernel / select_kernel / write_subject_kernel / write_holes_kernel from the
kernel statistics; tools/trace_matte_blur.py and tools/trace_matte_refine.py are the steps to hold them against."""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
spec = importlib.util.spec_from_file_location("_subject_ref", os.path.join("tests", "subject_ref.py"))
S = importlib.util.module_from_spec(spec)
spec.loader.exec_module(S)
from face_crop_plus_amd import matte as M  # noqa: E402

source, options = (sys.argv[1:3] + ["random", "both"][len(sys.argv) - 1:])[:2]
assert source in ("random", "parser") and options in ("su", "fh", "both"), (source, options)
keep, hole = options != "fh", 0 if options == "su" else 64
rng = np.random.default_rng(8)
if source == "random":
    labels = (rng.random((32, 256, 256)) < 0.41).astype(np.uint8)
else:
    from face_crop_plus_amd import Cropper
    lm = (np.zeros((1, 5, 2), np.float32), np.array(["a"]))
    c = Cropper(output_size=256, landmarks=lm, det_threshold=None, device="cuda:0", background=0, weights={"bisenet": "generated"})
    crops = rng.integers(0, 256, (32, 256, 256, 3), dtype=np.uint8)
    labels = c.par_model.parse(torch.from_numpy(crops).to("cuda:0"))[0].cpu().numpy()
bits = S.DEFAULT_BITS
if source == "parser":
    # the classes, most frequent first, whose share together comes nearest one half: subject and background in every map
    share = np.bincount(labels.reshape(-1), minlength=S.NUM_CLASSES)[:S.NUM_CLASSES] / labels.size
    order = np.argsort(-share)
    n = 1 + int(np.argmin(np.abs(np.cumsum(share[order]) - 0.5)))
    bits = sum(1 << int(c) for c in order[:n])
ld = torch.from_numpy(labels).to("cuda:0")
for n in (5, 20):
    for _ in range(n):
        out = M.subject_mask(ld, bits, keep, hole)
    torch.cuda.synchronize()
want = S.subject_mask(labels[:2], bits, keep, hole)
assert np.array_equal(out[:2].cpu().numpy(), want)
hard = S.mask0(labels, bits)
print("trace body ok", source, options, tuple(out.shape), "foreground %.3f -> %.3f" % (hard.mean(), out.float().mean().item()),
      "bits 0x%x, components of face 0: %d" % (bits, len(np.unique(S.components(hard[0], 8)[hard[0]]))))
