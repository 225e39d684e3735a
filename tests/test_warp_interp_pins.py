"""cv2.warpAffine(INTER_CUBIC / INTER_LANCZOS4) as an OpenCV wheel computes it: the restatement (tests/warp_interp_ref.py)
and both device kernels against ``tests/golden/opencv_interp.npz``, written by ``tools/make_cv2_fixture.py`` where cv2 is
installed.  Skips while the file is absent: the restatement stays unpinned until then."""
import importlib.util
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
BORDERS = ("constant", "replicate", "reflect", "wrap", "reflect_101")
METHODS = {"cubic": 2, "lanczos4": 4}


def _fixture():
    path = os.path.join(G, "opencv_interp.npz")
    if not os.path.isfile(path):
        pytest.skip("tests/golden/opencv_interp.npz is absent (no cv2 in the build container): cubic / Lanczos-4 warpAffine "
                    "stays unpinned; run `python tools/make_cv2_fixture.py` where opencv-python is installed and commit "
                    "the file")
    return np.load(path)


def _ref():
    spec = importlib.util.spec_from_file_location("_warp_interp_ref", os.path.join(os.path.dirname(__file__),
                                                                                   "warp_interp_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cases(z):
    for k in range(int(z["interp_cases"])):
        img, mats, dsize = z[f"interp{k}_img"], z[f"interp{k}_mat"], tuple(int(v) for v in z[f"interp{k}_dsize"])
        for m in METHODS:
            for bi, b in enumerate(BORDERS):
                yield k, img, mats, dsize, m, bi, z[f"interp{k}_{m}_{b}"]


def test_reference_equals_opencv():
    z = _fixture()
    R = _ref()
    for k, img, mats, dsize, m, b, want in _cases(z):
        for j, M in enumerate(mats):
            got = R.warp_affine_interp(img, M, dsize, b, METHODS[m])
            assert np.array_equal(got, want[j]), (f"case {k}, matrix {j}, {m}, border {BORDERS[b]}, cv2 {z['cv2_version']}: "
                                                  f"max |d| {np.abs(got.astype(int) - want[j].astype(int)).max()}")


@pytest.mark.gpu
def test_kernels_equal_opencv(device):
    from face_crop_plus_amd import align
    from face_crop_plus_amd.batch import upload_sources
    z = _fixture()
    for k, img, mats, dsize, m, b, want in _cases(z):
        idx = torch.zeros(len(mats), dtype=torch.int32, device=device)
        dm = torch.from_numpy(np.ascontiguousarray(mats).reshape(-1, 6)).to(device)
        got = align.warp_affine(torch.from_numpy(img)[None].to(device), idx, dm, None, None, dsize, b,
                                interpolation=m).cpu().numpy()
        assert np.array_equal(got, want), (k, m, BORDERS[b], "batch")
        blob, table = upload_sources([img], device)
        got = align.warp_affine_ragged(blob, np.repeat(table, len(mats), 0), dm, None, dsize, b,
                                       interpolation=m).cpu().numpy()
        assert np.array_equal(got, want), (k, m, BORDERS[b], "ragged")
