"""cv2.Laplacian(cv2.cvtColor(crop, cv2.COLOR_RGB2GRAY), cv2.CV_64F).var() as an OpenCV wheel computes it: the restatement
(tests/sharpness_ref.py) and the device kernel's sums against ``tests/golden/opencv_sharpness.npz``, written by
``tools/make_cv2_fixture.py`` where cv2 is installed.  Skips while the file is absent: the gray coefficients and the Laplacian
stay unpinned until then."""
import importlib.util
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")


def _fixture():
    path = os.path.join(G, "opencv_sharpness.npz")
    if not os.path.isfile(path):
        pytest.skip("tests/golden/opencv_sharpness.npz is absent (no cv2 in the build container): the RGB2GRAY coefficients "
                    "and the Laplacian of min_sharpness stay unpinned; run `python tools/make_cv2_fixture.py` where "
                    "opencv-python is installed and commit the file")
    return np.load(path)


def _ref():
    spec = importlib.util.spec_from_file_location("_sharpness_ref", os.path.join(os.path.dirname(__file__), "sharpness_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cases(z):
    for k in range(int(z["sharp_cases"])):
        yield k, z[f"sharp{k}_crop"], z[f"sharp{k}_gray"], z[f"sharp{k}_laplacian"], float(z[f"sharp{k}_var"])


def test_reference_equals_opencv():
    z = _fixture()
    R = _ref()
    for k, crop, g, lap, var in _cases(z):
        what = f"case {k} {crop.shape}, cv2 {z['cv2_version']}"
        assert np.array_equal(R.gray(crop), g), what
        assert np.array_equal(R.laplacian(g).astype(np.float64), lap), what          # integers below 2^53: exact in CV_64F
        assert abs(R.score(crop) - var) <= 1e-9 * max(var, 1e-300), what             # ndarray.var()'s summation order


@pytest.mark.gpu
def test_kernel_sums_equal_opencv(device):
    from face_crop_plus_amd import align
    z = _fixture()
    for k, crop, g, lap, var in _cases(z):
        lap = lap.astype(np.int64)
        want = [[int(lap.sum()), int((lap * lap).sum())]]
        got = align.sharpness_sums(torch.from_numpy(np.ascontiguousarray(crop))[None].to(device))
        assert got.cpu().tolist() == want, (k, crop.shape)
        score = align.sharpness_score(got, crop.shape[0] * crop.shape[1])[0]
        assert abs(score - var) <= 1e-9 * max(var, 1e-300), (k, crop.shape)
