"""cv2.createCLAHE(clip, (grid, grid)).apply(Y) between cv2.cvtColor(COLOR_RGB2YCrCb) and COLOR_YCrCb2RGB as an OpenCV
wheel computes them: the restatement (tests/clahe_ref.py) and the device kernels against ``tests/golden/opencv_clahe.npz``,
written by ``tools/make_cv2_fixture.py`` where cv2 is installed.  Skips while the file is absent: the colour conversion,
the clip / redistribute rule, the LUT rounding and the interpolation of ``Cropper(clahe=...)`` stay unpinned until then."""
import importlib.util
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")


def _fixture():
    path = os.path.join(G, "opencv_clahe.npz")
    if not os.path.isfile(path):
        pytest.skip("tests/golden/opencv_clahe.npz is absent (no cv2 in the build container): the colour conversion, LUTs and "
                    "interpolation of Cropper(clahe=...) stay unpinned; run `python tools/make_cv2_fixture.py` where "
                    "opencv-python is installed and commit the file")
    return np.load(path)


def _ref():
    spec = importlib.util.spec_from_file_location("_clahe_ref", os.path.join(os.path.dirname(__file__), "clahe_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cases(z):
    for k in range(int(z["clahe_cases"])):
        yield k, z[f"clahe{k}_crop"], float(z[f"clahe{k}_clip"]), int(z[f"clahe{k}_grid"]), z[f"clahe{k}_y"], z[f"clahe{k}_y_eq"], \
            z[f"clahe{k}_rgb"]


def test_reference_equals_opencv():
    z = _fixture()
    R = _ref()
    for k, crop, clip, grid, y, y_eq, rgb in _cases(z):
        what = f"case {k} {crop.shape}, clip {clip}, grid {grid}, cv2 {z['cv2_version']}"
        d = R.clahe_full(crop, clip, grid)
        assert np.array_equal(d["y"], y), what
        assert np.array_equal(d["y_eq"], y_eq), what
        assert np.array_equal(d["rgb"], rgb), what


@pytest.mark.gpu
def test_kernels_equal_opencv(device):
    from face_crop_plus_amd import clahe as C
    z = _fixture()
    for k, crop, clip, grid, y, y_eq, rgb in _cases(z):
        out = C.clahe(torch.from_numpy(np.ascontiguousarray(crop))[None].to(device), clip, grid)
        assert np.array_equal(out[0].cpu().numpy(), rgb), (k, crop.shape, clip, grid)
