"""cv2.GaussianBlur(mask, (K, K), 0) for K in 3, 5, 7 as an OpenCV wheel computes it on 0/255 masks: the restatement
(tests/matte_ref.py) and the device kernel's alpha against ``tests/golden/opencv_matte.npz``, written by
``tools/make_cv2_fixture.py`` where cv2 is installed.  Skips while the file is absent: the taps, the rounding and the
border of the soft edge of ``Cropper(background=...)`` stay unpinned until then."""
import importlib.util
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")


def _fixture():
    path = os.path.join(G, "opencv_matte.npz")
    if not os.path.isfile(path):
        pytest.skip("tests/golden/opencv_matte.npz is absent (no cv2 in the build container): the Gaussian taps, rounding and "
                    "border of Cropper(background=...) stay unpinned; run `python tools/make_cv2_fixture.py` where "
                    "opencv-python is installed and commit the file")
    return np.load(path)


def _ref():
    spec = importlib.util.spec_from_file_location("_matte_ref", os.path.join(os.path.dirname(__file__), "matte_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _cases(z):
    for k in range(int(z["matte_cases"])):
        for ksize in (3, 5, 7):
            yield k, ksize, z[f"matte{k}_mask"], z[f"matte{k}_blur{ksize}"]


def test_reference_equals_opencv():
    z = _fixture()
    R = _ref()
    for k, ksize, m, blur in _cases(z):
        what = f"case {k} {m.shape}, ksize {ksize}, cv2 {z['cv2_version']}"
        assert set(np.unique(m)) <= {0, 255}, what
        assert np.array_equal(R.alpha_separable(m, ksize), blur), what
        assert np.array_equal(R.alpha_direct(m, ksize), blur), what


@pytest.mark.gpu
def test_kernel_alpha_equals_opencv(device):
    from face_crop_plus_amd import matte as M
    z = _fixture()
    for k, ksize, m, blur in _cases(z):
        labels = torch.from_numpy((m // 255).astype(np.uint8))[None].to(device)          # class 1 where the mask is set
        crops = torch.zeros((1, *m.shape, 3), dtype=torch.uint8, device=device)
        _, alpha = M.matte(crops, labels, 1 << 1, ksize, (0, 0, 0), with_alpha=True)
        assert np.array_equal(alpha[0].cpu().numpy(), blur), (k, m.shape, ksize)
