"""Row a14 with either warpAffine family: the device kernel of the family an OpenCV fixture records (``warp_family``, written
by ``tools/make_cv2_fixture.py``) reproduces that wheel's cv2.warpAffine byte for byte.  Skips, like the other pins, while
``tests/golden/opencv_align.npz`` is absent."""
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), "golden")
BORDERS = ("constant", "replicate", "reflect", "wrap", "reflect_101")


def _fixture():
    path = os.path.join(G, "opencv_align.npz")
    if not os.path.isfile(path):
        pytest.skip("tests/golden/opencv_align.npz is absent (no cv2 in the build container): parity of row a14 stays "
                    "unpinned; run `python tools/make_cv2_fixture.py` where opencv-python is installed and commit the file")
    return np.load(path)


def _recorded_family(z):
    if "warp_family" in z.files:
        return str(z["warp_family"])
    from oracle import align_ref as A                   # older fixture: classify it as tools/make_cv2_fixture.py does
    worst = {v: 0 for v in ("fixed", "float32")}
    for k in range(int(z["warp_cases"])):
        img, mats, dsize = z[f"warp{k}_img"], z[f"warp{k}_mat"], tuple(int(v) for v in z[f"warp{k}_dsize"])
        for b in BORDERS:
            for j, m in enumerate(mats):
                for v in worst:
                    d = np.abs(A.warp_affine(img, m, dsize, A.BORDER[b], variant=v).astype(int) - z[f"warp{k}_{b}"][j]).max()
                    worst[v] = max(worst[v], int(d))
    return "fixed" if worst["fixed"] == 0 else ("float32" if worst["float32"] <= 1 else "unknown")


@pytest.mark.gpu
def test_kernel_of_the_recorded_family_equals_opencv(device):
    from face_crop_plus_amd import align
    from oracle import align_ref as A
    z = _fixture()
    family = _recorded_family(z)
    assert family in align.WARP_FAMILIES, f"cv2 {z['cv2_version']}: warpAffine of neither family ({family!r})"
    for k in range(int(z["warp_cases"])):
        img, mats, dsize = z[f"warp{k}_img"], z[f"warp{k}_mat"], tuple(int(v) for v in z[f"warp{k}_dsize"])
        dimg = torch.from_numpy(img)[None].to(device)
        idx = torch.zeros(len(mats), dtype=torch.int32, device=device)
        dm = torch.from_numpy(mats.reshape(-1, 6)).to(device)
        for b in BORDERS:
            got = align.warp_affine(dimg, idx, dm, None, None, dsize, align.border_code(b), family).cpu().numpy()
            want = z[f"warp{k}_{b}"]
            if np.array_equal(got, want):
                continue
            d = np.abs(got.astype(int) - want.astype(int))
            restated = np.stack([A.warp_affine(img, m, dsize, A.BORDER[b], variant=family) for m in mats])
            where = f"case {k}, border {b}, cv2 {z['cv2_version']}: max |d| {d.max()}, {(d > 0).mean():.2e} of bytes"
            assert np.array_equal(got, restated), f"{where}: the {family} kernel differs from its own oracle restatement"
            if family == "float32":
                pytest.fail(f"{where}: the float32 RESTATEMENT (oracle.align_ref.warp_affine_float32, which the kernel follows "
                            f"byte for byte) disagrees with this OpenCV wheel; the kernel is not what is wrong")
            pytest.fail(f"{where}: the fixed-point kernel and its restatement disagree with a fixed-family wheel")
