"""Record what OpenCV / torchvision THEMSELVES compute on seeded inputs, so that the "parity unpinned" rows of
DESIGN.md section 4 (a13 estimateAffine*2D, a14 warpAffine, f1 resize / copyMakeBorder, a3 ResNet-50 body)
can be pinned on any machine that has the wheels.  The build container has neither (no network), so the files this
script writes are absent there and `tests/test_third_party_pins.py` skips with that reason; once they exist the same
tests compare BOTH the CPU oracle (`oracle/align_ref.py`, `oracle/batch_ref.py`, `oracle/retinaface_ref.py`) and the HIP
kernels to them.

    pip install opencv-python torchvision          # anywhere with a network
    python tools/make_cv2_fixture.py                # writes tests/golden/opencv_align.npz, opencv_batch.npz,
                                                    #        opencv_interp.npz, opencv_sharpness.npz, opencv_matte.npz,
                                                    #        opencv_clahe.npz,
                                                    #        tests/golden/torchvision_resnet50.npz
    python -m pytest tests/test_third_party_pins.py            # oracle vs the pins (CPU)
    python -m pytest tests/test_third_party_pins.py -m gpu     # kernels vs the pins (MI355X)
    python -m pytest tests/test_warp_interp_pins.py            # cubic / Lanczos-4 restatement (and, -m gpu, kernels)
    python -m pytest tests/test_sharpness_pins.py              # RGB2GRAY + Laplacian restatement (and, -m gpu, the kernel)
    python -m pytest tests/test_matte_pins.py                  # GaussianBlur restatement (and, -m gpu, the kernel's alpha)
    python -m pytest tests/test_clahe_pins.py                  # YCrCb + CLAHE restatement (and, -m gpu, the kernels)

Everything is called exactly the way the reference calls it:
  cropper.py:515-527   cv2.estimateAffinePartial2D / estimateAffine2D(src, dst, ransacReprojThreshold=np.inf)[0]
  cropper.py:542-547   cv2.warpAffine(image, M, dsize, borderMode=cv2.BORDER_*)          (flags default INTER_LINEAR)
                       and the same call with flags=INTER_CUBIC / INTER_LANCZOS4 (Cropper(interpolation=...))
  utils.py:320-335     cv2.resize(image, (ww, hh), interpolation=INTER_AREA | INTER_CUBIC) + cv2.copyMakeBorder
  (not in the reference) cv2.Laplacian(cv2.cvtColor(crop, cv2.COLOR_RGB2GRAY), cv2.CV_64F).var()   (Cropper(min_sharpness=...))
  (not in the reference) cv2.GaussianBlur(mask, (K, K), 0) for K in 3, 5, 7 on 0/255 masks          (Cropper(background=...))
  (not in the reference) cv2.createCLAHE(clip, (g, g)).apply(Y) between cv2.cvtColor(COLOR_RGB2YCrCb / YCrCb2RGB)  (Cropper(clahe=...))
  retinaface.py:93-99  torchvision.models.resnet50() + _utils.IntermediateLayerGetter(layer2, layer3, layer4)
Only data is stored (inputs, outputs, library versions): no third-party source.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

BORDERS = ("constant", "replicate", "reflect", "wrap", "reflect_101")     # codes 0..4 of align.BORDER_MODES


def standard_target(out_w, out_h, face_factor=0.65):
    """The reference's 5-point target (cropper.py:392-439) via this repo's host code (pinned by host_logic.npz)."""
    from face_crop_plus_amd.cropper import landmarks_target
    return landmarks_target((out_w, out_h), face_factor)


def photo_like(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([127 + 90 * np.sin(xx / (17 + 9 * c) + c) * np.cos(yy / (23 - 5 * c)) for c in range(3)], -1)
    img += rng.normal(0, 25, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def describe_cv2(cv2):
    """What produced the numbers: the wheel's version, the CPU baseline / dispatch lines of its build, whether its optimised
    paths were on.  `opencv-python` is unpinned in the reference (setup.py:39) and its warp / resize kernels differ between
    releases and CPU dispatch levels: a fixture must say which algorithm family it records."""
    import platform
    info = cv2.getBuildInformation()
    keep = [ln.strip() for ln in info.splitlines()
            if any(k in ln for k in ("Version control", "CPU/HW features", "Baseline:", "Dispatched code generation", "requested:",
                                     "Use IPP", "Parallel framework", "Platform", "Host:"))
            or ln.strip().startswith(("SSE", "AVX", "NEON", "FP16", "VSX", "RVV"))]
    return {"cv2_version": np.array(cv2.__version__), "cv2_build_cpu": np.array(" | ".join(keep)),
            "cv2_use_optimized": np.array(bool(cv2.useOptimized())), "cv2_num_threads": np.array(int(cv2.getNumThreads())),
            "numpy_version": np.array(np.__version__), "python_version": np.array(platform.python_version()),
            "machine": np.array(platform.machine() + " " + (platform.processor() or ""))}


def make_align(cv2):
    rng = np.random.default_rng(101)
    out = describe_cv2(cv2)
    # ---- estimators: 64 five-point sets (similarity-like faces at several scales / rotations + jitter) and degenerate ones
    tgt = standard_target(256, 256)
    srcs = []
    for i in range(64):
        ang, sc = rng.uniform(-0.6, 0.6), rng.uniform(0.3, 4.0)
        R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]) * sc
        srcs.append((tgt @ R.T + rng.uniform(0, 3000, 2) + rng.normal(0, 2.0 * sc, (5, 2))).astype(np.float32))
    srcs.append(np.full((5, 2), 7.0, np.float32))                         # all points equal
    srcs.append(np.stack([np.linspace(0, 40, 5), np.linspace(0, 40, 5)], 1).astype(np.float32))   # collinear
    srcs = np.stack(srcs)
    for name, fn in (("partial", cv2.estimateAffinePartial2D), ("affine", cv2.estimateAffine2D)):
        mats, ok = np.zeros((len(srcs), 2, 3), np.float64), np.zeros(len(srcs), np.int32)
        for i, s in enumerate(srcs):
            m = fn(s, tgt, ransacReprojThreshold=np.inf)[0]
            if m is not None:
                mats[i], ok[i] = m, 1
        out[f"est_{name}_mat"], out[f"est_{name}_ok"] = mats, ok
    out["est_src"], out["est_dst"] = srcs, tgt
    # ---- warpAffine: 3 source sizes x 5 borders x 4 matrices (incl. one that looks far outside the image)
    k = 0
    for (h, w), (ow, oh) in (((97, 131), (64, 48)), ((240, 320), (128, 128)), ((512, 384), (256, 256))):
        img = photo_like(h, w, 200 + k)
        t = standard_target(ow, oh)
        mats = []
        for j in range(4):
            ang, sc = rng.uniform(-0.5, 0.5), rng.uniform(0.4, 2.5)
            R = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]) * sc
            centre = np.array([w, h]) * (rng.uniform(0.2, 0.8, 2) if j < 3 else np.array([1.1, -0.2]))
            s = ((t - t.mean(0)) @ R.T + centre).astype(np.float32)
            mats.append(cv2.estimateAffinePartial2D(s, t, ransacReprojThreshold=np.inf)[0])
        mats = np.stack(mats)
        out[f"warp{k}_img"], out[f"warp{k}_mat"], out[f"warp{k}_dsize"] = img, mats, np.array([ow, oh])
        for b in BORDERS:
            mode = getattr(cv2, f"BORDER_{b.upper()}")
            out[f"warp{k}_{b}"] = np.stack([cv2.warpAffine(img, m, (ow, oh), borderMode=mode) for m in mats])
            # the same calls with the wheel's optimised (IPP / HAL / SIMD-dispatch) paths switched off: the portable C++
            # implementation of the same release, i.e. the other algorithm family when the two differ
            cv2.setUseOptimized(False)
            try:
                out[f"warp{k}_{b}_noopt"] = np.stack([cv2.warpAffine(img, m, (ow, oh), borderMode=mode) for m in mats])
            finally:
                cv2.setUseOptimized(True)
        k += 1
    out["warp_cases"] = np.array(k)
    # which algorithm family this wheel's warpAffine belongs to, decided against the oracle's two variants exactly as
    # tests/test_third_party_pins.py::_warp_family does; recorded so that a later re-classification fails loudly
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import align_ref as A
    worst = {"fixed": 0, "float32": 0}
    for c in range(k):
        for b in BORDERS:
            for j, m in enumerate(out[f"warp{c}_mat"]):
                for variant in worst:
                    got = A.warp_affine(out[f"warp{c}_img"], m, tuple(int(v) for v in out[f"warp{c}_dsize"]), A.BORDER[b], variant=variant)
                    worst[variant] = max(worst[variant], int(np.abs(got.astype(int) - out[f"warp{c}_{b}"][j].astype(int)).max()))
    out["warp_family"] = np.array("fixed" if worst["fixed"] == 0 else ("float32" if worst["float32"] <= 1 else "unknown"))
    print("warpAffine family of this wheel:", out["warp_family"], worst)
    np.savez_compressed(os.path.join(GOLDEN, "opencv_align.npz"), **out)
    print("wrote opencv_align.npz", {n: v.shape for n, v in out.items() if n.startswith("est")})


def make_batch(cv2):
    """utils.py:320-335 for down-scaling (INTER_AREA) and up-scaling (INTER_CUBIC) inputs, integer and non-integer ratios,
    plus the five border types of copyMakeBorder."""
    out = describe_cv2(cv2)
    cases = [((270, 480), 128), ((135, 240), 256), ((600, 400), 200), ((301, 517), 224), ((64, 48), 160), ((540, 960), 256)]
    for k, ((h, w), size) in enumerate(cases):
        img = photo_like(h, w, 300 + k)
        interp = cv2.INTER_AREA if max(h, w) > size else cv2.INTER_CUBIC
        if (rw := size / w) < (rh := size / h):
            ww, hh = size, int(h * rw)
            pad = [(size - hh) // 2, (size - hh + 1) // 2, 0, 0]
        else:
            ww, hh = int(w * rh), size
            pad = [0, 0, (size - ww) // 2, (size - ww + 1) // 2]
        res = cv2.resize(img, (ww, hh), interpolation=interp)
        out[f"batch{k}_img"], out[f"batch{k}_size"], out[f"batch{k}_resized"] = img, np.array(size), res
        out[f"batch{k}_pad"] = np.array(pad)
        for b in BORDERS:
            out[f"batch{k}_{b}"] = cv2.copyMakeBorder(res, *pad, borderType=getattr(cv2, f"BORDER_{b.upper()}"))
    out["batch_cases"] = np.array(len(cases))
    np.savez_compressed(os.path.join(GOLDEN, "opencv_batch.npz"), **out)
    print("wrote opencv_batch.npz")


def make_interp(cv2):
    """cv2.warpAffine(flags=INTER_CUBIC | INTER_LANCZOS4) on 8UC3 for tests/test_warp_interp_pins.py: random and gradient
    images of 48x64 and 7x9, matrices with rotations, scales 0.3x to 5x, fractional shifts and sources partly or fully
    outside the crop, every border mode."""
    rng = np.random.default_rng(500)
    out = describe_cv2(cv2)
    out["cv2_ipp"] = np.array(" | ".join(ln.strip() for ln in cv2.getBuildInformation().splitlines() if "IPP" in ln))
    k = 0
    for (h, w), (ow, oh) in (((48, 64), (24, 20)), ((7, 9), (20, 16))):
        yy, xx = np.mgrid[0:h, 0:w]
        grad = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 9) % 256], -1).astype(np.uint8)
        for img in (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), grad):
            mats = []
            for j, s in enumerate((0.3, 0.8, 1.0, 1.7, 3.2, 5.0)):
                th = rng.uniform(-np.pi, np.pi) if j % 2 else rng.uniform(-0.3, 0.3)
                a, b = s * np.cos(th), s * np.sin(th)
                c = np.array([(w - 1) / 2, (h - 1) / 2]) + rng.uniform(-0.5, 0.5, 2) * np.array([w, h])
                tx, ty = np.array([(ow - 1) / 2, (oh - 1) / 2]) - np.array([a * c[0] - b * c[1], b * c[0] + a * c[1]])
                mats.append([[a, -b, tx + rng.uniform(-1, 1)], [b, a, ty + rng.uniform(-1, 1)]])
            mats.append([[1.1, 0.2, 3.0 * ow], [-0.2, 1.1, -2.0 * oh]])                # the source fully outside the crop
            mats = np.array(mats, np.float64)
            out[f"interp{k}_img"], out[f"interp{k}_mat"], out[f"interp{k}_dsize"] = img, mats, np.array([ow, oh])
            for name, flag in (("cubic", cv2.INTER_CUBIC), ("lanczos4", cv2.INTER_LANCZOS4)):
                for b in BORDERS:
                    mode = getattr(cv2, f"BORDER_{b.upper()}")
                    out[f"interp{k}_{name}_{b}"] = np.stack([cv2.warpAffine(img, m, (ow, oh), flags=flag, borderMode=mode)
                                                             for m in mats])
            k += 1
    out["interp_cases"] = np.array(k)
    np.savez_compressed(os.path.join(GOLDEN, "opencv_interp.npz"), **out)
    print("wrote opencv_interp.npz")


def make_sharpness(cv2):
    """cv2.Laplacian(cv2.cvtColor(crop, cv2.COLOR_RGB2GRAY), cv2.CV_64F).var() on seeded 8UC3 crops for
    tests/test_sharpness_pins.py: noise, photo-like content, a 0/255 checkerboard, the eight corners of the RGB cube (and
    every single-channel ramp: the rounding of each gray coefficient), sizes with a dimension of 1 and odd sizes."""
    rng = np.random.default_rng(600)
    out = describe_cv2(cv2)
    yy, xx = np.mgrid[0:32, 0:32]
    ramps = np.zeros((3 * 8, 32, 3), np.uint8)                             # channel c takes every value 0..255, the others 0
    for c in range(3):
        ramps[8 * c:8 * c + 8, :, c] = np.arange(256, dtype=np.uint8).reshape(8, 32)
    crops = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((1, 1), (1, 7), (5, 1), (2, 2), (17, 23), (64, 48))]
    crops += [photo_like(96, 80, 601), photo_like(57, 131, 602),
              np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1),
              np.array([[[r, g, b] for g in (0, 255) for b in (0, 255)] for r in (0, 255)], np.uint8), ramps]
    for k, crop in enumerate(crops):
        g = cv2.cvtColor(crop, cv2.COLOR_RGB2GRAY)
        lap = cv2.Laplacian(g, cv2.CV_64F)
        out[f"sharp{k}_crop"], out[f"sharp{k}_gray"], out[f"sharp{k}_laplacian"] = crop, g, lap
        out[f"sharp{k}_var"] = np.array(lap.var())
    out["sharp_cases"] = np.array(len(crops))
    np.savez_compressed(os.path.join(GOLDEN, "opencv_sharpness.npz"), **out)
    print("wrote opencv_sharpness.npz")


def make_matte(cv2):
    """cv2.GaussianBlur(m, (K, K), 0), K in 3, 5, 7, on seeded random 0/255 CV_8U masks for tests/test_matte_pins.py: the
    bit-exact fixed-point path of small kernels with sigma 0 and the default BORDER_REFLECT_101, at sizes below the radius
    (1x1, 1x5, 2x2, 3x2, 2x7: the border is reflected more than once) and above it."""
    rng = np.random.default_rng(700)
    out = describe_cv2(cv2)
    sizes = ((1, 1), (1, 5), (2, 2), (3, 2), (2, 7), (13, 17), (64, 48))
    for k, (h, w) in enumerate(sizes):
        m = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
        out[f"matte{k}_mask"] = m
        for ksize in (3, 5, 7):
            out[f"matte{k}_blur{ksize}"] = cv2.GaussianBlur(m, (ksize, ksize), 0)
    out["matte_cases"] = np.array(len(sizes))
    np.savez_compressed(os.path.join(GOLDEN, "opencv_matte.npz"), **out)
    print("wrote opencv_matte.npz")


def make_clahe(cv2):
    """cv2.cvtColor(crop, COLOR_RGB2YCrCb), cv2.createCLAHE(clip, (g, g)).apply(Y) and cv2.cvtColor(..., COLOR_YCrCb2RGB) on
    seeded crops for tests/test_clahe_pins.py: smooth and noisy content, sides that divide by the grid, that do not, and
    one of each (OpenCV then pads the divisible side by a full grid), a single tile, 2 x 2 pixel tiles, and saturated
    primaries over a ramp, whose way back to RGB clamps in both directions."""
    rng = np.random.default_rng(800)

    def smooth(h, w):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.zeros((h, w, 3))
        for ch in range(3):
            img[..., ch] = rng.uniform(40, 200)
            for _ in range(4):
                cy, cx, s = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, max(h, w) / 2)
                img[..., ch] += rng.uniform(-120, 120) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            img[..., ch] += rng.normal(0, rng.uniform(1, 12), (h, w))
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)

    colours = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (255, 255, 255), (0, 0, 0)])
    primaries = ((colours[(np.arange(48) * 8) // 48][None] * 3 + (np.arange(40) * 255 // 39)[:, None, None]) // 4).astype(np.uint8)
    cases = [(smooth(64, 64), 2.0, 8), (smooth(50, 37), 40.0, 8), (smooth(48, 37), 3.0, 8), (smooth(33, 31), 4.0, 1),
             (smooth(32, 32), 2.0, 16), (rng.integers(0, 256, (96, 80, 3), dtype=np.uint8), 2.0, 8),
             (np.full((64, 64, 3), 93, np.uint8), 0.5, 1), (primaries, 8.0, 4), (smooth(256, 256), 2.0, 8)]
    out = describe_cv2(cv2)
    for k, (crop, clip, grid) in enumerate(cases):
        ycc = cv2.cvtColor(crop, cv2.COLOR_RGB2YCrCb)
        y_eq = cv2.createCLAHE(clipLimit=clip, tileGridSize=(grid, grid)).apply(np.ascontiguousarray(ycc[..., 0]))
        rgb = cv2.cvtColor(np.dstack([y_eq, ycc[..., 1], ycc[..., 2]]), cv2.COLOR_YCrCb2RGB)
        out[f"clahe{k}_crop"], out[f"clahe{k}_clip"], out[f"clahe{k}_grid"] = crop, np.array(clip), np.array(grid)
        out[f"clahe{k}_y"], out[f"clahe{k}_y_eq"], out[f"clahe{k}_rgb"] = ycc[..., 0], y_eq, rgb
    out["clahe_cases"] = np.array(len(cases))
    np.savez_compressed(os.path.join(GOLDEN, "opencv_clahe.npz"), **out)
    print("wrote opencv_clahe.npz")


def make_resnet():
    """retinaface.py:93-99 with the build's generated `body.*` weights: the three feature maps torchvision's own
    ResNet-50 + IntermediateLayerGetter return for one seeded 96x128 input."""
    import torch
    import torchvision
    from torchvision.models import _utils, resnet50
    from face_crop_plus_amd import weights
    sd = weights.generate_state_dict("retinaface")
    body = _utils.IntermediateLayerGetter(resnet50(), {"layer2": 1, "layer3": 2, "layer4": 3})
    own = {k[len("body."):]: v for k, v in sd.items() if k.startswith("body.")}
    missing, unexpected = body.load_state_dict(own, strict=False)
    assert not unexpected and all(m.endswith("num_batches_tracked") for m in missing), (missing, unexpected)
    body.eval()
    x = torch.from_numpy(np.random.default_rng(400).normal(0, 50, (1, 3, 96, 128)).astype(np.float32))
    with torch.no_grad():
        feats = body(x)
    np.savez_compressed(os.path.join(GOLDEN, "torchvision_resnet50.npz"), x=x.numpy(),
                        torchvision_version=np.array(torchvision.__version__), torch_version=np.array(torch.__version__),
                        **{f"feat{k}": v.numpy() for k, v in feats.items()})
    print("wrote torchvision_resnet50.npz", {k: tuple(v.shape) for k, v in feats.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["cv2", "torchvision"], default=None)
    args = ap.parse_args()
    os.makedirs(GOLDEN, exist_ok=True)
    if args.only != "torchvision":
        try:
            import cv2
        except ImportError:
            print("cv2 is not installed: opencv_*.npz not written (pip install opencv-python)")
        else:
            make_align(cv2)
            make_batch(cv2)
            make_interp(cv2)
            make_sharpness(cv2)
            make_matte(cv2)
            make_clahe(cv2)
    if args.only != "cv2":
        try:
            import torchvision  # noqa: F401
        except ImportError:
            print("torchvision is not installed: torchvision_resnet50.npz not written")
        else:
            make_resnet()


if __name__ == "__main__":
    main()
