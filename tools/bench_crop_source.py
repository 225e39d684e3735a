"""crop_source="batch" against "original" on synthetic 12 MP photos (4000 x 3000) at resize_size 1024, batch 8 and 32.

    python tools/bench_crop_source.py [--images 64] [--interpolation linear|cubic|lanczos4] [--out FILE]

Prints one JSON line per measurement:
  * device time of the crop stage per batch (CUDA events, median of 20): batch mode = the warp on the resized batch;
    original mode = the INTER_AREA level build plus the ragged warp.  Three faces per image, at crop scales 0.67, 0.25 and
    0.1 (levels 0, 2 and 3), 256^2 crops; and the warps alone for the first 32 of those faces (batch and ragged sources);
  * end-to-end Cropper.process_dir images/s on a directory of JPEGs (generated RetinaFace weights, strategy "largest"),
    second of two runs (skipped with --images 0).
``--interpolation`` picks the filter of every warp (Cropper(interpolation=...)).  Nothing is gated on these numbers.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from face_crop_plus_amd import align  # noqa: E402
from face_crop_plus_amd.batch import build_batch  # noqa: E402

H, W, RS, OUT = 3000, 4000, 1024, (256, 256)


def _images(n, seed=0):
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, 256, (n, H // 16, W // 16, 3), dtype=np.uint8)
    return [np.ascontiguousarray(np.repeat(np.repeat(lo[i], 16, 0), 16, 1)) for i in range(n)]


def _faces(n):
    """Three faces per image: forward transforms source -> crop at scales 0.67, 0.25, 0.1."""
    mats, idx = [], []
    for i in range(n):
        for k, s in enumerate((0.67, 0.25, 0.1)):
            th = 0.1 * (k - 1)
            a, b = s * math.cos(th), s * math.sin(th)
            cx, cy = W * (k + 1) / 4, H / 2
            mats.append([a, -b, OUT[0] / 2 - (a * cx - b * cy), b, a, OUT[1] / 2 - (b * cx + a * cy)])
            idx.append(i)
    return np.array(mats, np.float64), np.array(idx, np.int64)


def _time(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def device_times(n, dev, interp="linear"):
    imgs = _images(n)
    batch, unscales, pads, (blob, table) = build_batch(imgs, RS, "constant", dev, keep_sources=True)
    mats, idx = _faces(n)
    ok = np.ones(len(idx), bool)
    jobs, srcs, mat_l, levels, need = align.plan_sources(table, idx, mats, ok)
    assert need <= blob.numel()
    # batch mode: the same faces on the resized batch (M composed with the batch's un-padded scale)
    mb = mats.copy().reshape(-1, 2, 3)
    r = (1.0 / unscales[idx])[:, None]                       # source px per batch px: x_s = (x_b + 0.5) r - 0.5
    mb[:, :, 2] += (mb[:, :, 0] + mb[:, :, 1]) * (0.5 * r - 0.5)
    mb[:, :, :2] *= r[:, :, None]
    mat_b = torch.from_numpy(mb.reshape(-1, 6)).to(dev)
    idx_d = torch.from_numpy(idx.astype(np.int32)).to(dev)
    pads_d = torch.from_numpy(pads.astype(np.int32)).to(dev)
    ok_d = torch.ones(len(idx), dtype=torch.int32, device=dev)
    mat_ld = torch.from_numpy(mat_l).to(dev)
    ip = {"interpolation": interp}
    t_batch = _time(lambda: align.warp_affine(batch, idx_d, mat_b, ok_d, pads_d, OUT, 0, **ip))
    t_levels = _time(lambda: align.resize_area_ragged(blob, jobs, blob))
    t_warp = _time(lambda: align.warp_affine_ragged(blob, srcs, mat_ld, ok_d, OUT, 0, **ip))
    t_orig = _time(lambda: (align.resize_area_ragged(blob, jobs, blob),
                            align.warp_affine_ragged(blob, srcs, mat_ld, ok_d, OUT, 0, **ip)))
    f32 = min(32, len(idx))
    t_batch32 = _time(lambda: align.warp_affine(batch, idx_d[:f32], mat_b[:f32], ok_d[:f32], pads_d, OUT, 0, **ip))
    t_warp32 = _time(lambda: align.warp_affine_ragged(blob, srcs[:f32], mat_ld[:f32], ok_d[:f32], OUT, 0, **ip))
    level_bytes = sum(j[4] * j[5] * 3 for j in jobs)
    read_bytes = sum(j[1] * j[2] * 3 for j in jobs)
    return {"metric": "crop_stage_device_ms", "interpolation": interp, "batch": n, "faces": len(idx),
            "levels": sorted(set(levels.tolist())), "batch_mode_warp_ms": round(t_batch, 4),
            f"batch_mode_warp_{f32}_faces_ms": round(t_batch32, 4), f"original_warp_{f32}_faces_ms": round(t_warp32, 4), "original_levels_ms": round(t_levels, 4),
            "original_warp_ms": round(t_warp, 4), "original_total_ms": round(t_orig, 4),
            "level_jobs": len(jobs), "level_source_gb_read": round(read_bytes / 1e9, 3),
            "level_gb_written": round(level_bytes / 1e9, 3)}


def end_to_end(n_images, bs, dev, tmp, interp="linear"):
    from PIL import Image
    from face_crop_plus_amd import Cropper
    src = os.path.join(tmp, "in")
    if not os.path.isdir(src):
        os.makedirs(src)
        for i, im in enumerate(_images(n_images, seed=1)):
            Image.fromarray(im).save(os.path.join(src, f"{i:04d}.jpg"), quality=90)
    res = {"metric": "process_dir_images_per_s", "interpolation": interp, "batch": bs, "images": n_images}
    for mode in ("batch", "original"):
        c = Cropper(output_size=OUT, resize_size=RS, strategy="largest", det_threshold=0.6, batch_size=bs, device=dev,
                    weights={"retinaface": "generated"}, crop_source=mode, interpolation=interp)
        rates = []
        for run in range(2):
            out = os.path.join(tmp, f"out_{mode}_{bs}_{run}")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.process_dir(src, out, desc=None)
            torch.cuda.synchronize()
            rates.append(n_images / (time.perf_counter() - t0))
            shutil.rmtree(out, ignore_errors=True)
        res[mode] = round(rates[-1], 1)
    res["original_over_batch"] = round(res["original"] / res["batch"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--interpolation", choices=align.INTERPOLATIONS, default="linear")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [device_times(n, dev, a.interpolation) for n in (8, 32)]
    if a.images > 0:
        tmp = tempfile.mkdtemp(prefix="fcp_crop_source_")
        try:
            lines += [end_to_end(a.images, bs, dev, tmp, a.interpolation) for bs in (8, 32)]
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
