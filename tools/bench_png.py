"""The timings of INTEGRATION.md section 2m (Cropper(png_encoder=...)), in one process on one machine:

  1. Pillow at compress_level=1 per 256x256x3 crop and per 256x256 mask, on this machine's CPU (one thread);
  2. pngenc.encode_streams for 32 such crops and for 32 such masks, device events around warmed calls, the same pixels, and the
     bytes that come back per face against the raw size;
  3. process_dir(output_format="png") over generated images with a landmark table and crop_source="original", with
     png_encoder="host" and "device", alternating, same worker settings.

    python tools/bench_png.py [n_files] [size] [repeats]
"""
import io
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from face_crop_plus_amd import Cropper, pngenc
from face_crop_plus_amd.cropper import landmarks_target

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
size = int(sys.argv[2]) if len(sys.argv) > 2 else 512
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 2
FACES, OUT = 32, 256
dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
base = rng.integers(0, 256, (size // 8, size // 8, 3), dtype=np.uint8)
img = np.asarray(Image.fromarray(base).resize((size, size), Image.BICUBIC))
crops = np.stack([np.ascontiguousarray(np.roll(img, 7 * i, 1)[i:i + OUT, :OUT]) for i in range(FACES)])
masks = ((crops.astype(np.int32).sum(-1) > 384) * 255).astype(np.uint8)


def pillow_ms(batch):
    best, total = 1e9, 0
    for _ in range(3):
        t0 = time.perf_counter()
        total = 0
        for px in batch:
            buf = io.BytesIO()
            Image.fromarray(px).save(buf, format="PNG", compress_level=1)
            total += buf.tell()
        best = min(best, (time.perf_counter() - t0) / len(batch))
    return best * 1e3, total / len(batch)


def device_us(batch):
    px = torch.from_numpy(batch).to(dev)
    f, h, w = batch.shape[:3]
    c = batch.shape[3] if batch.ndim == 4 else 1
    out = torch.empty((f, h * (w * c + 1) + 1024), dtype=torch.uint8, device=dev)
    for _ in range(5):
        lengths = pngenc.encode_streams(px, out)
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            lengths = pngenc.encode_streams(px, out)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / 20 * 1e3)
    files = pngenc.encode_png(px)
    for file, want in zip(files, batch):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(file))), want)
    return min(times), max(times), float(lengths.float().mean()), float(np.mean([len(x) for x in files]))


for name, batch in (("crop 256x256x3", crops), ("mask 256x256", masks)):
    ms, host_bytes = pillow_ms(batch)
    lo, hi, stream, file = device_us(batch)
    raw = batch[0].size
    print(f"{name}: Pillow level 1 {ms:.3f} ms per face, file {host_bytes:.0f} B | device {lo:.1f}..{hi:.1f} us per call of {FACES} "
          f"faces ({lo / FACES:.2f} us per face), stream {stream:.0f} B per face read back against {raw} B raw, file {file:.0f} B")

with tempfile.TemporaryDirectory() as d:
    src = os.path.join(d, "in")
    os.makedirs(src)
    names = []
    for i in range(n):
        names.append(f"{i:05d}.jpg")
        Image.fromarray(np.roll(img, i, 1)).save(os.path.join(src, names[-1]), quality=90)
    tgt = landmarks_target((OUT, OUT), 0.65)
    table = np.stack([tgt * (size / OUT) * 0.8 + np.float32(size * 0.1) for _ in range(n)]).astype(np.float32)
    for rep in range(repeats):
        for enc in ("host", "device"):
            c = Cropper(output_size=OUT, landmarks=(table, np.array(names)), output_format="png", png_encoder=enc,
                        crop_source="original", batch_size=32, device="cuda:0")
            dst = os.path.join(d, f"out_{enc}_{rep}")
            if rep == 0:
                c.process_dir(src, dst + "_warm", desc=None)
            t0 = time.time()
            c.process_dir(src, dst, desc=None)
            dt = time.time() - t0
            total = sum(os.path.getsize(os.path.join(dst, x)) for x in os.listdir(dst))
            print(f"process_dir png_encoder={enc} run {rep}: {n} files {size}x{size} -> {len(os.listdir(dst))} crops {OUT}x{OUT}, "
                  f"{n / dt:.1f} images/s, {total / max(len(os.listdir(dst)), 1):.0f} B per file (io_threads={c.io_threads}, "
                  f"host cores {os.cpu_count()})")
