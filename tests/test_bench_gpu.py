"""GPU: `bench.py --dump-outputs` writes what its timed path computed — the arrays the product's own calls return for the
benchmark's seeded batch — and the result line reports the timed steps it was asked for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_RECORDS = ("roofline", "hbm_kernels", "cpu_baseline", "parity_check", "extra")


@pytest.mark.parametrize("workload", ["detect", "full"])
def test_dumped_outputs_are_what_the_timed_path_returns(workload, tmp_path, device):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
           "--size", "256", "--workload", workload, "--enhance", "none", "--no-extra", "--no-cpu-baseline", "--no-telemetry",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([s for s in r.stdout.splitlines() if s.startswith('{"metric"')][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["dumped_outputs"]["dir"] == str(out)
    assert not set(line) & set(SIDE_RECORDS)                     # a plain run measures the headline only

    # the same seeded batch and weights through the same pipeline, in this process
    sys.path.insert(0, ROOT)
    import bench
    from face_crop_plus_amd import weights
    full = workload == "full"
    p = bench.Pipeline(device, weights.generate_state_dict("retinaface"), full=full, batch=4, size=256, out_size=256,
                       strategy="largest", precision="f16x3", enhance="none", streams=2, seed=1234,
                       sd_par=weights.generate_state_dict("bisenet") if full else None)
    p.step(False)
    torch.cuda.synchronize()
    want = bench.step_outputs(p)
    del p
    assert int(want["face_offset"][-1]) == 4                    # the CPU oracle finds one face in each of these 4 images
    assert set(line["dumped_outputs"]["arrays"]) == set(want) and {f.name for f in out.iterdir()} == {k + ".npy" for k in want}
    assert ("labels" in want) == full
    total = 0
    for k, v in want.items():
        got = np.load(out / (k + ".npy"))
        total += (out / (k + ".npy")).stat().st_size
        assert got.dtype == (np.float32 if v.dtype in (np.uint8, np.float32) else np.float64), k
        assert np.array_equal(got, v.astype(got.dtype)), k
    assert total <= bench.DUMP_LIMIT_BYTES


def test_full_adds_the_side_records_after_the_same_timed_steps(tmp_path):
    """`--full` keeps the headline fields and adds the roofline (with its per-launch table), the HBM kernel records and the
    CPU baseline with the oracle's parity check of the timed batch (`extra` is left out here: its workloads are full-size)."""
    table = tmp_path / "launches.csv"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
           "--size", "256", "--full", "--no-extra", "--cpu-seconds", "1", "--launch-table", str(table)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([s for s in r.stdout.splitlines() if s.startswith('{"metric"')][-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert set(line) >= set(SIDE_RECORDS) - {"extra"} and "extra" not in line
    assert line["roofline"]["launches_per_step"] > 0 and line["roofline"]["achieved"] > 0
    assert "warp_affine_kernel<4>" in line["hbm_kernels"]
    assert line["cpu_baseline"]["value"] > 0
    pc = line["parity_check"]
    assert pc["indices_equal"] and pc["faces"] > 0 and pc["crop_bytes_differing"] == 0 and not pc["vacuous"]
    rows = table.read_text().splitlines()
    assert rows[0].startswith("launch,us,") and len(rows) == 1 + line["roofline"]["launches_per_step"]
