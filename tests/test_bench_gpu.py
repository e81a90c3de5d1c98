"""A plain `bench.py` run on the GPU: the headline line only, and --dump-outputs writes the timed path's last outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_outputs(dev, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--spinup-ms", "0",
                        "--num-rays", "256", "--num-rays-lidar", "128", "--num-steps", "64", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["outputs_finite"] is True and d["unit"] == "rays/s" and d["dtype"] == "f16"
    assert abs(d["value"] - 384 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    for leg in ("roofline", "kernels", "cpu_baseline", "outputs_match_oracle", "train", "eval", "occupancy", "fresh_batches", "detail"):
        assert leg not in d, leg  # --full only
    depth = np.load(tmp_path / "lidar_depth.npy")
    image = np.load(tmp_path / "camera_image.npy")
    weights = np.load(tmp_path / "camera_weights.npy")
    assert depth.shape == (128,) and image.shape == (256, 3) and weights.shape == (256, 64)
    assert depth.dtype == image.dtype == weights.dtype == np.float32 and np.isfinite(image).all()
