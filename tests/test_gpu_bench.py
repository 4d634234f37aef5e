"""bench.py's plain run (no --full): the headline figure and nothing else, and --dump-outputs with what the last timed step computed.
Two runs with the same arguments must see the same inputs (noise, dropout masks drawn on the device from fixed seeds)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16",
           "--dump-outputs", out_dir]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(out_dir, "*.npy"))}
    return json.loads(lines[0]), arrays


def test_plain_bench_run_is_lean_and_dumps_the_last_step(tmp_path):
    j, a = _plain_run(str(tmp_path / "a"))
    assert j["metric"] == "GAN train images/sec (G+D step) at 32x32x3 bs128" and j["unit"] == "images/sec"
    assert j["higher_is_better"] is True and j["dtype"] == "f32" and j["steps"] == 3 and j["warmup"] == 1
    assert j["value"] > 0 and j["ms_per_step"] > 0 and abs(j["value"] - 16 * 1000.0 / j["ms_per_step"]) < 1e-6 * j["value"]
    for moved in ("roofline", "step_roofline", "c2f", "cpu_baseline", "alt_math", "host_input_images_per_sec", "host_enqueue_ms_per_step"):
        assert moved not in j, "a plain run measured %s (that belongs behind --full)" % moved
    assert j["dumped_outputs"]["arrays"] == len(a) and j["dumped_outputs"]["sampled"] == []
    for name in ("D_loss", "D_outputs", "D_confusion", "D_noise", "G_loss", "G_outputs", "G_samples", "G_noise", "params_G", "params_D"):
        assert name in a, sorted(a)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["G_samples"].shape == (16, 32, 32, 3) and a["D_outputs"].shape == (16, 1) and a["D_noise"].shape == (8 * 100,)
    assert a["params_D"].size == 2863239                                   # D's flat vector, models.lua:382-416
    assert a["D_confusion"].dtype == np.float64 and (a["D_confusion"] == np.round(a["D_confusion"])).all()    # int32 counts, exact
    assert all(np.isfinite(v).all() for v in a.values())
    assert ((a["G_samples"] >= 0) & (a["G_samples"] <= 1)).all()           # G ends in a Sigmoid (models.lua:57-81)
    # the same arguments again: the same inputs, and the same step up to rounding
    j2, b = _plain_run(str(tmp_path / "b"))
    assert sorted(a) == sorted(b)
    for name in a:
        assert a[name].shape == b[name].shape, name
        if name.endswith("_noise") or "_masks" in name:
            assert np.array_equal(a[name], b[name]), name
    assert abs(a["D_loss"][0] - b["D_loss"][0]) <= 1e-4 * abs(a["D_loss"][0])
