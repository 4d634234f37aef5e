"""bench.py --dump-outputs, host side: dtypes, the size budget and the seeded sample that keeps a large output inside it."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_outputs_are_float_and_small_ones_are_kept_whole(tmp_path):
    arrays = {"x": torch.arange(12, dtype=torch.float32).view(3, 4), "counts": torch.tensor([3, 1, 0, 4], dtype=torch.int32),
              "d": torch.ones(5, dtype=torch.float64)}
    s = bench.write_outputs(str(tmp_path), arrays)
    assert s["arrays"] == 3 and s["sampled"] == [] and sorted(os.listdir(str(tmp_path))) == ["counts.npy", "d.npy", "x.npy"]
    x, c, d = (np.load(str(tmp_path / n)) for n in ("x.npy", "counts.npy", "d.npy"))
    assert x.dtype == np.float32 and x.shape == (3, 4) and np.array_equal(x, np.arange(12).reshape(3, 4))
    assert c.dtype == np.float64 and c.tolist() == [3, 1, 0, 4] and d.dtype == np.float64
    assert s["bytes"] == x.nbytes + c.nbytes + d.nbytes


def test_a_set_over_the_budget_is_cut_by_a_fixed_seeded_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    big = torch.arange(1 << 19, dtype=torch.float32)            # 2 MB, alone over the 1 MB budget
    arrays = {"big": big, "mid": torch.ones(1 << 16), "small": torch.zeros(10)}
    s1 = bench.write_outputs(str(tmp_path / "a"), arrays)
    s2 = bench.write_outputs(str(tmp_path / "b"), arrays)
    assert s1["sampled"] == ["big"] and s1["bytes"] <= 1 << 20 and s1 == dict(s2, dir=s1["dir"])
    a, b = np.load(str(tmp_path / "a" / "big.npy")), np.load(str(tmp_path / "b" / "big.npy"))
    assert np.array_equal(a, b) and a.ndim == 1 and 0 < a.size < big.numel()
    assert (np.diff(a) > 0).all() and np.isin(a, big.numpy()).all()          # distinct elements, in their original order
    assert np.load(str(tmp_path / "a" / "mid.npy")).size == 1 << 16 and np.load(str(tmp_path / "a" / "small.npy")).size == 10
