"""CPU: bench.py's command line (plain run by default, --full, --dump-outputs) and the output dump's format and budget."""
import os
import sys

import numpy as np
import torch


def test_plain_run_is_the_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert (a.steps, a.full, a.dump_outputs) == (100, True, "out")


def test_dump_outputs_float32_and_fixed_sample(monkeypatch, tmp_path):
    import bench
    monkeypatch.setattr(bench, "DUMP_ARRAY_MAX_ELEMS", 1000)
    monkeypatch.setattr(bench, "DUMP_TOTAL_MAX_BYTES", 6000)
    small = torch.arange(12, dtype=torch.float64).view(3, 4)
    big = np.random.RandomState(5).standard_normal(5000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big, "scalars": np.ones((16, 9), np.float32)})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "scalars.npy", "small.npy"]
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.numpy().astype(np.float32))
    b1, b2 = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert b1.dtype == np.float32 and np.array_equal(b1, b2)
    # the smaller arrays are written whole first; the big one gets what is left of the budget, sampled from its own values
    assert b1.size == min(1000, (6000 - 4 * (12 + 144)) // 4)
    assert np.isin(b1, big.astype(np.float32)).all()
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 6000 + 3 * 128      # + the .npy headers
