"""bench.py's --full / --dump-outputs plumbing (CPU only, no kernel runs):
the options parse with --full off by default, and dump_outputs writes the
reduce value and the scanned segment (whole when small, a fixed sample that
keeps the final element when large) as float32 / float64 .npy files that are
the same from call to call."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_full_and_dump_options(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_small_and_sampled(tmp_path, monkeypatch):
    import torch
    out = torch.cumsum(torch.arange(1000, dtype=torch.float32), 0)
    red = torch.tensor([out[-1].item()], dtype=torch.float64)
    unused = torch.zeros(1, dtype=torch.float64)
    bench.dump_outputs(torch, np, str(tmp_path / "a"), 0, 1, out, red, unused)
    s = np.load(tmp_path / "a" / "inclusive_scan.npy")
    r = np.load(tmp_path / "a" / "reduce.npy")
    assert s.dtype == np.float32 and np.array_equal(s, out.numpy())
    assert r.dtype == np.float64 and r.shape == (1,) and r[0] == out[-1].item()

    # a segment larger than the sample: DUMP_SAMPLE fixed positions, the last one the final element
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 64)
    for d in ("b", "c"):
        bench.dump_outputs(torch, np, str(tmp_path / d), 0, 1, out, red, unused)
    b, c = (np.load(tmp_path / d / "inclusive_scan.npy") for d in ("b", "c"))
    assert b.shape == (64,) and np.array_equal(b, c)
    assert b[-1] == out[-1].item() and np.all(np.diff(b) >= 0) and np.all(np.isin(b, out.numpy()))

    # int32 outputs are written as float64 (exact); N > 1 writes the folded result, per-rank names
    oi = torch.arange(100, dtype=torch.int32)
    bench.dump_outputs(torch, np, str(tmp_path / "i"), 1, 2, oi, torch.tensor([7], dtype=torch.int32),
                       torch.tensor([11], dtype=torch.int32))
    si = np.load(tmp_path / "i" / "inclusive_scan.rank1.npy")
    assert si.dtype == np.float64 and si.shape == (64,) and si[-1] == 99.0 and np.array_equal(si, np.round(si))
    assert np.load(tmp_path / "i" / "reduce.rank1.npy")[0] == 11.0
