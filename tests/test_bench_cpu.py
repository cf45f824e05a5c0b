"""bench.py --dump-outputs: float32 files, the budget held by a fixed sample that is the same on every run."""
import numpy as np
import torch

import bench


def test_dump_outputs_float32_and_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    wav = torch.randn(8, 1, 300, generator=torch.Generator().manual_seed(0))
    loss = torch.tensor([0.25], dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"wav": wav, "loss": loss})
    a, b = np.load(tmp_path / "a" / "wav.npy"), np.load(tmp_path / "b" / "wav.npy")
    assert a.dtype == np.float32 and a.nbytes <= 2000 and np.array_equal(a, b)
    assert np.isin(a, wav.numpy().reshape(-1)).all()
    small = np.load(tmp_path / "a" / "loss.npy")
    assert small.dtype == np.float32 and small.tolist() == [0.25]
