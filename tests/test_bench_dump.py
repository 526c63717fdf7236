"""bench.py --dump-outputs on the CPU: what it writes, in which precision, and the size cap with its fixed sample."""
import os

import numpy as np
import torch

import bench


def test_dump_writes_every_array_whole_when_it_fits(tmp_path):
    a = torch.randn(2560, 2)
    b = torch.randn(3, 4, dtype=torch.float64)
    c = torch.arange(10, dtype=torch.int32)
    info = bench._dump_outputs(str(tmp_path), {"a": a, "b": b, "c": c})
    assert np.array_equal(np.load(tmp_path / "a.npy"), a.numpy())
    assert np.load(tmp_path / "b.npy").dtype == np.float64 and np.array_equal(np.load(tmp_path / "b.npy"), b.numpy())
    assert np.load(tmp_path / "c.npy").dtype == np.float32 and np.array_equal(np.load(tmp_path / "c.npy"), np.arange(10))
    assert all(v["sample"] is None for v in info.values())


def test_dump_over_the_limit_keeps_the_same_sample(tmp_path):
    big = torch.randn(300_000)
    small = torch.randn(1000)
    limit = 600_000
    first = bench._dump_outputs(str(tmp_path / "1"), {"big": big, "small": small}, limit=limit)
    bench._dump_outputs(str(tmp_path / "2"), {"big": big, "small": small}, limit=limit)
    total = sum(os.path.getsize(tmp_path / "1" / f"{n}.npy") for n in ("big", "small"))
    assert total <= limit
    assert first["big"]["sample"] is not None and first["big"]["elements"] < big.numel()
    for n in ("big", "small"):
        x = np.load(tmp_path / "1" / f"{n}.npy")
        assert np.array_equal(x, np.load(tmp_path / "2" / f"{n}.npy"))
        assert np.isin(x, (big if n == "big" else small).numpy()).all()
