"""CPU: what bench.py --dump-outputs writes - the groups in key order as float64, and beyond its size limit the same seeded
sample of groups whatever order the groupby returned them in."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_in_key_order(tmp_path):
    g = torch.Generator().manual_seed(0)
    keys = torch.randperm(1000, generator=g)
    sums = torch.rand(1000, generator=g, dtype=torch.float64)
    counts = torch.randint(0, 50, (1000,), generator=g, dtype=torch.int32)
    assert bench.dump_outputs(str(tmp_path), keys, {"sum": sums, "count_valid": counts}) == (1000, 1000)
    order = torch.argsort(keys).numpy()
    for name, col in (("keys", keys), ("sum", sums), ("count_valid", counts)):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64
        assert np.array_equal(got, col.numpy()[order].astype(np.float64))


def test_dump_outputs_samples_the_same_groups_beyond_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 2 * 8 * 100)  # room for 100 rows of keys + one column
    g = torch.Generator().manual_seed(1)
    keys = torch.randperm(1000, generator=g)
    shuffle = torch.randperm(1000, generator=g)
    assert bench.dump_outputs(str(tmp_path / "a"), keys, {"v": keys * 0.5}) == (1000, 100)
    assert bench.dump_outputs(str(tmp_path / "b"), keys[shuffle], {"v": keys[shuffle] * 0.5}) == (1000, 100)
    ka, kb = np.load(tmp_path / "a" / "keys.npy"), np.load(tmp_path / "b" / "keys.npy")
    assert np.array_equal(ka, kb) and np.all(np.diff(ka) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "v.npy"), ka * 0.5)  # the columns stay aligned with the keys
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= bench.DUMP_LIMIT_BYTES
