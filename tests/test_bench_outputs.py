"""bench.py --dump-outputs (no GPU): the files it writes, and the fixed sample of an output beyond
the byte limit."""
import os

import numpy as np

import bench


def test_dump_outputs_whole_arrays_as_float32(tmp_path):
    a = np.arange(12, dtype=np.float64).reshape(3, 4)
    bench.dump_outputs(str(tmp_path / "d"), {"predictions": a, "params": np.ones(5, np.float32)})
    assert sorted(os.listdir(tmp_path / "d")) == ["params.npy", "predictions.npy"]
    got = np.load(tmp_path / "d" / "predictions.npy")
    assert got.dtype == np.float32 and got.shape == (3, 4) and np.array_equal(got, a)
    bench.dump_outputs(str(tmp_path / "d2"), {"predictions": a}, rank=1, world=2)
    assert os.listdir(tmp_path / "d2") == ["predictions_rank1.npy"]


def test_dump_outputs_samples_beyond_the_limit_the_same_way_every_time(tmp_path):
    rng = np.random.default_rng(0)
    arrays = {"a": rng.standard_normal((1000, 3)).astype(np.float32), "b": rng.standard_normal(500).astype(np.float32)}
    limit = 4000   # bytes, against 14000 of output
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=limit)
    total = 0
    for name, src in arrays.items():
        x, y = np.load(tmp_path / "x" / (name + ".npy")), np.load(tmp_path / "y" / (name + ".npy"))
        assert np.array_equal(x, y) and x.dtype == np.float32 and 0 < x.size < src.size
        # elements of the source, in their order
        flat = src.reshape(-1)
        pos = np.searchsorted(np.sort(flat), x)
        assert np.array_equal(np.sort(flat)[pos], x)
        order = np.argsort(flat, kind="stable")[pos]
        assert np.all(np.diff(order) > 0)
        total += x.nbytes
    assert total <= limit
