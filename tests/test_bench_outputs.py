"""bench.py --dump-outputs without a GPU: the conversion to float32 / float64 and the 64 MB budget."""
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_small_arrays_are_written_whole(tmp_path):
    b = _bench()
    idx = np.arange(12, dtype=np.int32).reshape(3, 4) * 100_003
    dist = np.arange(12, dtype=np.uint8).reshape(3, 4)
    b.dump_outputs(str(tmp_path), {"knn_indices": idx, "knn_distances": dist}, suffix="_rank1")
    gi, gd = np.load(tmp_path / "knn_indices_rank1.npy"), np.load(tmp_path / "knn_distances_rank1.npy")
    assert gi.dtype == np.float64 and gd.dtype == np.float32
    assert np.array_equal(gi, idx) and np.array_equal(gd, dist)


def test_dump_outputs_over_budget_is_a_fixed_sample(tmp_path):
    b = _bench()
    n = 6_000_000                                   # 48 MB as float64 + 24 MB as float32: over the budget
    arrays = {"indices": np.arange(n, dtype=np.int32), "weights": (np.arange(n) % 251).astype(np.uint8)}
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), arrays)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 10 ** 6
    for name in arrays:
        a, c = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert np.array_equal(a, c) and 0 < a.size < n
    pos = np.load(tmp_path / "a" / "indices.npy").astype(np.int64)      # the sample of arange is its positions
    assert np.all(np.diff(pos) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "weights.npy"), (pos % 251).astype(np.float32))
