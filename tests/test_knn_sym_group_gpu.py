"""
The group logs of the symmetric kNN sweep: delivered keys are gathered by the receiver's group of sixteen
rows - one atomic and one contiguous run of entries per group and batch - and pg_knn_sym_merge_kernel bins a group's log
by the receiver's place.  Inputs: tests/knn_sym_group_testdata.py, pinned without a GPU by tests/test_knn_sym_group_cpu.py.

Every entry of (indices, distances) against the C oracle AND byte for byte against the rectangular path (PG_KNN_SYM=0),
every call forced with PG_KNN_SYM=1 and held to the planner's "[pg plan sym] rows=N:" line (check / launch of
tests/test_knn_sym_edges_gpu.py).
"""
import numpy as np
import pytest
import torch

import knn_sym_testdata as D
import knn_sym_group_testdata as G
from test_knn_sym_edges_gpu import FAR, check, launch, oracle
from test_knn_sym_gpu import case as clustered_case


@pytest.mark.gpu
@pytest.mark.parametrize("n", G.SEAM_NS)
def test_group_block_and_super_tile_seams(monkeypatch, capfd, n):
    """clusters whose members sit on either side of rows 16, 32, 64, 128, and a last group of 1, 8 and 9 rows"""
    tok, _ = G.seam_case(n)
    check(monkeypatch, capfd, tok, oracle(tok, G.SEAM_KS), (FAR, {}))


@pytest.mark.gpu
@pytest.mark.parametrize("over", [False, True], ids=["exactly_full", "one_over"])
def test_log_capacity(monkeypatch, capfd, over):
    """PG_KNN_SYM_CAPL=8: a group that receives exactly 128 entries, 8 a row (all kept, k = 8 needs every one), and one that
    receives 129 (the whole group is evicted and recomputed); the evict limit out of reach and at its default"""
    tok = G.full_case(over)
    capl = {"PG_KNN_SYM_CAPL": str(G.FULL_CAPL)}
    check(monkeypatch, capfd, tok, oracle(tok, G.FULL_KS), ({**capl, **FAR}, capl))


@pytest.mark.gpu
def test_a_batch_in_64_groups(monkeypatch, capfd):
    """the grouping loop at its full length: every delivered key of pass 0 has a group of its own, every run is one entry"""
    tok, _ = G.spread_case()
    check(monkeypatch, capfd, tok, oracle(tok, G.SPREAD_KS), (FAR, {}))


@pytest.mark.gpu
def test_a_batch_in_one_group(monkeypatch, capfd):
    """runs of up to 64 entries into one log, two passes and the group's own rows appending to one counter"""
    tok = G.dense_case()
    check(monkeypatch, capfd, tok, oracle(tok, G.DENSE_KS), (FAR, {}))


@pytest.mark.gpu
def test_direct_form_delivers_from_the_epilogue(monkeypatch, capfd):
    """L = 5: every pair is below the cap, the dense form computes every distance and delivers in place"""
    tok = D.width_case(G.DIRECT_N, G.DIRECT_L)
    check(monkeypatch, capfd, tok, oracle(tok, G.DIRECT_KS), (FAR, {}))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "interleaved"])
def test_entries_with_seven_distance_bits(monkeypatch, capfd, order):
    """PG_KNN_GUESS=65: distances up to 64 travel in 7 bits above a 21-bit row; low groups keep their logs, high ones overflow"""
    tok, _ = G.wide_case(order)
    guess = {"PG_KNN_GUESS": G.WIDE_GUESS}
    check(monkeypatch, capfd, tok, oracle(tok, G.WIDE_KS), ({**guess, **FAR}, guess))


@pytest.mark.gpu
def test_three_forced_runs_are_byte_identical(monkeypatch, capfd):
    """the arrival order within a log is arbitrary; the result does not depend on it"""
    from prograph_amd import _native as nat
    tok, ref = clustered_case(3000, "contiguous")
    planes = nat.pack(torch.from_numpy(tok), bits=5)
    runs = [launch(monkeypatch, capfd, planes, planes, 16, "1", FAR) for _ in range(3)]
    assert all(took for _, _, took in runs)
    for idx, dist, _ in runs:
        assert idx.tobytes() == runs[0][0].tobytes() and dist.tobytes() == runs[0][1].tobytes()
    assert np.array_equal(runs[0][0], ref[16][0]) and np.array_equal(runs[0][1], ref[16][1])
