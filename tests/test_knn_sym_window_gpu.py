"""
The merge of the symmetric kNN sweep (pg_knn_sym_merge_kernel) with its rounds on a WINDOW of a lane's
delivered keys: four registers move at a win, a lane that won four times takes the next four in a cold branch (the refill),
and the next trip's header - the block's passes and the group's count - is read a trip ahead.  PG_KNN_SYM_MERGE_WINDOW=1 / 2
select the narrow instances, where every second / third win of a lane refills: the cold path runs on ordinary inputs.
Every case runs with the knob unset (four), 1 and 2; k over (1, 16, 19).

Forced with PG_KNN_SYM=1, PG_ENGINE=mfma, PG_MM_R=2; every forced call is held to the planner's "[pg plan sym] rows=N:"
line and compared entry by entry with the C oracle and byte for byte with the rectangular path (PG_KNN_SYM=0).  Inputs:
tests/knn_sym_testdata.py and the generator's clusters (test_knn_sym_gpu.case: one oracle per shape, shared).  Which lane
holds which delivered key is the arrival order's: tests/test_knn_sym_window_cpu.py has the distributions pinned.
"""
import numpy as np
import pytest
import torch

import knn_sym_testdata as D
from test_knn_sym_edges_gpu import FAR, check, launch, oracle
from test_knn_sym_gpu import case as clustered_case

KS = (1, 16, 19)
WINDOWS = ({}, {"PG_KNN_SYM_MERGE_WINDOW": "1"}, {"PG_KNN_SYM_MERGE_WINDOW": "2"})


def windows(*envs):
    """every env at every window width"""
    return tuple({**w, **env} for env in envs for w in WINDOWS)


@pytest.mark.gpu
def test_rows_of_0_to_257_tied_delivered_keys(monkeypatch, capfd):
    """300 identical rows: row j receives j keys, all at distance 0, up to 257 (evicted).  A row with 17 or more delivered
    winners has a lane that wins twice (sixteen lanes): a window of one must refill, rows of 256 keys refill at every width"""
    tok, rows, _ = D.duplicates(D.SLOT256_N, D.SLOT256_SIZE, 1, start=D.SLOT256_START)
    got = D.delivered(tok, D.CAPS[64])[rows]
    assert set((0, 1, 16, 17, 64, 65, 256, 257)) <= set(got.tolist())
    check(monkeypatch, capfd, tok, oracle(tok, KS), windows(FAR, {}))


@pytest.mark.gpu
def test_slots_of_eight(monkeypatch, capfd):
    """24 identical rows, slots of 8: at most one delivered key a lane, the window's first place alone is ever used"""
    tok, _, _ = D.duplicates(D.SLOT8_N, 24, 1)
    check(monkeypatch, capfd, tok, oracle(tok, KS), windows({"PG_KNN_SYM_CAPL": "8", **FAR}, {"PG_KNN_SYM_CAPL": "8"}))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 20, 65, 193])
def test_tiny_graphs(monkeypatch, capfd, n):
    """fewer keys than k + 1 ("no entry" wins and moves nothing), waves and lanes without rows, one trip and one header"""
    tok = D.tiny_case(n, 64)
    check(monkeypatch, capfd, tok, oracle(tok, KS), windows(FAR, {}))


@pytest.mark.gpu
def test_seven_records_a_row(monkeypatch, capfd):
    """pieces of 3 super-tiles at N = 3000: seven own lists beside the delivered keys, winners of both kinds in turns"""
    tok, ref = clustered_case(3000, "strided256")
    check(monkeypatch, capfd, tok, {k: ref[k] for k in KS}, windows({"PG_KNN_SYM_PIECE": "3"}))


@pytest.mark.gpu
def test_many_trips_a_workgroup(monkeypatch, capfd):
    """one workgroup makes all 63 trips of N = 1000: the header read ahead is used and overwritten trip after trip"""
    tok, ref = clustered_case(1000, "strided64")
    check(monkeypatch, capfd, tok, {k: ref[k] for k in KS}, windows({"PG_KNN_SYM_MERGE_WGS": "1", **FAR}))


@pytest.mark.gpu
def test_every_row_evicted(monkeypatch, capfd):
    """clusters of 12: every row loses the cap and the rectangular launch takes over; every workgroup's trip is its last -
    it asks for no header behind the workspace's regions"""
    tok, ref = clustered_case(1000, "strided12")
    check(monkeypatch, capfd, tok, {k: ref[k] for k in KS}, windows({}))


@pytest.mark.gpu
def test_three_runs_are_byte_identical(monkeypatch, capfd):
    """delivery goes through atomics in arbitrary order: which lane's window holds a key changes, the result does not"""
    from prograph_amd import _native as nat
    tok, ref = clustered_case(3000, "contiguous")
    planes = nat.pack(torch.from_numpy(tok), bits=5)
    for w in WINDOWS:
        runs = [launch(monkeypatch, capfd, planes, planes, 19, "1", {**w, **FAR}) for _ in range(3)]
        assert all(took for _, _, took in runs), w
        for idx, dist, _ in runs:
            assert idx.tobytes() == runs[0][0].tobytes() and dist.tobytes() == runs[0][1].tobytes(), w
        assert np.array_equal(runs[0][0], ref[19][0]) and np.array_equal(runs[0][1], ref[19][1]), w
