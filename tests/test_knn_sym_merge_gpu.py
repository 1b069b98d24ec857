"""
The merge of the symmetric kNN sweep (pg_knn_sym_merge_kernel) where its rebuilt form can go wrong: the head
of a row's slot is loaded before the row's count is known and masked afterwards; the delivered keys stay in registers,
sixteen a lane, sorted by each lane and merged from the lanes' heads together with the heads of the own lists; the records
of a block's passes are PG_MM_KL keys of which the last k + 1 count; and the decision behind the merge is taken by the
workgroup that draws the last ticket, workgroups and waves without rows included.

Forced with PG_KNN_SYM=1, PG_ENGINE=mfma, PG_MM_R=2; every forced call is held to the planner's "[pg plan sym] rows=N:"
line and compared entry by entry with the C oracle and byte for byte with the rectangular path (PG_KNN_SYM=0).  Inputs:
tests/knn_sym_testdata.py and the generator's clusters (test_knn_sym_gpu.case: one oracle per shape, shared).
"""
import numpy as np
import pytest
import torch

import knn_sym_testdata as D
from test_knn_sym_edges_gpu import FAR, check, launch, oracle
from test_knn_sym_gpu import case as clustered_case

KS = (1, 16, 19)                                             # k = 19: k + 1 = PG_MM_KL, a record has no leading entries


@pytest.mark.gpu
def test_slots_of_eight_masked_behind_the_count(monkeypatch, capfd):
    """24 identical rows at ascending indices, slots of 8: member j holds min(j, 8) keys of a slot whose first 8 entries are
    loaded whatever j is - 0, 1, 7 (capL - 1), 8 (capL), 9 (capL + 1: evicted), 15, 16, 17 delivered keys"""
    tok, rows, _ = D.duplicates(D.SLOT8_N, 24, 1)
    got = D.delivered(tok, D.CAPS[64])[rows]
    assert got.tolist() == list(range(24))
    check(monkeypatch, capfd, tok, oracle(tok, KS), ({"PG_KNN_SYM_CAPL": "8", **FAR}, {"PG_KNN_SYM_CAPL": "8"}))


@pytest.mark.gpu
def test_the_production_slot_masked_behind_the_count(monkeypatch, capfd):
    """300 identical rows, slots of 256: rows that receive 0, 1, 15, 16 (one key a lane: nothing to sort), 17 (the first lane
    with two), 63, 64, 65, 255, 256 (every register of every lane) and 257 keys (evicted); all keys tie on distance 0"""
    tok, rows, _ = D.duplicates(D.SLOT256_N, D.SLOT256_SIZE, 1, start=D.SLOT256_START)
    got = D.delivered(tok, D.CAPS[64])[rows]
    assert set((0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257)) <= set(got.tolist())
    check(monkeypatch, capfd, tok, oracle(tok, KS), (FAR, {}))


@pytest.mark.gpu
@pytest.mark.parametrize("outer", [FAR, {}], ids=["outer_merge", "outer_default"])
@pytest.mark.parametrize("middle", [{}, {"PG_KNN_SYM_EVICT_LIMIT": "0"}, FAR], ids=["default", "fallback", "out_of_reach"])
def test_three_calls_on_one_workspace(monkeypatch, capfd, middle, outer):
    """one N, so one cached workspace: 300 identical rows (slots overflow, rows evicted), strided clusters, the first again.
    A ticket, a count of evicted rows or counts of delivered keys left by the call before show as a wrong result.  The 700
    unrelated rows of the first input are evicted too: with the limit out of reach (outer_merge) the first and the third
    call keep the merge's own output, with the default limit they hand over to the rectangular launch and reset the count."""
    from prograph_amd import _native as nat
    a, _, _ = D.duplicates(D.SLOT256_N, D.SLOT256_SIZE, 1, start=D.SLOT256_START)
    b, bref = clustered_case(D.SLOT256_N, "strided64")
    assert a.shape == b.shape
    aref = oracle(a, (16,))
    pa, pb = nat.pack(torch.from_numpy(a), bits=5), nat.pack(torch.from_numpy(b), bits=5)
    rect = [launch(monkeypatch, capfd, p, p, 16, "0", {}) for p in (pa, pb)]
    assert not rect[0][2] and not rect[1][2]
    runs = [launch(monkeypatch, capfd, p, p, 16, "1", env) for p, env in ((pa, outer), (pb, middle), (pa, outer))]
    for (idx, dist, took), (ridx, rdist, _), (oidx, odist), name in zip(runs, (rect[0], rect[1], rect[0]), (aref[16], bref[16], aref[16]),
                                                                         ("first", "middle", "third")):
        assert took, (name, "the forced call did not take the symmetric path")
        assert np.array_equal(idx, oidx) and np.array_equal(dist, odist), (name, "oracle")
        assert idx.tobytes() == ridx.tobytes() and dist.tobytes() == rdist.tobytes(), (name, "rectangular path")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 20, 63, 65, 129, 193])
def test_ticket_with_idle_waves(monkeypatch, capfd, n):
    """the merge's last workgroup has waves without rows (16 rows a workgroup): they take no part and the workgroup still
    draws its ticket; limit out of reach and the default one"""
    tok = D.tiny_case(n, 64)
    check(monkeypatch, capfd, tok, oracle(tok, KS), (FAR, {}))


@pytest.mark.gpu
def test_ticket_when_every_row_is_evicted(monkeypatch, capfd):
    """clusters of 12 (< k + 1): every row loses the cap, the last workgroup finds more than N / 16 evicted rows and hands
    the launch to the rectangular sweep"""
    tok, ref = clustered_case(1000, "strided12")
    check(monkeypatch, capfd, tok, {16: ref[16], 19: ref[19]}, ({},))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3000, "strided256"), (D.PIECES_16[0], "contiguous")], ids=["seven_pieces", "sixteen_pieces"])
def test_records_across_pieces(monkeypatch, capfd, shape):
    """pieces of 3 super-tiles: seven records a row at N = 3000, sixteen - one per lane of the row's group - in block 0 of
    N = 6017; the last k + 1 keys of each record"""
    n, kind = shape
    assert n == 3000 or D.pieces_asked(n, 3) == 16
    tok, ref = clustered_case(n, kind)
    check(monkeypatch, capfd, tok, {k: ref[k] for k in KS}, ({"PG_KNN_SYM_PIECE": "3"},))


@pytest.mark.gpu
@pytest.mark.parametrize("wgs", ["1", "3"])
@pytest.mark.parametrize("n", [193, 1000])
def test_workgroups_take_rows_in_turns(monkeypatch, capfd, n, wgs):
    """the production grid is eight workgroups a CU, every wave takes four rows after four rows: one and three workgroups
    for 13 and 63 workgroups' rows - waves that go round a different number of times, the staged records overwritten, one
    ticket a workgroup; clusters of 64 (limit out of reach) and of 12 (every row evicted, the fallback decided)"""
    for kind, env in (("strided64", FAR), ("strided12", {})):
        tok, ref = clustered_case(n, kind)
        check(monkeypatch, capfd, tok, {16: ref[16], 19: ref[19]}, ({"PG_KNN_SYM_MERGE_WGS": wgs, **env},))
