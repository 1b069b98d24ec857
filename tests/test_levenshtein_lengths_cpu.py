"""
Set B of the Levenshtein tests (tests/lev_testdata.py) without a GPU: the two references - the C oracle and the numpy
Wagner-Fischer table - agree on every pair, the oracle's banded distance and kNN lists are what the full matrix says,
and the set holds what tests/test_levenshtein_lengths_gpu.py needs to mean something: distances on both sides of every
band, in-band pairs across every dword boundary of the 128-bit pattern, in-band pairs shorter than the band, ties, and
epsilon graphs that are neither empty nor full.  Everything here is asserted from the references alone.
"""
import numpy as np
import pytest

import lev_testdata as LT
from oracle import c_oracle as C

BANDS = range(1, 9)


@pytest.fixture(scope="module")
def B():
    return LT.set_b()


@pytest.fixture(scope="module")
def D():
    return LT.set_b_matrix()


def test_layout_and_families(B, D):
    n = len(B)
    assert B.shape == (LT.B_BLOCKS * len(LT.LENS), 128) == (441, 128) and B.dtype == np.uint8
    lens = LT.lengths(B)
    assert np.array_equal(lens, [LT.LENS[r % len(LT.LENS)] for r in range(n)])
    assert np.array_equal((B != 0).sum(1), lens)                         # zeros are trailing padding only
    assert B.max() == 31 and {16, 31} <= set(np.unique(B)) and set(np.unique(B)) == set(range(32))
    assert np.array_equal(B, LT.set_b()) and LT.set_b() is B              # deterministic
    fam = np.array([LT.set_b_layout(r)[1] for r in range(n)])
    for f in LT.FAMILIES:                                                # every family at every length, interleaved
        assert sorted(lens[fam == f]) == sorted(LT.LENS * 3)
    assert all(len(set(fam[r:r + 7])) == 7 for r in range(n) if r % 21 <= 14)     # within a block of 21 rows
    homo = {(int(lens[r]), int(B[r, 0])) for r in np.nonzero(fam == "homopolymer")[0] if lens[r]}
    assert {(l, 31) for l in LT.LENS if l} <= homo and (128, 16) in homo
    h128, h127 = (next(r for r in range(n) if fam[r] == "homopolymer" and lens[r] == l and B[r, 0] == 31) for l in (128, 127))
    assert (B[h128] == 31).all() and D[h128, h127] == 1                  # the canonical carry chain
    for f in ("period2", "period3"):                                     # x = y[1:] occurs, on both sides of a boundary
        rows = np.nonzero(fam == f)[0]
        shifted = {(int(lens[y]), int(lens[x])) for y in rows for x in rows
                   if lens[y] == lens[x] + 1 and np.array_equal(B[y, 1:lens[y]], B[x, :lens[x]])}
        assert {(33, 32), (65, 64), (97, 96), (128, 127)} <= shifted, (f, shifted)
    rng = np.random.default_rng(0)
    parent = B[next(r for r in range(n) if fam[r] == "parent_piece" and lens[r] == 128)].astype(np.int64)
    for L in LT.LENS:
        for v in range(3):
            row, p, at = LT._mutant(rng, parent, L, v)
            assert len(row) == L and 1 <= min(row, default=1) and max(row, default=1) <= 31
            if L >= 30:
                assert p in LT.MUTANT_PARENTS and 1 <= len(at) <= 9 and at[0] in LT.EDGES
                assert 1 <= C.lev_pair(np.array(row + [0] * (128 - L)), np.pad(parent[:p], (0, 128 - p)), 128) <= len(at)
    for r in np.nonzero((fam == "mutant") & (lens >= 30))[0]:            # and the set's own mutants are near a parent piece
        assert 1 <= D[r][(fam == "parent_piece") & np.isin(lens, LT.MUTANT_PARENTS)].min() <= 9
    off = ~np.eye(n, dtype=bool)
    assert ((D == 0) & off & (lens[:, None] > 0)).any()                  # exact duplicates of non-empty rows
    assert (lens == 0).sum() >= 2
    assert all((D[r][D[r] > 0] > 8).all() for r in np.nonzero((fam == "uniform") & (lens >= 30))[0])    # unrelated rows


def test_the_two_references_agree_on_every_pair(B, D):
    U, inv = np.unique(B, axis=0, return_inverse=True)                   # every pair of set B is a pair of distinct rows
    inv = inv.reshape(-1)
    assert np.array_equal(U[inv], B)
    W = LT.wagner_fischer(U, U)
    assert W.dtype == np.int64 and np.array_equal(W[np.ix_(inv, inv)], D)
    assert np.array_equal(D, D.T) and (np.diag(D) == 0).all()
    lens = LT.lengths(B)
    assert (D >= abs(lens[:, None] - lens[None, :])).all() and (D <= np.maximum(lens[:, None], lens[None, :])).all()
    # `oracle_pairs` is `pair_matrix` (c_oracle.lev_pair) without the per-pair numpy round trip; operands of unequal widths
    assert np.array_equal(LT.pair_matrix(B[:42], B[200:221]), D[200:221, :42])
    assert np.array_equal(LT.wagner_fischer(B[:6, :9], B[21:63]), D[21:63, :6])


def test_banded_pairs_and_knn_lists_are_the_capped_matrix(B, D):
    for band in BANDS:
        capped = np.minimum(D, band + 1)
        assert np.array_equal(LT.oracle_pairs(B, B, band), capped)
        assert all(C.lev_pair(B[a], B[b], band) == capped[a, b] for a, b in ((0, 1), (8, 9), (29, 30), (440, 419)))
        for k in (1, 8, 63):
            want = LT.knn_from_matrix(capped, k, 1)                      # stable sort, rank 0 dropped
            got = C.lev_knn(B, k, band=band)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (band, k)
        got = C.lev_knn(B, 8, band=band, row0=37, nrows=150)
        assert np.array_equal(got[0], LT.knn_from_matrix(capped[37:187], 8, 1)[0])
    few = C.lev_knn(B[:40], 63, band=4)                                  # N < k + 1: the ranks that do not exist
    assert (few[0][:, 39:] == -1).all() and (few[1][:, 39:] == 255).all() and (few[0][:, :39] >= 0).all()
    assert np.array_equal(few[0][:, :39], LT.knn_from_matrix(np.minimum(D[:40, :40], 5), 39, 1)[0])


def test_set_b_keeps_the_gpu_tests_from_being_vacuous(B, D):
    n = len(B)
    lens = LT.lengths(B)
    off = ~np.eye(n, dtype=bool)
    lo, hi = np.minimum(lens[:, None], lens[None, :]), np.maximum(lens[:, None], lens[None, :])
    for band in BANDS:
        assert ((D == band) & off).any() and ((D == band + 1) & off).any()         # both sides of the cap
        inband = (D <= band) & off
        for edge in (32, 64, 96):                                        # lengths on either side of a dword boundary
            assert (inband & (lo < edge) & (hi >= edge)).any(), (band, edge)       # ... the last bit of a dword
            assert (inband & (lo <= edge) & (hi > edge)).any(), (band, edge)       # ... the first bit of the next
            assert (inband & (lo < edge) & (hi > edge)).any() or band == 1, (band, edge)   # 30 vs 34, 62 vs 66
        assert (inband & (lo < band)).any()                              # a sequence shorter than the band
        assert (inband & (lo == 0) & (hi > 0)).any()                     # ... the empty one
        capped = np.minimum(D, band + 1)
        idx, d = LT.knn_from_matrix(capped, 63, 1)
        assert (np.diff(d.astype(int), axis=1) == 0).any() and (d[:, 0] == d[:, 62]).any() and (d[:, 0] < d[:, 62]).any()
        assert (d[:, 0] > band).any() and (d[:, 7] <= band).any()        # rows with nothing in the band, rows with 8 and more
        assert (d[:, 62] <= band).any() or band < 7                      # ... and with all 63 ranks
        assert ((capped <= band).sum(1) > 16).any()                      # more candidates than a slot of 16 holds
    for thr in range(9):                                                 # epsilon graphs: never empty (with d = 0 kept, or
        assert ((D == thr) & off).any()                                  # from thr = 1 on), never full
    assert 0 < ((D <= 8) & off).sum() < off.sum() and ((D > 40) & off).any() and ((D <= 40) & (D > 9)).any()
    assert (((D <= 8) & off).sum(1) == 0).any()                          # and rows without a neighbour
