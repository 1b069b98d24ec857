"""
The inputs of tests/test_knn_sym_edges_gpu.py sit where that file needs them - pinned here with the C oracle and the host plan,
without a GPU (tests/knn_sym_testdata.py builds them).

The symmetric sweep decides a row by two comparisons with the cap c - a pair is delivered to its higher row when d < c, a row
is evicted when its rank-k distance is >= c - and by one with its slot (more than capL delivered keys: evicted), and a row's
lists are at most sixteen.  A ladder row's rank-k distance is a formula, a duplicate's delivered keys are its position in its
cluster, a block's pieces are the plan's: each statement below names the rows that sit one below a seam, on it and above it.
A ladder or a cluster moved off its seam (another length, another stride) fails here, not silently on the GPU.
"""
import numpy as np
import pytest

import knn_sym_testdata as D
from test_knn_sym_cpu import SLOTS, plan


def oracle_knn(tok, k):
    from oracle import c_oracle as Co
    return Co.knn(tok, k)


def hamming(tok):
    t = tok.astype(np.int16)
    return (t[:, None, :] != t[None, :, :]).sum(axis=2)


@pytest.mark.parametrize("l", [1, 5, 31, 32, 64])
def test_ladder_distances_are_index_differences(l):
    m = min(l + 1, 24)
    lad = D.ladder(D.filler(1, l, l)[0], m)
    assert lad.min() >= 1 and lad.max() <= 20
    assert np.array_equal(hamming(lad), np.abs(np.arange(m)[:, None] - np.arange(m)[None, :]))
    with pytest.raises(AssertionError):
        D.ladder(D.filler(1, l, l)[0], l + 2)                # one member more than the positions allow


@pytest.mark.parametrize("order", D.ORDERS)
@pytest.mark.parametrize("l", [64, 32])
def test_ladders_are_unrelated_to_each_other_and_to_the_rest(l, order):
    """every pair that is not inside one ladder is at or above the cap in use (and above the largest forced one below 65)"""
    tok, rows = D.ladder_case(l, order)
    assert tok.shape == (D.LADDER_N, l) and [len(r) for r in rows] == list(D.LADDER_M)
    d = hamming(tok)
    inside = np.eye(len(tok), dtype=bool)
    for r in rows:
        inside[np.ix_(r, r)] = True
        assert np.array_equal(d[np.ix_(r, r)], np.abs(np.arange(len(r))[:, None] - np.arange(len(r))[None, :]))
    assert d[~inside].min() >= max(D.CAPS[l], D.MAX_K + 1)   # (k <= 19: a rank inside a ladder is never tied with one outside)
    between = d[np.ix_(rows[0], rows[1])].min()
    print(f"L={l} {order}: minimum distance outside the ladders {d[~inside].min()}, between them {between}")
    assert between >= D.CAPS[l]
    if order == "straddling":
        assert rows[0][0] == 56 and rows[0][-1] == 79 and rows[1][0] == 120 and rows[1][-1] == 140
    if order == "interleaved":
        assert np.array_equal(np.sort(np.concatenate(rows))[:42], np.arange(3, 45))
    if order == "descending":
        assert (np.diff(rows[0]) == -1).all() and (np.diff(rows[1]) == -1).all()


@pytest.mark.parametrize("l", [64, 32])
def test_cap_seams_of_the_ladders(l):
    """c = the cap.  End members have rank-k distance k, interior ones ceil(k / 2), a member j from an end k - j until that:
      k = c - 1    no ladder row reaches the cap; the end members sit at exactly c - 1
      k = c        the end members sit exactly at c (evicted), their neighbours at c - 1 (kept)
      k = 2c - 2   interior rows sit at c - 1 (kept), the rows within c - 1 of an end are at or above the cap
      k = 2c - 1   every ladder row is at or above the cap, interior ones exactly at it"""
    c = D.CAPS[l]
    assert D.cap_ks(c) == (c - 1, c, 2 * c - 2, 2 * c - 1) and min(D.LADDER_M) >= 2 * c - 1 and D.LADDER_M[0] >= 2 * c + 2
    tok, rows = D.ladder_case(l, "ascending")
    for k in D.cap_ks(c):
        dist = oracle_knn(tok, k)[1]
        for r in rows:
            m = len(r)
            got = dist[r, k - 1].astype(int)
            assert list(got) == [D.rank_k_distance(m, j, k) for j in range(m)]          # the formula is the oracle's answer
            below, at, above = got < c - 1, got == c, got > c
            ends = np.zeros(m, dtype=bool)
            ends[[0, m - 1]] = True
            if k == c - 1:
                assert got.max() == c - 1 and (got[ends] == c - 1).all() and (got[~ends] < c - 1).all()
            elif k == c:
                assert (at == ends).all() and got[1] == c - 1 and got[m - 2] == c - 1 and not above.any()
            elif k == 2 * c - 2:
                interior = (np.arange(m) >= c - 1) & (np.arange(m) <= m - c)
                assert interior.sum() >= 3 and (got[interior] == c - 1).all() and (got[~interior] >= c).all()
                assert got[c - 2] == c and got[m - c + 1] == c and got[0] == k
            else:
                assert (got >= c).all() and got.min() == c and got[m // 2] == c and not below.any()
    # the filler rows: no neighbour below the cap at all
    others = np.setdiff1d(np.arange(len(tok)), np.concatenate(rows))
    assert oracle_knn(tok, 1)[1][others, 0].min() >= c


@pytest.mark.parametrize("guess", [3, 65])
def test_forced_caps(guess):
    """PG_KNN_GUESS=3: its four ks are 2..5 and the seams are the default cap's, at other rows; 65: above every distance"""
    assert D.cap_ks(3) == (2, 3, 4, 5) and D.cap_ks(65) == ()
    for l in (64, 32):
        tok, rows = D.ladder_case(l, "ascending")
        if guess == 65:
            assert hamming(tok).max() < 65
            continue
        dist = oracle_knn(tok, 4)[1]
        got = dist[rows[0], 3].astype(int)
        assert got[0] == 4 and got[1] == 3 and (got[2:-2] == 2).all()


@pytest.mark.parametrize("size,stride", D.SLOT8_CLUSTERS)
def test_slot_seams_of_eight(size, stride):
    """member j receives exactly j keys: members 7, 8 and 9 are one below a slot of 8, exactly at it (kept, every key needed from
    k = 9 on) and one above (evicted); with stride 2 the row behind an overflowing member belongs to the other cluster, which
    lags 8 members behind: a row that keeps its slot and reads it from the first entry on"""
    capl = 8
    tok, a, b = D.duplicates(D.SLOT8_N, size, stride)
    got = D.delivered(tok, D.CAPS[64])
    assert size > capl + 1 and list(got[a]) == list(range(size))
    assert got[a[capl - 1]] == capl - 1 and got[a[capl]] == capl and got[a[capl + 1]] == capl + 1
    if stride == 2:
        assert list(got[b]) == list(range(size)) and not np.array_equal(tok[a[0]], tok[b[0]])
        over = a[got[a] > capl]                              # A's overflowing members: the row behind each is B's, keeps its slot
        assert len(over) == size - capl - 1 and np.isin(over + 1, b).all()              # and reads it from the first entry on
        near = over[:capl] + 1
        assert np.array_equal(near, b[1:1 + len(near)]) and list(got[near]) == list(range(1, 1 + len(near)))
    assert got.sum() == (1 if b is None else 2) * size * (size - 1) // 2              # nobody else receives anything
    for k in D.SLOT8_KS:
        idx, dist = oracle_knn(tok, k)
        for rows in (a,) if b is None else (a, b):
            want = min(k + 1, size)                          # the k + 1 smallest keys: the cluster's lowest indices (rank 0: member 0)
            for j in (capl - 1, capl, capl + 1):
                assert np.array_equal(idx[rows[j], :want - 1], rows[1:want]) and want > capl + 1
                assert (dist[rows[j], :want - 1] == 0).all()
                assert k < size or dist[rows[j], k - 1] >= D.CAPS[64]                   # cluster smaller than k + 1: above the cap
    assert min(D.SLOT8_KS) >= capl + 1                       # every delivered key of members 8 and 9 is among their k + 1 smallest


def test_slot_seam_of_the_production_slot():
    capl = 256
    tok, a, b = D.duplicates(D.SLOT256_N, D.SLOT256_SIZE, 1, start=D.SLOT256_START)
    assert b is None and len(a) > capl + 1
    got = D.delivered(tok[:a[-1] + 1], D.CAPS[64])
    assert list(got[a]) == list(range(D.SLOT256_SIZE)) and got.sum() == D.SLOT256_SIZE * (D.SLOT256_SIZE - 1) // 2
    assert [got[a[capl + i]] for i in (-1, 0, 1)] == [capl - 1, capl, capl + 1]
    assert [int(a[capl + i]) for i in (-1, 0, 1)] == [355, 356, 357]
    idx, dist = oracle_knn(tok, 19)
    # member 256: rank 0 is member 0, ranks 1..19 members 1..19 - delivered keys all; its own (k+1)-th key (0, row 275) lies
    # above every one of the 256 delivered keys, so the merge packs all 256
    assert np.array_equal(idx[a[capl]], a[1:20]) and (dist[a[capl]] == 0).all()


def block0_pieces(n, piece):
    p = plan(n, SLOTS, int(piece))
    return int((p[:, 0] == 0).sum()), p


def test_sixteen_pieces_and_the_clamp():
    n16, piece16 = D.PIECES_16
    n17, piece17 = D.PIECES_17
    got, p = block0_pieces(n16, piece16)
    assert got == 16 and D.pieces_asked(n16, piece16) == 16
    assert max((p[:, 0] == b).sum() for b in range((n16 + 63) // 64)) == 16
    got, p = block0_pieces(n17, piece17)
    assert D.pieces_asked(n17, piece17) == 17 and got == 16                             # asked for 17, clamped
    assert (p[:, 0] == 1).sum() == 16 and (p[:, 0] == 2).sum() == 16                   # (blocks 1 and 2: 51 and 50 super-tiles)
    # the smallest such graphs: one row fewer is one super-tile fewer
    assert block0_pieces(n16 - 1, piece16)[0] == 15 and D.pieces_asked(n17 - 1, piece17) == 16
    # ... and no shorter graph reaches sixteen with any piece length, fixed or guided
    for nst in range(1, 48):
        for piece in (0, 1, 2, 3, 4, 5, 6, 8):
            for slots in (8, SLOTS):
                assert (plan(nst * 128, slots, piece)[:, 0] == 0).sum() < 16, (nst, piece, slots)


def test_shapes_of_the_gpu_file():
    for n in D.WIDTH_NS:
        for l in D.WIDTHS:
            tok = D.width_case(n, l)
            assert tok.shape == (n, l) and tok.min() >= 1 and tok.max() <= 20
            m = min(l + 1, 24)
            assert np.array_equal(hamming(tok[56:56 + m]), np.abs(np.arange(m)[:, None] - np.arange(m)[None, :]))
            assert (hamming(tok[80:128:2]) == 0).all() and (hamming(tok[81:128:2]) == 0).all()
    # L <= 5: every pair is below the one-group cap - row r receives r keys, rows from 257 on overflow the production slot
    for l in (1, 5):
        assert l < D.CAPS[32]
        assert np.array_equal(D.delivered(D.width_case(1000, l), D.CAPS[32]), np.arange(1000))
    for n in D.TINY_NS:
        for l in D.TINY_LS:
            tok = D.tiny_case(n, l)
            assert tok.shape == (n, l) and np.array_equal(tok[n - 1], tok[0])
            idx, dist = oracle_knn(tok, 19)
            assert (idx[:, n - 1:] == -1).all() and (dist[:, n - 1:] == 255).all()     # N < k + 1: ranks that do not exist
            assert (idx[:, :n - 1] >= 0).all()
