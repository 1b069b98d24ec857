"""tests/knn_sym_group_testdata.py pinned to its seams without a GPU: the counts of delivered keys per row and per group of
sixteen receiver rows, from the definition (pairs with a lower index and d < cap)."""
import numpy as np

import knn_sym_testdata as D
import knn_sym_group_testdata as G


def test_seam_clusters_sit_on_the_seams():
    for n in G.SEAM_NS:
        tok, (a, b, c) = G.seam_case(n)
        assert sorted(list(a) + list(b)) == list(G.SEAM_ROWS) and n % 16 != 0
        got = D.delivered(tok, G.CAP)
        for rows in (a, b, c):
            assert [got[r] for r in rows] == list(range(len(rows)))      # member j: j delivered keys
        assert got.sum() == sum(len(r) * (len(r) - 1) // 2 for r in (a, b, c))
        if n > 129:
            assert (n - 1) // 16 != (n - 17) // 16 and len(c) == 3
        else:
            assert got[128] == 4 and G.group_entries(tok, G.CAP)[8] == 4   # the last group: one row, capacity capL


def test_a_log_exactly_full_and_one_over():
    cap_g = G.GROUP * G.FULL_CAPL
    kept = G.full_case(False)
    got = D.delivered(kept, G.CAP)
    assert (got[G.FULL_RECEIVERS] == G.FULL_CAPL).all() and G.group_entries(kept, G.CAP)[8] == cap_g
    assert (G.group_entries(kept, G.CAP)[:8] == 2 * 28).all() and got[144:].sum() == 0
    over = G.full_case(True)
    got = D.delivered(over, G.CAP)
    assert got[129] == 9 and (np.delete(got[G.FULL_RECEIVERS], 1) == 8).all() and G.group_entries(over, G.CAP)[8] == cap_g + 1
    assert max(G.FULL_KS) == G.FULL_CAPL


def test_a_batch_in_64_groups_and_a_batch_in_one():
    tok, recv = G.spread_case()
    got = D.delivered(tok, G.CAP)
    assert got.sum() == 64 and (got[recv] == 1).all()
    assert len(set(recv // 16)) == 64 and set(recv % 16) == set(range(16)) and (np.diff(recv) >= 16).all()
    tok = G.dense_case()
    got = D.delivered(tok, G.CAP)
    assert len(set(G.DENSE_RECEIVERS // 16)) == 1
    assert [got[r] for r in G.DENSE_RECEIVERS] == [128 + j for j in range(16)]
    assert G.group_entries(tok, G.CAP)[16] == 16 * 128 + 120 < 16 * 256


def test_wide_cap_delivers_every_ladder_distance():
    for order in ("ascending", "interleaved"):
        tok, rows = G.wide_case(order)
        got = D.delivered(tok, int(G.WIDE_GUESS))
        assert got[rows[0]].max() >= 64 and len(tok) == G.WIDE_N
        ent = G.group_entries(tok, int(G.WIDE_GUESS))
        assert ent.min() <= 16 * 256 < ent.max()                          # logs that keep their entries and logs that overflow
