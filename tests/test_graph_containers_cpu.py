"""
The graph containers and the analytics built on them, without a GPU (prograph_amd/graph.py; DESIGN.md §5, "Empty slots
of a kNN table").

A slot of a kNN table with idx < 0 is no edge, for every consumer: `KNNGraph.to_tuples`, `host` and `as_csr` against
results written by hand, together with `_ranks()` cutting; a table without such slots keeps going the way of views; the
side-car round trip.  Then `rescore(..., k=, store=)` on the stand-in of tests/fake_list_native.py - the graph that used to
carry -1 into the frame - through every analytics call, against the independent model of tests/csr_model.py, and the
stand-in of `pg_csr_row_stats` itself against that model on the lists of tests/test_csr_kernels_gpu.py.
"""
import numpy as np
import pandas as pd
import pytest
import torch

import csr_model as M
import fake_list_native
import fake_native
from prograph_amd import synth
from prograph_amd.distance import local_alignment
from prograph_amd.graph import CSRGraph, KNNGraph, load_graphs, save_graphs

# 5 rows, 4 ranks: trailing slots (row 0), an interior one (row 1), a full row, an empty row, a leading one (row 4)
IDX = np.array([[3, 1, -1, -1], [2, -1, 0, 4], [0, 1, 3, 4], [-1, -1, -1, -1], [-1, 2, 3, -1]], dtype=np.int32)
DIST = np.array([[5, 3, 0, 0], [7, 0, 2, 9], [1, 1, 4, 6], [0, 0, 0, 0], [0, 8, 8, 0]], dtype=np.int32)
ROWS = [([3, 1], [5, 3]), ([2, 0, 4], [7, 2, 9]), ([0, 1, 3, 4], [1, 1, 4, 6]), ([], []), ([2, 3], [8, 8])]


def _knn(idx=IDX, dist=DIST, ncols=5, **kw):
    return KNNGraph(torch.from_numpy(idx.copy()), torch.from_numpy(dist.copy()), ncols, **kw)


def _same_rows(got, want, wdtype=np.int64):
    assert len(got) == len(want)
    for (gi, gw), (wi, ww) in zip(got, want):
        assert gi.dtype == np.int64 and gw.dtype == wdtype
        assert gi.tolist() == wi and gw.tolist() == ww


# ---------------------------------------------------------------- the containers
def test_empty_slots_are_no_edges_for_tuples_host_and_csr():
    g = _knn()
    _same_rows(g.to_tuples(), ROWS)
    idx, w = g.host()
    _same_rows(list(zip(idx, w)), ROWS)
    c = g.as_csr()
    assert isinstance(c, CSRGraph) and c.ncols == 5 and c.row0 == 0 and c.nrows == 5 and c.nnz == 11
    assert c.indptr.dtype == torch.int64 and c.indptr.tolist() == [0, 2, 5, 9, 9, 11]
    assert c.indices.dtype == torch.int32 and c.indices.tolist() == [3, 1, 2, 0, 4, 0, 1, 3, 4, 2, 3]
    assert c.weights.dtype == torch.int32 and c.weights.tolist() == [5, 3, 7, 2, 9, 1, 1, 4, 6, 8, 8]
    assert g.as_csr() is c                                                # looked at once, kept on the object
    assert c.degree(boolean_weights=True).tolist() == [2, 3, 4, 0, 2]
    # the rows are views into two flat host arrays, not a copy each
    t = g.to_tuples()
    assert all(a.base is not None and b.base is not None for a, b in t)
    # similarity, row0 and final travel with it
    s = _knn(similarity=True, row0=3, ncols=9)
    assert s.as_csr().similarity and s.as_csr().row0 == 3 and s.as_csr().ncols == 9
    _same_rows(s.to_tuples(), [(i, [np.float32(1) / np.float32(1 + v) for v in w]) for i, w in ROWS], np.float32)
    f = KNNGraph(torch.from_numpy(IDX.copy()), torch.from_numpy(DIST.astype(np.float32)), 5, final=True)
    assert f.as_csr().final and f.as_csr().weights.dtype == torch.float32
    _same_rows(f.to_tuples(), ROWS, np.float32)


@pytest.mark.parametrize("first, ncols, ranks", [(1, 5, 4), (1, 4, 3), (1, 3, 2), (0, 3, 3), (1, 1, 0), (0, 0, 0)])
def test_ranks_beyond_the_data_are_cut_before_the_slots_are_counted(first, ncols, ranks):
    """`_ranks()`: min(k, ncols - first) columns of the table exist; the rest is cut whatever it holds."""
    g = _knn(ncols=ncols, first=first)
    assert g._ranks() == ranks
    want = [([c for c in IDX[r, :ranks].tolist() if c >= 0], [d for c, d in zip(IDX[r, :ranks].tolist(), DIST[r, :ranks].tolist()) if c >= 0])
            for r in range(5)]
    _same_rows(g.to_tuples(), want)
    c = g.as_csr()
    assert c.indptr.tolist() == np.concatenate([[0], np.cumsum([len(i) for i, _ in want])]).tolist()
    assert c.indices.tolist() == [v for i, _ in want for v in i] and c.weights.tolist() == [v for _, w in want for v in w]
    # a slot beyond the ranks does not make a table ragged: rows 2's table alone is full in its first `ranks` columns
    full = KNNGraph(torch.from_numpy(IDX[2:3].copy()), torch.from_numpy(DIST[2:3].copy()), ncols, first=first)
    idx, w = full.host()
    assert isinstance(idx, np.ndarray) and idx.shape == (1, ranks) and w.shape == (1, ranks)
    cut = KNNGraph(torch.tensor([[0, 1, -1, -1]], dtype=torch.int32), torch.zeros((1, 4), dtype=torch.int32), 3, first=1)
    assert cut._ranks() == 2 and cut._without_empty_slots() is False and cut.host()[0].tolist() == [[0, 1]]


def test_a_table_without_empty_slots_goes_the_way_of_views():
    idx = torch.tensor([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], dtype=torch.int32)
    dist = torch.tensor([[1, 2, 3], [1, 1, 2], [2, 1, 1], [3, 2, 1]], dtype=torch.uint8)
    g = KNNGraph(idx, dist, 4)
    assert g._without_empty_slots() is False
    c = g.as_csr()
    assert c.indices.data_ptr() == idx.data_ptr() and c.weights.data_ptr() == dist.data_ptr()    # the table itself
    assert c.indices.dtype == torch.int32 and c.weights.dtype == torch.uint8
    assert c.indptr.tolist() == [0, 3, 6, 9, 12]
    hi, hw = g.host()
    assert isinstance(hi, np.ndarray) and hi.shape == (4, 3) and hi.dtype == np.int64 and hw.shape == (4, 3)
    assert hi.tolist() == idx.tolist() and hw.tolist() == dist.tolist()
    t = g.to_tuples()
    assert all(a.base is t[0][0].base is not None and b.base is t[0][1].base is not None for a, b in t)   # rows of two arrays
    assert [a.tolist() for a, _ in t] == idx.tolist()
    # the look is made once: a later as_csr does not reduce again
    seen = []
    real_all = torch.Tensor.all
    try:
        torch.Tensor.all = lambda self, *a, **k: (seen.append(1), real_all(self, *a, **k))[1]
        h = KNNGraph(idx, dist, 4)
        h.as_csr(), h.host(), h.to_tuples(), h.as_csr()
    finally:
        torch.Tensor.all = real_all
    assert len(seen) == 1


def test_side_car_round_trip_keeps_the_slots_and_their_meaning(tmp_path, monkeypatch):
    fake_native.install(monkeypatch)
    g = _knn()
    e = g.as_csr()
    path = str(tmp_path / "graphs.npz")
    save_graphs(path, {"K": g, "E": e})
    back = load_graphs(path)
    assert torch.equal(back["K"].idx, g.idx) and torch.equal(back["K"].dist, g.dist)   # the table as it was, -1 included
    _same_rows(back["K"].to_tuples(), ROWS)
    for name in ("indptr", "indices", "weights"):
        assert torch.equal(getattr(back["K"].as_csr(), name), getattr(e, name))
        assert torch.equal(getattr(back["E"], name), getattr(e, name))
    # a side-car whose table names a column below -1, or a CSR any negative column, is still refused
    bad = _knn()
    bad.idx[0, 0] = -2
    save_graphs(path, {"K": bad, "E": CSRGraph(e.indptr, e.indices - 1, e.weights, 5)})
    assert load_graphs(path) == {}


# ---------------------------------------------------------------- rescore(k=, store=) through the analytics
N, L, A = 24, 20, 21


def _score_table(seed):
    rng = np.random.default_rng(seed)
    S = rng.integers(-4, 2, (A, A))
    S = np.triu(S) + np.triu(S, 1).T
    S[np.arange(A), np.arange(A)] = rng.integers(2, 6, A)
    return S


@pytest.fixture()
def stored(tmp_path, monkeypatch):
    """A Prograph with the graph `R` = rescore(k=4, store="R") of a candidate graph whose rows have 0..6 entries."""
    from prograph_amd import Prograph
    fake_list_native.install(monkeypatch)
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=8, seed=5, members=4)
    f = tmp_path / "containers.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": np.random.default_rng(0).uniform(0, 1, N)}).to_csv(f)
    P = Prograph(file=str(f))
    rng = np.random.default_rng(16)
    lens = rng.integers(0, 7, N)
    lens[:3] = (0, 1, 6)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.concatenate([np.sort(rng.choice(N, n, replace=False)) for n in lens]).astype(np.int32)
    cand = CSRGraph(torch.from_numpy(indptr), torch.from_numpy(cols), torch.zeros(len(cols), dtype=torch.int32), N)
    G = P.rescore(cand, local_alignment(_score_table(3), 3, gap_open=2), k=4, store="R")
    return P, G, lens


def _f(P):
    from sklearn.preprocessing import MinMaxScaler
    return MinMaxScaler().fit_transform(P("Fitness").to_numpy().reshape(-1, 1)).reshape(-1)


def _model_of(G, f, boolean):
    idx, w = G.host()
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in idx])])
    flat = lambda rows, dt: np.concatenate([np.asarray(r) for r in rows]).astype(dt) if indptr[-1] else np.zeros(0, dt)
    return M.analytics(indptr, flat(idx, np.int64), None if boolean else flat(w, np.float64), f, G.nrows)


def test_a_rescored_knn_graph_puts_no_empty_slot_into_the_frame(stored):
    P, G, lens = stored
    assert isinstance(G, KNNGraph) and int((G.idx < 0).sum()) > 0
    short = np.minimum(lens, 4)
    assert (short < 4).sum() >= 10 and (short == 0).sum() >= 1
    col = P("R")
    assert [len(i) for i, _ in col] == short.tolist() and [len(w) for _, w in col] == short.tolist()
    assert all((np.asarray(i) >= 0).all() for i, _ in col)
    assert P._device_graph("R") is not None                               # ... and the stored graph answers for the column
    for i, (idx, w) in enumerate(col):
        keep = G.idx[i] >= 0
        assert idx.tolist() == G.idx[i][keep].tolist() and w.tolist() == G.dist[i][keep].tolist()


@pytest.mark.parametrize("path", ["device", "host"])
def test_analytics_of_a_rescored_knn_graph_equal_the_model(stored, path):
    """Integer scores, 24 rows: every sum is exact, so the device path (the stand-in of `pg_csr_row_stats`) and the host
    path both equal the model; the Dirichlet energy to the rounding of its float64 sum."""
    P, G, lens = stored
    if path == "host":
        P.csr_graphs.clear()
        assert P._device_graph("R") is None
    f = _f(P)
    for boolean in (False, True):
        m = _model_of(G, f, boolean)
        assert np.array_equal(P.degree("R", boolean), m["degree"])
        assert np.array_equal(P.adjacency("R", boolean).toarray(), m["adjacency"])
        for mode in ("outdegree", "indegree"):
            assert np.array_equal(P.laplacian("R", boolean, mode).toarray(), m["laplacian"][mode])
            got = float(np.asarray(P.dirichlet("R", boolean, mode=mode)).reshape(-1)[0])
            assert abs(got - m["dirichlet"][mode]) <= (N * N + N) * 2.0 ** -52 * m["dirichlet_abs"][mode]
            if path == "device":
                assert np.array_equal(P._device_graph("R").laplacian_diagonal(boolean, mode), m["laplacian"][mode].diagonal())
    lv, want = P.local_variance("R"), _model_of(G, f, True)["local_variance"]
    assert np.array_equal(np.isnan(lv), np.isnan(want)) and np.isnan(want).sum() == (lens == 0).sum()
    assert np.all(np.abs(lv - want)[~np.isnan(want)] <= 8 * 2.0 ** -52)     # at most 4 terms below 1, a quotient, a difference
    nx = P.graph_to_networkx("R")
    names = list(P("Sequence"))
    I, J, _ = P.get_neighbour_coords("R")
    assert (J >= 0).all() and len(I) == int(np.minimum(lens, 4).sum())
    assert {frozenset((names[i], names[j])) for i, j in zip(I, J)} == {frozenset(e) for e in nx.edges()}


# ---------------------------------------------------------------- the stand-in of pg_csr_row_stats
@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("weights", ["none", "u8", "f32"])
@pytest.mark.parametrize("nrows, row0", [(1, 0), (3, 37), (4, 0), (5, 37), (19, 0), (19, 37)])
def test_the_stand_in_of_row_stats_equals_the_model(nrows, row0, weights, negative):
    indptr, indices = M.edge_lists(nrows, row0, M.SEED[nrows])
    if negative:
        indices = M.with_negative_columns(indptr, indices)
    w, f = M.exact_weights(weights, len(indices)), M.exact_values(M.NCOLS)
    want = M.row_stats(indptr, indices, w, f, row0, M.NCOLS)
    got = fake_native._csr_row_stats(torch.from_numpy(indptr), torch.from_numpy(indices), None if w is None else torch.from_numpy(w),
                                     f=torch.from_numpy(f), want=M.KEYS, row0=row0, ncols=M.NCOLS)
    for key in M.KEYS:
        assert np.array_equal(got[key].numpy(), want[key]), key
