"""
The graph operations `sorted`, `transpose`, `symmetrize` without a GPU:

- the model of tests/graph_ops_model.py once against scipy.sparse, on a graph scipy can express (positive float32 weights, no
  duplicate entries, where a missing entry and a zero are the same thing);
- the NumPy stand-in of tests/fake_graph_native.py against the model, bit for bit, on the edge lists of tests/csr_model.py
  (row lengths around a wave's 64 entries, a hub column, repeated columns, `row0 != 0`, no-edge entries) in all five weight
  dtypes, NaN and both zeros among the floats;
- the containers on the stand-in: a `KNNGraph` with empty slots, `row0 != 0`, `nrows != ncols`, the `ValueError`s, a side-car round
  trip of a symmetrised graph, and `Prograph.symmetrize(store=)` through `degree` / `dirichlet` against `csr_model.analytics`;
- the argument checks of the C entries, which return before any launch, with a NULL stream.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import csr_model as M
import fake_graph_native
import fake_native
import graph_ops_model as G
from prograph_amd import _native, synth
from prograph_amd.graph import CSRGraph, KNNGraph, load_graphs, save_graphs

DTYPES, weights_of, square_lists = G.DTYPES, G.weights_of, G.square_lists


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def arrays(triple):
    return tuple(t.numpy() for t in triple)


# ---------------------------------------------------------------- the model against scipy
def test_the_model_equals_scipy_on_a_graph_scipy_can_express():
    from scipy import sparse
    rng = np.random.default_rng(3)
    n = 40
    dense = np.where(rng.random((n, n)) < 0.15, rng.integers(1, 1000, (n, n)) / 8.0, 0.0).astype(np.float32)
    A = sparse.csr_matrix(dense)
    A.sort_indices()
    perm = np.concatenate([rng.permutation(np.arange(a, b)) for a, b in zip(A.indptr[:-1], A.indptr[1:])]).astype(np.int64)
    indptr, indices, w = A.indptr.astype(np.int64), A.indices[perm].astype(np.int32), A.data[perm]      # rows in a random order

    def scipy_arrays(X):
        X = sparse.csr_matrix(X)
        X.eliminate_zeros()
        X.sort_indices()
        return X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data.astype(np.float32)

    G.same(G.sorted_rows(indptr, indices, w, n), scipy_arrays(A))
    G.same(G.transpose(indptr, indices, w, n), scipy_arrays(A.T.tocsr()))
    G.same(G.symmetrize(indptr, indices, w, "union", "max"), scipy_arrays(A.maximum(A.T)))
    G.same(G.symmetrize(indptr, indices, w, "mutual", "min"), scipy_arrays(A.minimum(A.T)))
    rect = sparse.csr_matrix(dense[:7])                                     # 7 rows of node 100.. over 40 columns
    rect.sort_indices()
    t = G.transpose(rect.indptr.astype(np.int64), rect.indices.astype(np.int32), rect.data, n, row0=100)
    want = scipy_arrays(rect.T.tocsr())
    G.same(t, (want[0], want[1] + 100, want[2]))


# ---------------------------------------------------------------- the stand-in against the model
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("negative", [False, True], ids=["edges", "negative_columns"])
@pytest.mark.parametrize("nrows, row0", [(1, 0), (3, 37), (4, 0), (5, 37), (19, 0), (19, 37)])
def test_the_stand_in_sorts_and_transposes_as_the_model(nrows, row0, negative, dtype):
    indptr, indices = M.edge_lists(nrows, row0, M.SEED[nrows])
    if negative:
        indices = M.with_negative_columns(indptr, indices)
    w = weights_of(dtype, len(indices), nrows)
    G.same(arrays(fake_graph_native.csr_sort_rows(T(indptr), T(indices), T(w), M.NCOLS)), G.sorted_rows(indptr, indices, w, M.NCOLS))
    G.same(arrays(fake_graph_native.csr_transpose(T(indptr), T(indices), T(w), M.NCOLS, row0=row0)),
           G.transpose(indptr, indices, w, M.NCOLS, row0))
    # columns at or past ncols are no edges either
    G.same(arrays(fake_graph_native.csr_transpose(T(indptr), T(indices), T(w), 100, row0=row0)), G.transpose(indptr, indices, w, 100, row0))
    G.same(arrays(fake_graph_native.csr_sort_rows(T(indptr), T(indices), T(w), 100)), G.sorted_rows(indptr, indices, w, 100))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("negative", [False, True], ids=["edges", "negative_columns"])
@pytest.mark.parametrize("nrows", [1, 3, 4, 5, 19])
def test_the_stand_in_symmetrises_as_the_model(nrows, negative, dtype):
    indptr, indices = square_lists(nrows, negative)
    w = weights_of(dtype, len(indices), nrows)
    for mode in ("union", "mutual"):
        for combine in ("min", "max"):
            got = arrays(fake_graph_native.csr_symmetrize(T(indptr), T(indices), T(w), mode=mode, combine=combine))
            G.same(got, G.symmetrize(indptr, indices, w, mode, combine))
            G.same(G.transpose(*got, nrows), got)                           # S equals its transpose, bit for bit


def test_the_model_on_a_graph_small_enough_to_read():
    """0 -> 1 (5), 1 -> 0 (3), 0 -> 2 (7), 2 -> 2 (4) and (9), 1 -> 0 again (8), one empty slot."""
    indptr = np.array([0, 3, 5, 7], dtype=np.int64)
    indices = np.array([2, -1, 1, 0, 0, 2, 2], dtype=np.int32)
    w = np.array([7, 99, 5, 3, 8, 4, 9], dtype=np.int16)
    G.same(G.sorted_rows(indptr, indices, w, 3), (np.array([0, 2, 4, 6]), np.array([1, 2, 0, 0, 2, 2], np.int32), np.array([5, 7, 3, 8, 4, 9], np.int16)))
    G.same(G.transpose(indptr, indices, w, 3), (np.array([0, 2, 3, 6]), np.array([1, 1, 0, 0, 2, 2], np.int32), np.array([3, 8, 5, 7, 4, 9], np.int16)))
    G.same(G.symmetrize(indptr, indices, w, "union", "min"),
           (np.array([0, 2, 3, 5]), np.array([1, 2, 0, 0, 2], np.int32), np.array([3, 7, 3, 7, 4], np.int16)))
    G.same(G.symmetrize(indptr, indices, w, "mutual", "max"),
           (np.array([0, 1, 2, 3]), np.array([1, 0, 2], np.int32), np.array([8, 8, 9], np.int16)))


# ---------------------------------------------------------------- the containers
IDX = np.array([[3, 1, -1, -1], [2, -1, 0, 4], [0, 1, 3, 4], [-1, -1, -1, -1], [-1, 2, 3, -1]], dtype=np.int32)
DIST = np.array([[5, 3, 0, 0], [7, 0, 2, 9], [1, 1, 4, 6], [0, 0, 0, 0], [0, 8, 8, 0]], dtype=np.int32)


def _graph_arrays(g):
    return g.indptr.numpy(), g.indices.numpy(), g.weights.numpy()


def test_a_knn_table_with_empty_slots_through_the_three_methods(monkeypatch):
    fake_graph_native.install(monkeypatch)
    for table in (KNNGraph(T(IDX), T(DIST), 5, similarity=True),              # the CSR without the slots
                  KNNGraph(T(IDX), T(DIST), 5).as_csr(),
                  CSRGraph(T(np.arange(0, 21, 4)), T(IDX.reshape(-1)), T(DIST.reshape(-1)), 5, final=True)):   # the slots as -1 entries
        e = table.as_csr() if isinstance(table, KNNGraph) else table
        src = _graph_arrays(e)
        s, t = table.sorted(), table.transpose()
        G.same(_graph_arrays(s), G.sorted_rows(*src, 5))
        G.same(_graph_arrays(t), G.transpose(*src, 5))
        assert (s.nrows, s.ncols, s.row0, t.nrows, t.ncols, t.row0) == (5, 5, 0, 5, 5, 0)
        for mode in ("union", "mutual"):
            u = table.symmetrize(mode)
            G.same(_graph_arrays(u), G.symmetrize(*src, mode, "min"))
            assert isinstance(u, CSRGraph) and (u.similarity, u.final) == (e.similarity, e.final) and u.weights.dtype == torch.int32
    mutual = KNNGraph(T(IDX), T(DIST), 5).symmetrize("mutual", combine="max")
    assert [(i.tolist(), w.tolist()) for i, w in mutual.to_tuples()] == [([1], [3]), ([0, 2], [3, 7]), ([1, 4], [7, 8]), ([], []), ([2], [8])]


def test_shards_and_rectangles_transpose_and_sort_but_do_not_symmetrise(monkeypatch):
    fake_graph_native.install(monkeypatch)
    indptr, indices = M.edge_lists(5, 37, M.SEED[5])
    w = weights_of(np.float16, len(indices))
    g = CSRGraph(T(indptr), T(indices), T(w), M.NCOLS, similarity=True, row0=37, final=True)
    t, s = g.transpose(), g.sorted()
    assert (t.nrows, t.ncols, t.row0, t.similarity, t.final) == (M.NCOLS, 42, 0, True, True)
    assert (s.nrows, s.ncols, s.row0, s.similarity, s.final) == (5, M.NCOLS, 37, True, True)
    G.same(_graph_arrays(t), G.transpose(indptr, indices, w, M.NCOLS, 37))
    G.same(_graph_arrays(s), G.sorted_rows(indptr, indices, w, M.NCOLS))
    back = t.transpose()                                                    # rows 0..41 of which the first 37 are empty
    assert (back.nrows, back.ncols, back.row0) == (42, M.NCOLS, 0) and int(back.indptr[37]) == 0
    G.same((back.indptr.numpy()[37:], back.indices.numpy(), back.weights.numpy()), _graph_arrays(s))
    with pytest.raises(ValueError, match="square"):
        g.symmetrize()
    with pytest.raises(ValueError, match="square"):
        CSRGraph(T(indptr), T(indices), T(w), M.NCOLS).symmetrize()            # row0 = 0 but 5 rows over 300 columns
    sq_indptr, sq_indices = square_lists(5)
    sq = CSRGraph(T(sq_indptr), T(sq_indices), T(weights_of(np.uint8, len(sq_indices))), 5)
    with pytest.raises(ValueError, match="mode"):
        sq.symmetrize("both")
    with pytest.raises(ValueError, match="combine"):
        sq.symmetrize("union", combine="mean")
    assert sq.symmetrize("mutual").weights.dtype == torch.uint8


def test_a_symmetrised_graph_goes_through_the_side_car(tmp_path, monkeypatch):
    fake_native.install(monkeypatch)
    fake_graph_native.install(monkeypatch)
    s = KNNGraph(T(IDX), T(DIST.astype(np.float32)), 5, final=True).symmetrize("union", combine="max")
    path = str(tmp_path / "graphs.npz")
    save_graphs(path, {"S": s, "T": s.transpose()})
    back = load_graphs(path)
    for name in ("S", "T"):                                                 # and the transpose of S is S
        assert (back[name].ncols, back[name].row0, back[name].final, back[name].similarity) == (5, 0, True, False)
        G.same(_graph_arrays(back[name]), _graph_arrays(s))
    assert [i.tolist() for i, _ in back["S"].to_tuples()] == [[1, 2, 3], [0, 2, 4], [0, 1, 3, 4], [0, 2, 4], [1, 2, 3]]


# ---------------------------------------------------------------- Prograph.symmetrize(store=) through the analytics
N, L = 40, 12


@pytest.fixture()
def pgraph(tmp_path, monkeypatch):
    from prograph_amd import Prograph
    fake_native.install(monkeypatch)
    fake_graph_native.install(monkeypatch)
    tok = synth.clustered_tokens(N, L, seed=3, members=3)
    f = tmp_path / "ops.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": np.random.default_rng(1).uniform(0, 1, N)}).to_csv(f)
    P = Prograph(file=str(f))
    P.build_graph(k=4, store="K")
    return P


def _analytics(g, f):
    indptr, idx, w = g.host()
    return M.analytics(indptr, idx, w.astype(np.float64), f, g.nrows)


@pytest.mark.parametrize("source", ["name", "container", "column"])
@pytest.mark.parametrize("mode", ["union", "mutual"])
def test_prograph_symmetrize_stores_a_graph_the_analytics_run_on(pgraph, mode, source):
    from sklearn.preprocessing import MinMaxScaler
    P = pgraph
    K = P.csr_graphs["K"]
    if source == "column":
        P.csr_graphs.clear()                                                # the column alone: uploaded from its tuples
        assert P._device_graph("K") is None
    S = P.symmetrize(K if source == "container" else "K", mode=mode, store="M")
    assert isinstance(S, CSRGraph) and P._device_graph("M") is S
    want = G.symmetrize(*_graph_arrays(K.as_csr()), mode, "min")
    assert np.array_equal(S.indptr.numpy(), want[0]) and np.array_equal(S.indices.numpy(), want[1])
    assert np.array_equal(S.weights.numpy().astype(np.int64), want[2].astype(np.int64))
    assert 0 < S.nnz and (mode == "union") == (S.nnz > K.as_csr().nnz)       # a kNN graph is not symmetric: the two modes differ
    f = MinMaxScaler().fit_transform(P("Fitness").to_numpy().reshape(-1, 1)).reshape(-1)
    m = _analytics(S, f)
    assert np.array_equal(P.degree("M"), m["degree"])
    got = float(np.asarray(P.dirichlet("M")).reshape(-1)[0])
    assert abs(got - m["dirichlet"]["outdegree"]) <= (N * N + N) * 2.0 ** -52 * m["dirichlet_abs"]["outdegree"]
    # the smoothness functional: on a symmetric adjacency f^T L f is half the sum of w (f_i - f_j)^2 over the stored entries
    indptr, idx, w = S.host()
    rows = np.repeat(np.arange(N), np.diff(indptr))
    half = 0.5 * float(np.sum(w * (f[rows] - f[idx]) ** 2))
    assert abs(got - half) <= 1e-9 * max(1.0, abs(half))
    tuples = P.symmetrize("K", mode=mode, output="tuples")
    assert [i.tolist() for i, _ in tuples] == [r.tolist() for r in np.split(want[1], want[0][1:-1])]


# ---------------------------------------------------------------- the C entries refuse bad arguments before any launch
def test_graph_entries_validate_their_arguments_without_gpu():
    lib = _native.lib()
    p = ctypes.c_void_p(4096)                                               # never dereferenced
    BAD = -1
    assert lib.pg_csr_sort_workspace(10) == 80 and lib.pg_csr_sort_workspace(0) == 8 and lib.pg_csr_sort_workspace(-1) == -1
    assert lib.pg_csr_transpose_workspace(10, 3) == 92 and lib.pg_csr_transpose_workspace(-1, 3) == -1
    assert lib.pg_csr_symmetrize_workspace(10, 6) == 160 and lib.pg_csr_symmetrize_workspace(1, -1) == -1

    def count(indptr=p, indices=p, nrows=4, nnz=10, ncols=4, counts=p, ws=p, nbytes=80):
        return lib.pg_csr_sort_rows_count(indptr, indices, nrows, nnz, ncols, counts, ws, nbytes, None)

    def fill(indptr=p, w=p, eb=4, nrows=4, nnz=10, counts=p, out_indptr=p, out_idx=p, out_w=p, ws=p, nbytes=80):
        return lib.pg_csr_sort_rows_fill(indptr, w, eb, nrows, nnz, counts, out_indptr, out_idx, out_w, ws, nbytes, None)

    def hist(indices=p, nnz=10, ncols=4, counts=p):
        return lib.pg_csr_histogram(indices, nnz, ncols, counts, None)

    def transpose(indptr=p, indices=p, w=p, eb=2, nrows=4, nnz=10, ncols=4, row0=0, t_indptr=p, t_idx=p, t_w=p, ws=p, nbytes=96):
        return lib.pg_csr_transpose(indptr, indices, w, eb, nrows, nnz, ncols, row0, t_indptr, t_idx, t_w, ws, nbytes, None)

    def sym_count(a_indptr=p, a_idx=p, a_w=p, nnz_a=10, t_indptr=p, t_idx=p, t_w=p, nnz_t=10, eb=4, kind=2, mode=0, combine=0, nrows=4,
                  counts=p, ws=p, nbytes=200):
        return lib.pg_csr_symmetrize_count(a_indptr, a_idx, a_w, nnz_a, t_indptr, t_idx, t_w, nnz_t, eb, kind, mode, combine, nrows,
                                           counts, ws, nbytes, None)

    def sym_fill(a_indptr=p, nnz_a=10, t_indptr=p, nnz_t=10, eb=4, nrows=4, out_indptr=p, out_idx=p, out_w=p, ws=p, nbytes=200):
        return lib.pg_csr_symmetrize_fill(a_indptr, nnz_a, t_indptr, nnz_t, eb, nrows, out_indptr, out_idx, out_w, ws, nbytes, None)

    odd = ctypes.c_void_p(4100)                                             # a workspace that is not 8-byte aligned
    cases = [
        (count, "pg_csr_sort_rows_count", [dict(indptr=None), dict(indices=None), dict(counts=None), dict(ws=None), dict(nrows=-1),
                                           dict(nnz=-1), dict(ncols=-1), dict(nbytes=79), dict(ws=odd), dict(nrows=1 << 31)]),
        (fill, "pg_csr_sort_rows_fill", [dict(indptr=None), dict(w=None), dict(counts=None), dict(out_indptr=None), dict(out_idx=None),
                                         dict(out_w=None), dict(ws=None), dict(eb=0), dict(eb=3), dict(eb=8), dict(nrows=-1),
                                         dict(nnz=-1), dict(nbytes=79)]),
        (hist, "pg_csr_histogram", [dict(indices=None), dict(counts=None), dict(nnz=-1), dict(ncols=-1), dict(ncols=1 << 31)]),
        (transpose, "pg_csr_transpose", [dict(indptr=None), dict(indices=None), dict(w=None), dict(t_indptr=None), dict(t_idx=None),
                                         dict(t_w=None), dict(ws=None), dict(eb=3), dict(eb=-1), dict(nrows=-1), dict(nnz=-1),
                                         dict(ncols=-1), dict(row0=-1), dict(row0=(1 << 31) - 4), dict(nbytes=95), dict(ws=odd)]),
        (sym_count, "pg_csr_symmetrize_count", [dict(a_indptr=None), dict(a_idx=None), dict(a_w=None), dict(t_indptr=None),
                                                dict(t_idx=None), dict(t_w=None), dict(counts=None), dict(ws=None), dict(nnz_a=-1),
                                                dict(nnz_t=-1), dict(nrows=-1), dict(eb=3), dict(eb=1, kind=2), dict(kind=3),
                                                dict(kind=-1), dict(mode=2), dict(mode=-1), dict(combine=2), dict(combine=-1),
                                                dict(nbytes=199), dict(ws=odd)]),
        (sym_fill, "pg_csr_symmetrize_fill", [dict(a_indptr=None), dict(t_indptr=None), dict(out_indptr=None), dict(out_idx=None),
                                              dict(out_w=None), dict(ws=None), dict(nnz_a=-1), dict(nnz_t=-1), dict(nrows=-1),
                                              dict(eb=5), dict(nbytes=199)]),
    ]
    for call, name, bads in cases:
        for bad in bads:
            assert call(**bad) == BAD, (name, bad)
            assert name.encode() in lib.pg_last_error(), (name, bad)
    # nothing to do is no error, and nothing is launched for it
    assert count(nrows=0) == 0 and fill(nrows=0) == 0 and fill(nnz=0, nbytes=8) == 0 and hist(ncols=0) == 0
    assert transpose(nrows=0) == 0 and transpose(nnz=0, nbytes=24) == 0 and sym_count(nrows=0) == 0 and sym_fill(nrows=0) == 0
    assert sym_fill(nnz_a=0, nnz_t=0, nbytes=10) == 0


def test_the_product_has_no_cpu_path_for_the_graph_operations():
    g = CSRGraph(T(np.array([0, 1, 2], np.int64)), T(np.array([1, 0], np.int32)), T(np.array([3, 4], np.uint8)), 2)
    for call in (g.sorted, g.transpose, g.symmetrize):
        with pytest.raises(_native.NativeUnavailable):
            call()
