"""
Levenshtein on the GPU, all exact: the operator (`pg_levenshtein_dense` and the torch expression) against the C
oracle's unbanded distance, kNN and epsilon graphs of `build_graph(distance=levenshtein)` against the oracle's lists,
identity of the routes, the Prograph surface, search.  Inputs: tests/lev_testdata.py (set A).
"""
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import lev_testdata as LT
from oracle import c_oracle as C
from oracle import prograph_oracle as O
from prograph_amd import synth
from prograph_amd.distance import levenshtein

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]


@pytest.fixture(scope="module")
def A():
    return LT.set_a()


@pytest.fixture(scope="module")
def pg(A, tmp_path_factory):
    from prograph_amd import Prograph
    f = tmp_path_factory.mktemp("lev") / "set_a.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(A),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(A))}).to_csv(f)
    P = Prograph(file=str(f))                                    # variable-length strings end to end
    assert np.array_equal(P.tokenized, A)
    return P


@pytest.fixture(scope="module")
def matrix(A):
    """The operator's whole (N, N) matrix - itself checked against the oracle in test_operator_*."""
    T = torch.from_numpy(A).cuda()
    return levenshtein(T, T).cpu().numpy()


def _csr(G):
    return G.indptr.cpu().numpy(), G.indices.cpu().numpy(), G.weights.cpu().numpy()


def _same_csr(G, want):
    ip, ix, w = _csr(G)
    assert ip.dtype == np.int64 and ix.dtype == np.int32 and w.dtype == np.uint8
    assert np.array_equal(ip, want[0]) and np.array_equal(ix, want[1]) and np.array_equal(w, want[2])


def _wf(a, b):
    return O.levenshtein_full(a, int((a != 0).sum()), b, int((b != 0).sum()))


def test_operator_on_the_kernel(A):
    X, Y = torch.from_numpy(A).cuda(), torch.from_numpy(A[:200]).cuda()
    d = levenshtein(X, Y)
    assert d.shape == (200, len(A)) and d.dtype == torch.int64 and d.device == X.device
    got = d.cpu().numpy()
    assert np.array_equal(got, LT.pair_matrix(A, A[:200]))
    rng = np.random.default_rng(1)
    for m, n in zip(rng.integers(0, 200, 300), rng.integers(0, len(A), 300)):
        assert got[m, n] == _wf(A[m], A[n])
    # operands of different widths, an all-zero row, the longest possible answer
    Xs = A[:50, :].copy()
    Xs[7] = 0
    Ys = np.zeros((3, 40), dtype=np.uint8)
    Ys[0, :40] = 21
    Ys[1, :17] = A[0, :17]
    d2 = levenshtein(torch.from_numpy(Xs).cuda(), torch.from_numpy(Ys).cuda()).cpu().numpy()
    assert np.array_equal(d2, LT.pair_matrix(Xs, np.pad(Ys, ((0, 0), (0, 88)))))
    assert d2[2, 7] == 0 and d2[0, 7] == 40 and d2[2, 0] == (A[0] != 0).sum()
    full = np.full((2, 128), 5, dtype=np.uint8)
    full[1] = 6
    assert levenshtein(torch.from_numpy(full).cuda(), torch.from_numpy(full).cuda()).cpu().tolist() == [[0, 128], [128, 0]]
    s = levenshtein(X, Y, similarity=True)
    assert s.dtype == torch.float32 and torch.equal(s, 1 / (1 + d))
    assert torch.equal(levenshtein(X.to(torch.float16), Y.to(torch.float16)), d)
    assert torch.equal(levenshtein(X.to(torch.int64), Y[:, :100].to(torch.int64)), levenshtein(X, Y[:, :100].contiguous()))
    for bad in ((X[:0], Y), (X, Y[:0])):
        with pytest.raises(ValueError):
            levenshtein(*bad)
    with pytest.raises(ValueError):
        levenshtein(X.to(torch.float16) + 0.5, Y)


def test_operator_torch_expression_on_the_device(A):
    import sys
    mod = sys.modules["prograph_amd.distance.levenshtein"]
    rng = np.random.default_rng(2)
    X = np.zeros((60, 150), dtype=np.int64)
    for r in X:
        l = int(rng.integers(0, 151))
        r[:l] = rng.integers(1, 201, l)
    X[5, 3] = 0                                                  # interior zero: a symbol
    X[6] = 0
    Y = X[:9, :90].copy()
    Y[1, 10] = 0
    d = levenshtein(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
    assert d.is_cuda and d.dtype == torch.int64
    want = np.array([[O.levenshtein_full(y, (np.nonzero(y)[0].max() + 1) if y.any() else 0,
                                         x, (np.nonzero(x)[0].max() + 1) if x.any() else 0) for x in X] for y in Y])
    assert np.array_equal(d.cpu().numpy(), want)
    # eligible tokens with one interior zero: not the kernel's input, same definition
    Z = A[:40].copy()
    Z[3, 10] = 0
    dz = levenshtein(torch.from_numpy(Z).cuda(), torch.from_numpy(Z[:5]).cuda()).cpu().numpy()
    assert np.array_equal(dz, np.array([[O.levenshtein_full(y, np.nonzero(y)[0].max() + 1, x, np.nonzero(x)[0].max() + 1)
                                         for x in Z] for y in Z[:5]]))
    # kernel == torch expression on eligible inputs
    T = torch.from_numpy(A[:300]).cuda()
    assert torch.equal(levenshtein(T, T[:64]), mod._torch_levenshtein(T, T[:64]))


def test_knn_graph_hybrid_and_beyond_63(A, pg, matrix, monkeypatch):
    from prograph_amd import _native
    want_idx, want_d = C.lev_knn(A, 16, band=128)
    far = want_d[:, 15] > 8
    assert far.sum() >= 10 and (~far).sum() >= 10, "both kinds of rows must be present"
    banded = C.lev_knn(A, 16, band=8)
    assert np.array_equal(banded[0][~far], want_idx[~far]) and np.array_equal(banded[1][~far], want_d[~far])
    seen = []
    real = _native.levenshtein_dense
    monkeypatch.setattr(_native, "levenshtein_dense", lambda xo, yo, **kw: (seen.append((yo.n, kw.get("rows"))), real(xo, yo, **kw))[1])
    G = pg.build_graph(k=16, distance=levenshtein, output="csr")
    assert sum(r[1] - r[0] for _, r in seen) == int(far.sum()) and all(n == int(far.sum()) for n, _ in seen)
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.uint8
    assert np.array_equal(G.idx.cpu().numpy(), want_idx) and np.array_equal(G.dist.cpu().numpy(), want_d)
    monkeypatch.setenv("PG_LEV_ROUTE", "dense")                  # route identity: dense only
    del seen[:]
    G2 = pg.build_graph(k=16, distance=levenshtein, output="csr")
    assert sum(r[1] - r[0] for _, r in seen) == len(A)
    assert torch.equal(G2.idx, G.idx) and torch.equal(G2.dist, G.dist)
    monkeypatch.delenv("PG_LEV_ROUTE")
    tuples = pg.build_graph(k=100, distance=levenshtein)
    wi, wd = LT.knn_from_matrix(matrix, 100, 1)
    assert all(np.array_equal(gi, a) and np.array_equal(gw, b) and gi.dtype == np.int64 and gw.dtype == np.int64
               for (gi, gw), a, b in zip(tuples, wi, wd))


@pytest.mark.parametrize("comp,eps", [("le", 1), ("le", 3), ("le", 8), ("lt", 3), ("eq", 3)])
def test_fused_eps_graph(A, pg, comp, eps, monkeypatch):
    want = LT.csr_from_banded(A, LT.OPS[comp], eps)
    G = pg.build_graph(eps=eps, distance=levenshtein, comp=LT.OPS[comp], output="csr")
    _same_csr(G, want)
    ip, ix, _ = _csr(G)
    assert (np.diff(ip) == 0).any() and all((np.diff(ix[a:b]) > 0).all() for a, b in zip(ip[:-1], ip[1:]))
    if (comp, eps) in (("le", 3), ("le", 8)):
        dup = np.nonzero((LT.pair_matrix(A[:300], A[:300]) == 0).sum(1) > 1)[0]
        assert len(dup) and all(i not in ix[ip[i]:ip[i + 1]] for i in dup)       # d > 0: duplicates are no neighbours
        monkeypatch.setenv("PG_LEV_ROUTE", "dense")              # route identity
        _same_csr(pg.build_graph(eps=eps, distance=levenshtein, comp=LT.OPS[comp], output="csr"), want)
        monkeypatch.delenv("PG_LEV_ROUTE")
        from prograph_amd import _native
        op = _native.lev_operand(torch.from_numpy(A))
        small = _native.levenshtein_eps(op, _native.CMP_LE, eps, cap=16)          # rows outgrow 16 slots: the filter reruns
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(small, want))


def test_eps_graph_dense_route(A, pg, matrix):
    at8 = int(((matrix <= 8) & (matrix > 0)).sum())
    eps = 60
    want = LT.csr_from_matrix(matrix, operator.le, eps)
    assert len(want[1]) > at8, "the threshold must reach beyond the fused graph"
    _same_csr(pg.build_graph(eps=eps, distance=levenshtein, output="csr"), want)
    _same_csr(pg.build_graph(eps=100, distance=levenshtein, comp=operator.ge, output="csr"), LT.csr_from_matrix(matrix, operator.ge, 100))
    empty = pg.build_graph(eps=0.5, distance=levenshtein, output="csr")
    assert empty.nnz == 0 and empty.nrows == len(A)


def test_surface(A, pg, matrix, tmp_path):
    sub = np.arange(100, 400)
    want = LT.csr_from_matrix(matrix[np.ix_(sub, sub)], operator.le, 4)
    got = pg.build_graph(eps=4, distance=levenshtein, idxs=sub)
    assert len(got) == len(sub) and want[0][-1] > 0
    for i, (gi, gw) in enumerate(got):
        a, b = want[0][i], want[0][i + 1]
        assert np.array_equal(gi, want[1][a:b]) and np.array_equal(gw, want[2][a:b])
        assert not len(gi) or (gi.dtype == np.int64 and gw.dtype == np.int64)
    sim = pg.build_graph(eps=4, distance=levenshtein, idxs=sub, similarity=True)
    for (gi, gw), (si, sw) in zip(got, sim):
        assert np.array_equal(gi, si) and (not len(gi) or (sw.dtype == np.float32 and np.array_equal(sw, (1 / (1 + torch.from_numpy(gw))).numpy())))
    ks = pg.build_graph(k=4, distance=levenshtein, similarity=True)
    wi, wd = LT.knn_from_matrix(matrix, 4, 1)
    assert all(np.array_equal(gi, a) and gw.dtype == np.float32 for (gi, gw), a in zip(ks, wi))
    G = pg.build_graph(eps=5, distance=levenshtein, store="L", output="csr")
    assert "L" in pg.csr_graphs and pg._device_graph("L") is not None
    deg, dirichlet, lv = pg.degree("L"), pg.dirichlet("L"), pg.local_variance("L")
    pg.graph["L_host"] = list(pg.graph["L"])                     # same rows, no device graph behind them
    assert pg._device_graph("L_host") is None
    assert np.array_equal(deg, pg.degree("L_host")) and np.isclose(dirichlet, pg.dirichlet("L_host"), rtol=1e-9)
    assert np.allclose(lv, pg.local_variance("L_host"), equal_nan=True)
    from prograph_amd.utils import save
    from prograph_amd import Prograph
    assert save(pg, name="lev_saved", directory=str(tmp_path) + "/", graphs="csr")
    back = Prograph(file=str(tmp_path / "lev_saved.pkl"))
    assert "L" in back.csr_graphs
    _same_csr(back.csr_graphs["L"], _csr(G))
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(back.graph["L"], pg.graph["L"]))


def test_search_and_single_sequence_queries(A, pg):
    rng = np.random.default_rng(11)
    Q = np.zeros((55, 128), dtype=np.uint8)
    for i in range(50):
        r = A[7 * i][A[7 * i] > 0]
        kind = i % 3
        r = np.delete(r, rng.integers(0, len(r), 1 + i % 4)) if kind == 0 else \
            np.insert(r[:120], int(rng.integers(0, 100)), rng.integers(1, 21, 1 + i % 3)) if kind == 1 else r.copy()
        if kind == 2 and i % 2:
            r[int(rng.integers(0, len(r)))] = 1 + (r[0] % 20)
        Q[i, :len(r)] = r
    for i in range(50, 55):
        l = int(rng.integers(30, 129))
        Q[i, :l] = rng.integers(1, 21, l)
    strings = synth.tokens_to_strings(Q)
    assert len(set(map(len, strings))) > 10
    D = levenshtein(torch.from_numpy(A).cuda(), torch.from_numpy(Q).cuda()).cpu().numpy()
    assert np.array_equal(D[::6], LT.pair_matrix(A, Q[::6])) and (D.min(1) == 0).any()
    wi, wd = LT.knn_from_matrix(D, 5, 0)
    for got in (pg.search(strings, k=5, distance=levenshtein), pg.search(Q, k=5, distance=levenshtein)):
        assert all(np.array_equal(gi, a) and np.array_equal(gw, b) and gw.dtype == np.int64 for (gi, gw), a, b in zip(got, wi, wd))
    want = LT.csr_from_matrix(D, operator.le, 4, keep_zero=True)
    got = pg.search(strings, eps=4, distance=levenshtein)
    assert want[0][-1] > 50 and any(len(g[0]) == 0 for g in got) and any(len(g[0]) and g[1].min() == 0 for g in got)
    for i, (gi, gw) in enumerate(got):
        a, b = want[0][i], want[0][i + 1]
        assert np.array_equal(gi, want[1][a:b]) and np.array_equal(gw, want[2][a:b])
    G = pg.search(strings, eps=4, distance=levenshtein, output="csr")
    _same_csr(G, want)
    K = pg.search(strings, k=70, distance=levenshtein, output="csr")
    w70 = LT.knn_from_matrix(D, 70, 0)
    assert K.first == 0 and np.array_equal(K.idx.cpu().numpy(), w70[0]) and np.array_equal(K.dist.cpu().numpy(), w70[1])
    longest = int((A != 0).sum(1).max())
    long_q = "".join(synth.tokens_to_strings(A[:1])[0][:100] + "ACDEFGHIKLMNPQRSTVWYACDEFGHI")[:128]
    assert len(long_q) == 128 and len(long_q) >= longest and long_q not in pg.seq_idxs
    dl = levenshtein(torch.from_numpy(A).cuda(), torch.from_numpy(pg.tokenize(long_q)).cuda()).cpu().numpy()[0]
    rows, dmin = pg.nearest_neighbour(long_q, distance=levenshtein)
    assert list(rows.index) == [int(np.argsort(dl, kind="stable")[0])] and dmin == dl.min()
    hood = pg.neighbourhood(long_q, int(dl.min()) + 2, distance=levenshtein)
    assert list(hood.index) == list(np.nonzero(dl <= dl.min() + 2)[0]) and len(hood) >= 1
    short = synth.tokens_to_strings(A[3:4])[0][:60]
    ds = levenshtein(torch.from_numpy(A).cuda(), torch.from_numpy(pg.tokenize(short)).cuda()).cpu().numpy()[0]
    assert list(pg.neighbourhood(short, int(ds.min()), distance=levenshtein).index) == list(np.nonzero(ds <= ds.min())[0])
