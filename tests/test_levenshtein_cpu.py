"""
Levenshtein without a GPU: the torch expression of the operator on CPU tensors against the oracle, and the host logic
of `build_graph(distance=levenshtein)` / `search` (route choice, the hybrid kNN merge, containers, dtypes, errors)
through tests/fake_lev_native.py, which answers the native calls from the C oracle.
"""
import ctypes
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import fake_lev_native
import lev_testdata as LT
from oracle import c_oracle as C
from oracle import prograph_oracle as O
from prograph_amd import synth
from prograph_amd.distance import levenshtein, levenshtein_knn   # noqa: F401  (both stay importable)


def _wf(a, b):
    a, b = np.asarray(a), np.asarray(b)
    la = len(a) - int(np.argmax(a[::-1] != 0)) if a.any() else 0
    lb = len(b) - int(np.argmax(b[::-1] != 0)) if b.any() else 0
    return O.levenshtein_full(a, la, b, lb)


def _rows(rng, n, width, hi, lmin=0):
    T = np.zeros((n, width), dtype=np.int64)
    for r in T:
        l = int(rng.integers(lmin, width + 1))
        r[:l] = rng.integers(1, hi + 1, l)
    return T


def test_torch_expression_is_the_definition():
    rng = np.random.default_rng(3)
    X, Y = _rows(rng, 30, 150, 200), _rows(rng, 7, 90, 200)      # tokens up to 200, 150 positions, unequal widths
    X[3, 5] = 0                                                  # an interior zero is a symbol
    X[4] = 0                                                     # the empty sequence
    Y[2] = 0
    d = levenshtein(torch.from_numpy(X), torch.from_numpy(Y))
    assert d.shape == (7, 30) and d.dtype == torch.int64 and d.device.type == "cpu"
    assert np.array_equal(d.numpy(), np.array([[_wf(y, x) for x in X] for y in Y]))
    assert d[2, 4] == 0 and d[2, 0] == (X[0] != 0).sum()         # d(empty, b) = len(b): no cap
    s = levenshtein(torch.from_numpy(X), torch.from_numpy(Y), similarity=True)
    assert s.dtype == torch.float32 and torch.equal(s, 1 / (1 + d))
    # eligible inputs: the expression equals the C oracle's unbanded distance, in any integer-valued dtype
    A = LT.set_a()[:40]
    want = LT.pair_matrix(A, A[:6])
    for dt in (torch.uint8, torch.int64, torch.float16):
        assert np.array_equal(levenshtein(torch.from_numpy(A).to(dt), torch.from_numpy(A[:6]).to(dt)).numpy(), want)
    # blocks of the table do not change the result
    import sys
    mod = sys.modules["prograph_amd.distance.levenshtein"]       # (the package attribute of that name is the function)
    old = mod._DP_ELEMS
    try:
        mod._DP_ELEMS = 129 * 7
        assert np.array_equal(levenshtein(torch.from_numpy(A), torch.from_numpy(A[:6])).numpy(), want)
    finally:
        mod._DP_ELEMS = old


def test_operator_errors():
    with pytest.raises(ValueError):
        levenshtein(torch.zeros((0, 4)), torch.ones((2, 4)))
    with pytest.raises(ValueError):
        levenshtein(torch.ones((2, 4)), torch.zeros((0, 4)))
    with pytest.raises(ValueError):
        levenshtein(torch.tensor([[1.5, 2.0]]), torch.tensor([[1.0, 2.0]]))
    with pytest.raises(ValueError):
        levenshtein(torch.tensor([[1, 300]]), torch.tensor([[1, 2]]))
    with pytest.raises(ValueError):
        levenshtein(torch.tensor([[1, -2]]), torch.tensor([[1, 2]]))


def test_new_c_entries_reject_bad_arguments_without_a_launch():
    from prograph_amd import _native
    lib = _native.lib()
    p = ctypes.c_void_p(16)
    bad = _native.lib().pg_last_error
    assert lib.pg_levenshtein_dense(None, 1, 256, p, p, 1, 256, p, 128, p, 8, 1, None) == -1          # null pointer
    assert lib.pg_levenshtein_dense(p, 1, 256, p, p, 1, 256, p, 129, p, 8, 1, None) == -1 and b"1..128" in bad()
    assert lib.pg_levenshtein_dense(p, 1, 256, p, p, 1, 256, p, 128, p, 4, 1, None) == -1             # int32 output: no
    assert lib.pg_lev_eps_pairs(p, 1, 128, 128, p, 256, p, 9, 64, p, p, p, p, p, None) == -1 and b"0..8" in bad()
    assert lib.pg_lev_eps_pairs(p, 1, 129, 129, p, 256, p, 8, 64, p, p, p, p, p, None) == -1          # width 129
    assert lib.pg_lev_eps_pairs(p, 1, 128, 128, p, 256, p, 8, 64, p, p, None, p, p, None) == -1       # no mirror table
    assert lib.pg_lev_eps_count(1, 64, 0, 9, p, p, p, p, None) == -1                                  # threshold 9
    assert lib.pg_lev_eps_count(1, 64, 3, 3, p, p, p, p, None) == -1                                  # `ge` is not fused
    assert lib.pg_lev_eps_fill(1, 64, 0, 3, p, p, p, p, None, p, p, None) == -1                       # null indptr


# ---------------------------------------------------------------- host logic through the stand-in
@pytest.fixture()
def pg(tmp_path, monkeypatch):
    fake_lev_native.install(monkeypatch)
    from prograph_amd import Prograph
    tok = LT.set_a()[:300]
    f = tmp_path / "lev.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    return Prograph(file=str(f)), tok


def _same_tuples(got, want_idx, want_w, wdtype=np.int64):
    assert len(got) == len(want_idx)
    for (gi, gw), wi, ww in zip(got, want_idx, want_w):
        assert len(gi) == len(wi)
        if len(wi):
            assert gi.dtype == np.int64 and gw.dtype == wdtype
        assert np.array_equal(gi, wi) and np.array_equal(gw, ww)


def test_hybrid_knn_merges_banded_and_dense_rows(pg):
    P, tok = pg
    k = 8
    want_idx, want_d = C.lev_knn(tok, k, band=128)
    far = want_d[:, k - 1] > 8
    assert 0 < far.sum() < len(tok), "both kinds of rows must be present"
    del fake_lev_native.calls[:]
    got = P.build_graph(k=k, distance=levenshtein)
    _same_tuples(got, want_idx, want_d)
    assert fake_lev_native.calls == [("banded_knn", len(tok)), ("dense", int(far.sum()))]     # only the rows that need it
    sim = P.build_graph(k=k, distance=levenshtein, similarity=True)
    _same_tuples(sim, want_idx, (1 / (1 + torch.from_numpy(want_d.astype(np.int64)))).numpy(), np.float32)
    # beyond 63 ranks every row is dense; the graph is the stable sort of the matrix
    del fake_lev_native.calls[:]
    sub = np.arange(90)
    D = LT.pair_matrix(tok[sub], tok[sub])
    got = P.build_graph(k=70, distance=levenshtein, idxs=sub)
    wi, wd = LT.knn_from_matrix(D, 70, 1)
    _same_tuples(got, wi, wd)
    assert [c[0] for c in fake_lev_native.calls] == ["dense"]
    G = P.build_graph(k=k, distance=levenshtein, output="csr")
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.uint8 and G.first == 1


def test_eps_routes(pg, monkeypatch):
    P, tok = pg
    sub = np.arange(120)
    D = LT.pair_matrix(tok[sub], tok[sub])
    for comp, eps, route in (("le", 3, "eps"), ("lt", 3, "eps"), ("eq", 3, "eps"), ("le", 8.5, "eps"), ("le", 9, "dense"),
                             ("ge", 100, "dense"), ("gt", 3, "dense"), ("le", 0.5, None), ("eq", 2.5, None), ("lt", 1, None)):
        del fake_lev_native.calls[:]
        G = P.build_graph(eps=eps, distance=levenshtein, comp=LT.OPS[comp], idxs=sub, output="csr")
        ip, ix, w = LT.csr_from_matrix(D, LT.OPS[comp], eps)
        assert np.array_equal(G.indptr.numpy(), ip) and np.array_equal(G.indices.numpy(), ix) and np.array_equal(G.weights.numpy(), w), (comp, eps)
        assert G.indices.dtype == torch.int32 and G.weights.dtype == torch.uint8 and G.indptr.dtype == torch.int64
        assert sorted(set(c[0] for c in fake_lev_native.calls)) == ([route] if route else []), (comp, eps, fake_lev_native.calls)
    monkeypatch.setenv("PG_LEV_ROUTE", "dense")
    del fake_lev_native.calls[:]
    G = P.build_graph(eps=3, distance=levenshtein, idxs=sub, output="csr")
    ip, ix, w = LT.csr_from_matrix(D, operator.le, 3)
    assert np.array_equal(G.indices.numpy(), ix) and np.array_equal(G.weights.numpy(), w) and G.weights.dtype == torch.uint8
    assert set(c[0] for c in fake_lev_native.calls) == {"dense"}
    monkeypatch.delenv("PG_LEV_ROUTE")
    tuples = P.build_graph(eps=3, distance=levenshtein, idxs=sub)
    for i, (gi, gw) in enumerate(tuples):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
        assert not len(gi) or (gi.dtype == np.int64 and gw.dtype == np.int64)
    with pytest.raises(ValueError):
        P.build_graph(eps=3, k=3, distance=levenshtein)


def test_ineligible_tokens_take_the_generic_loop_with_the_operator(pg):
    P, tok = pg
    rng = np.random.default_rng(5)
    wide = _rows(rng, 12, 20, 60, lmin=5)                        # tokens above 31
    wide[1] = wide[0]
    P.graph["Wide"] = list(wide)[:1] * (len(P) - 12) + list(wide)
    sub = np.arange(len(P) - 12, len(P))
    del fake_lev_native.calls[:]
    got = P.build_graph(eps=12, distance=levenshtein, representation="Wide", idxs=sub)
    D = np.array([[_wf(a, b) for b in wide] for a in wide])
    ip, ix, w = LT.csr_from_matrix(D, operator.le, 12)
    assert ip[-1] > 0 and not fake_lev_native.calls
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
        assert not len(gi) or gw.dtype == np.int64


def test_search_and_single_sequence_queries(pg):
    P, tok = pg
    rng = np.random.default_rng(11)
    qs = []
    for i in range(12):
        r = tok[i][tok[i] > 0]
        r = np.delete(r, rng.integers(0, len(r), 3)) if i % 2 else np.insert(r[:120], 5, [3, 4, 5])
        qs.append(r)
    qs.append(rng.integers(1, 21, 77))
    qs.append(tok[5][tok[5] > 0])                               # a dataset row: d = 0 is kept
    Q = np.zeros((len(qs), 128), dtype=np.uint8)
    for r, q in zip(Q, qs):
        r[:len(q)] = q
    strings = synth.tokens_to_strings(Q)
    assert len(set(len(s) for s in strings)) > 3
    D = LT.pair_matrix(tok, Q)
    wi, wd = LT.knn_from_matrix(D, 5, 0)
    _same_tuples(P.search(strings, k=5, distance=levenshtein), wi, wd)
    ip, ix, w = LT.csr_from_matrix(D, operator.le, 4, keep_zero=True)
    got = P.search(strings, eps=4, distance=levenshtein)
    assert ip[-1] > len(qs) // 2
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    assert got[-1][1].min() == 0
    G = P.search(Q, k=3, distance=levenshtein, output="csr")
    assert G.first == 0 and G.nrows == len(qs) and G.ncols == len(tok) and G.dist.dtype == torch.uint8
    rows, dmin = P.nearest_neighbour(strings[0], distance=levenshtein)
    assert list(rows.index) == [int(wi[0, 0])] and dmin == wd[0, 0]
    hood = P.neighbourhood(strings[1], 4, distance=levenshtein)
    assert list(hood.index) == list(ix[ip[1]:ip[2]])
    assert np.array_equal(P.calc_neighbours(strings[-1], eps=2, distance=levenshtein, comp=operator.le),
                          np.nonzero(D[-1] <= 2)[0])
    with pytest.raises(ValueError):
        P.search(strings, k=2, eps=2, distance=levenshtein)
