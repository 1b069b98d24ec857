"""
Gapped alignment distance without a GPU: the constructor's validation, the operator's torch expression on CPU tensors
against the definition in numpy (with both identities: (1 - I, 1) is `levenshtein`, a prohibitive gap gives
`substitution`), and the host logic of the graph / search routes through tests/fake_aln_native.py.
"""
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import fake_aln_native
from prograph_amd import synth
from prograph_amd.distance import alignment, levenshtein, substitution


def lengths(T):
    T = np.asarray(T)
    return np.where(T != 0, np.arange(1, T.shape[1] + 1), 0).max(axis=1, initial=0)


def definition(C, gap, X, Y):
    """(M, N) int64: H[len y][len x] of the recurrence, the plain double loop over positions, all (M, N) pairs at once."""
    C, X, Y = np.asarray(C, dtype=np.int64), np.atleast_2d(np.asarray(X, dtype=np.intp)), np.atleast_2d(np.asarray(Y, dtype=np.intp))
    lx, ly = lengths(X), lengths(Y)
    M, N, LX = len(Y), len(X), X.shape[1]
    H = np.empty((LX + 1, M, N), dtype=np.int64)
    H[:] = (np.arange(LX + 1) * gap)[:, None, None]
    at = np.broadcast_to(lx[None, None, :], (1, M, N))
    out = np.take_along_axis(H, at, 0)[0].copy()                  # empty y: len(x) * gap
    for i in range(1, int(ly.max(initial=0)) + 1):
        cy = C[Y[:, i - 1]]
        diag = H[0].copy()
        H[0] = i * gap
        for j in range(1, LX + 1):
            up = H[j].copy()
            H[j] = np.minimum(diag + cy[:, X[:, j - 1]], np.minimum(up, H[j - 1]) + gap)
            diag = up
        done = ly == i
        out[done] = np.take_along_axis(H, at, 0)[0][done]
    return out


def knn_of(D, k, first):
    order = np.argsort(D, axis=1, kind="stable")[:, first:first + k]
    return order, np.take_along_axis(D, order, 1)


def csr_of(D, comp, eps, keep_zero=False):
    keep = comp(D, eps) & ((D >= 0) if keep_zero else (D > 0))
    r, c = np.nonzero(keep)
    return np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64), c, D[r, c]


def table(rng, a, values):
    C = np.triu(rng.choice(np.asarray(values), size=(a, a)), 1)
    return C + C.T


def rows_of(rng, a, lens, width):
    T = np.zeros((len(lens), width), dtype=np.int64)
    for r, l in enumerate(lens):
        T[r, :l] = rng.integers(1, a, l)
    return T


# ---------------------------------------------------------------- the constructor
def test_constructor_validation():
    good = table(np.random.default_rng(0), 5, np.arange(1, 256))
    dist = alignment(good, 7)
    assert dist.symbols == 5 and dist.gap == 7 and dist.max_cost == max(good.max(), 7)
    assert alignment(good, 255).max_cost == 255 and alignment(good, 3.0).gap == 3 and alignment(good, np.int64(9)).gap == 9
    assert alignment(good.astype(np.float64), 1).symbols == 5 and alignment(torch.from_numpy(good), 1).symbols == 5
    asym, diag = good.copy(), good.copy()
    asym[1, 2] += 1
    diag[3, 3] = 1
    bad = {"1-D": good[0], "not square": good[:, :4], "one symbol": np.zeros((1, 1), dtype=int),
           "33 symbols": np.zeros((33, 33), dtype=int), "fraction": good + np.where(np.eye(5), 0, 0.5), "negative": -good,
           "above 255": good * 0 + np.where(np.eye(5), 0, 256), "nan": np.where(np.eye(5), 0, np.nan),
           "asymmetric": asym, "diagonal": diag}
    for what, C in bad.items():                                   # the table rules of `substitution`
        with pytest.raises(ValueError):
            alignment(C, 5)
            pytest.fail(what)
    for gap in (0, 256, -1, 2.5, True, False, np.bool_(True), float("nan"), float("inf"), None, "3"):
        with pytest.raises(ValueError):
            alignment(good, gap)
            pytest.fail(repr(gap))
    mine = good.copy()
    dist = alignment(mine, 2)
    mine[0, 1] = mine[1, 0] = 0                                   # the table was copied
    assert np.array_equal(dist.table, good) and dist.table.dtype == np.uint8
    with pytest.raises(ValueError):
        dist.table[0, 1] = 9
    sub = substitution(good)                                      # a substitution lends its table
    lent = alignment(sub, 4)
    assert np.array_equal(lent.table, sub.table) and lent.gap == 4
    S = np.array([[4, -1, -2, 0], [-1, 5, 0, -3], [-2, 0, 6, 1], [0, -3, 1, 3]])
    assert np.array_equal(alignment(substitution.from_scores(S), 6).table, substitution.from_scores(S).table)
    X, Y = torch.tensor([[1, 2, 3, 4]]), torch.tensor([[1, 3, 4, 0]])
    assert int(lent(X, Y)) == int(alignment(good, 4)(X, Y)) == min(4, int(good[2, 1] + good[3, 2] + good[4, 3] + 4))


# ---------------------------------------------------------------- the operator on the host
@pytest.mark.parametrize("a,gap", [(21, 1), (21, 7), (32, 255), (32, 40)])
def test_operator_against_the_definition_on_cpu_tensors(a, gap):
    rng = np.random.default_rng(100 * a + gap)
    C = table(rng, a, np.arange(256))
    dist = alignment(C, gap)
    X = rows_of(rng, a, rng.integers(0, 41, 40), 40)              # tokens up to a - 1 = 31, lengths 0..40
    Y = rows_of(rng, a, [0, 1, 5, 31, 17, 16, 30], 31)            # unequal widths
    X[3] = 0                                                      # empty rows on both sides
    X[::4, 2], Y[3, 7], Y[4, 0] = 0, 0, 0                         # interior zeros: symbol 0 of the table
    X[5, :] = 0
    X[5, 9] = a - 1                                               # leading zeros count: length 10
    want = definition(C, gap, X, Y)
    d = dist(torch.from_numpy(X), torch.from_numpy(Y))
    assert d.shape == (7, 40) and d.dtype == torch.int64 and d.device.type == "cpu"
    assert np.array_equal(d.numpy(), want)
    assert (want[0] == lengths(X) * gap).all() and want[0, 5] == 10 * gap
    wide = dist(torch.from_numpy(Y), torch.from_numpy(X))         # the first operand is the narrower one: the transpose
    assert np.array_equal(wide.numpy(), want.T)
    one = dist(torch.from_numpy(X), torch.from_numpy(Y[2]))       # a 1-D operand
    assert one.shape == (1, 40) and np.array_equal(one.numpy(), want[2:3])
    padded = dist(torch.from_numpy(np.pad(X, ((0, 0), (0, 9)))), torch.from_numpy(Y))       # padding changes nothing
    assert np.array_equal(padded.numpy(), want)
    for dt in (torch.uint8, torch.int32, torch.float16, torch.float64):
        assert np.array_equal(dist(torch.from_numpy(X).to(dt), torch.from_numpy(Y).to(dt)).numpy(), want)
    s = dist(torch.from_numpy(X), torch.from_numpy(Y), similarity=True)
    assert s.dtype == torch.float32 and torch.equal(s, 1 / (1 + d))
    import sys
    mod = sys.modules["prograph_amd.distance.alignment"]         # (the package attribute of that name is the class)
    old = mod._DP_ELEMS
    try:
        mod._DP_ELEMS = 41 * 9                                     # blocks of the table do not change the result
        assert np.array_equal(dist(torch.from_numpy(X), torch.from_numpy(Y)).numpy(), want)
    finally:
        mod._DP_ELEMS = old
    assert np.array_equal(alignment(C.copy(), gap)(torch.from_numpy(X), torch.from_numpy(Y)).numpy(), want)


def test_operator_errors():
    dist = alignment(1 - np.eye(21, dtype=int), 1)
    with pytest.raises(ValueError):
        dist(torch.zeros((0, 4)), torch.ones((2, 4)))
    with pytest.raises(ValueError):
        dist(torch.ones((2, 4)), torch.zeros((0, 4)))
    with pytest.raises(ValueError):
        dist(torch.tensor([[1.5, 2.0]]), torch.tensor([[1.0, 2.0]]))
    with pytest.raises(ValueError):
        dist(torch.tensor([[1, 300]]), torch.tensor([[1, 2]]))
    with pytest.raises(ValueError):
        dist(torch.tensor([[1, -2]]), torch.tensor([[1, 2]]))
    with pytest.raises(ValueError):
        dist(torch.tensor([[1, 21]]), torch.tensor([[1, 2]]))     # a token outside the table
    with pytest.raises(ValueError):
        dist(torch.tensor([[1, 20]]), torch.tensor([[21, 2]]))
    assert int(dist(torch.tensor([[1, 20]]), torch.tensor([[20, 2]]))) == 2


def test_one_minus_identity_with_gap_one_is_levenshtein():
    tok, _ = synth.clustered_varlen_tokens(170, Lmax=40, Lmin=12, seed=3, members=10)
    X, Y = torch.from_numpy(tok[:120].astype(np.int64)), torch.from_numpy(tok[120:].astype(np.int64))
    for a in (21, 32):
        got = alignment(1 - np.eye(a, dtype=int), 1)(X, Y)
        assert got.shape == (50, 120) and torch.equal(got, levenshtein(X, Y))
    assert np.array_equal(got.numpy(), definition(1 - np.eye(32, dtype=int), 1, tok[:120], tok[120:]))


def test_with_a_prohibitive_gap_it_is_substitution():
    rng = np.random.default_rng(8)
    C = table(rng, 21, np.arange(1, 49))
    X, Y = torch.from_numpy(rng.integers(1, 21, (60, 8))), torch.from_numpy(rng.integers(1, 21, (9, 8)))
    assert 2 * 193 > 8 * C.max()
    assert torch.equal(alignment(C, 193)(X, Y), substitution(C)(X, Y))
    assert not torch.equal(alignment(C, 5)(X, Y), substitution(C)(X, Y))          # with a cheap gap, gaps pay


# ---------------------------------------------------------------- host logic through the stand-in
N, L = 120, 24


@pytest.fixture()
def pg(tmp_path, monkeypatch):
    fake_aln_native.install(monkeypatch)
    from prograph_amd import Prograph
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=16, seed=5, members=12)
    tok = tok.copy()
    tok[7] = tok[8]
    assert lengths(tok).max() == L
    f = tmp_path / "aln.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    del fake_aln_native.calls[:]
    return P, tok


def _names():
    return [c[0] for c in fake_aln_native.calls]


def _arrays(got):
    return np.array([i for i, _ in got]), np.array([w for _, w in got])


def test_graph_routes(pg):
    from prograph_amd import _native
    P, tok = pg
    rng = np.random.default_rng(3)
    C = table(rng, 21, 2 * np.arange(1, 7))
    dist = alignment(C, 5)
    D = definition(C, 5, tok, tok)
    G = P.build_graph(k=5, distance=dist, output="csr")
    assert fake_aln_native.calls == [("operand", N, L, 21), ("dense", N, 2, 5), ("f16_knn", 5, 1, False)]
    wi, wd = knn_of(D, 5, 1)
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.first == 1
    assert np.array_equal(G.idx.numpy(), wi) and np.array_equal(G.dist.numpy(), wd)
    gi, gw = _arrays(P.build_graph(k=5, distance=dist))
    assert gi.dtype == np.int64 and gw.dtype == np.int64 and np.array_equal(gi, wi) and np.array_equal(gw, wd)
    gi, gw = _arrays(P.build_graph(k=5, distance=dist, similarity=True))
    assert gw.dtype == np.float32 and np.array_equal(gi, wi) and np.array_equal(gw, (1 / (1 + torch.from_numpy(wd))).numpy())
    # every ordering: the integer threshold, d = 0 excluded, no keep_zero
    for name, comp, eps, thr in (("le", operator.le, 20, 20.0), ("lt", operator.lt, 20.5, 21.0), ("eq", operator.eq, 10, 10.0),
                                 ("ge", operator.ge, 90.5, 91.0), ("gt", operator.gt, 90, 90.0), ("eq", operator.eq, 10.5, -1.0)):
        del fake_aln_native.calls[:]
        G = P.build_graph(eps=eps, distance=dist, comp=comp, output="csr")
        assert fake_aln_native.calls[-1] == ("f16_eps", getattr(_native, "CMP_" + name.upper()), thr, False, False), fake_aln_native.calls
        ip, ix, w = csr_of(D, comp, eps)
        assert G.weights.dtype == torch.int16 and G.indices.dtype == torch.int32 and G.indptr.dtype == torch.int64
        assert np.array_equal(G.indptr.numpy(), ip) and np.array_equal(G.indices.numpy(), ix) and np.array_equal(G.weights.numpy(), w)
    sub = np.arange(50, 120)
    del fake_aln_native.calls[:]
    got = P.build_graph(eps=20, distance=dist, idxs=sub)
    assert fake_aln_native.calls[:2] == [("operand", 70, L, 21), ("dense", 70, 2, 5)]
    ip, ix, w = csr_of(D[np.ix_(sub, sub)], operator.le, 20)
    assert ip[-1] > 0
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
        assert not len(gi) or (gi.dtype == np.int64 and gw.dtype == np.int64)
    del fake_aln_native.calls[:]
    P.build_graph(k=2, distance=alignment(C.copy(), 5))           # an equal table and gap in another instance
    assert "dense" in _names()
    gi, gw = _arrays(P.build_graph(k=N + 5, distance=dist))       # k beyond n - 1 is clamped
    assert gi.shape == (N, N - 1)
    one = P.build_graph(k=3, distance=dist, idxs=np.array([4]), output="csr")     # one row asks for nothing
    assert one.idx.shape[0] == 1 and one.idx.shape[1] == 0 and one.dist.dtype == torch.int16
    del fake_aln_native.calls[:]
    for k in (0, -1, -70):                                        # k <= 0: refused before anything is staged
        with pytest.raises(ValueError):
            P.build_graph(k=k, distance=dist)
        with pytest.raises(ValueError):
            P.build_graph(k=k, distance=dist, output="csr", idxs=sub)
    with pytest.raises(ValueError):
        P.build_graph(k=3, eps=3, distance=dist)
    assert not fake_aln_native.calls


def test_routes_at_below_and_above_the_bounds(pg):
    P, tok = pg
    rng = np.random.default_rng(4)
    sub = np.arange(30)

    def route(dist, **kw):
        del fake_aln_native.calls[:]
        got = P.build_graph(distance=dist, idxs=sub, **kw)
        return got, bool(fake_aln_native.calls)

    # width 24: 24 * 85 = 2040 native, and no integer cost meets 2048 at this width; 24 * 86 = 2064 generic - by the
    # table and by the gap
    C = table(rng, 21, [1, 2, 3])
    for dist, native in ((alignment(C, 85), True), (alignment(C, 86), False)):
        D = definition(C, dist.gap, tok[sub], tok[sub])
        gi, gw = _arrays(route(dist, k=3)[0])
        assert route(dist, k=3)[1] is native
        wi, wd = knn_of(D, 3, 1)
        assert np.array_equal(gi, wi) and np.array_equal(gw, wd) and gw.dtype == np.int64
    big = C.copy()
    big[1, 2] = big[2, 1] = 86
    assert route(alignment(big, 5), k=3)[1] is False and route(alignment(np.minimum(big, 85), 5), k=3)[1] is True
    # the bound itself: 16 positions at 128 = 2048 native, at 129 generic; 128 positions at 16 native, at 17 generic
    rows = np.arange(N - 12, N)
    narrow, wide = rows_of(rng, 21, rng.integers(1, 17, 12), 16), rows_of(rng, 21, rng.integers(100, 129, 12), 128)
    over = rows_of(rng, 21, rng.integers(100, 130, 12), 129)
    P.graph["W16"] = list(narrow[:1]) * (N - 12) + list(narrow)
    P.graph["W128"] = list(wide[:1]) * (N - 12) + list(wide)
    P.graph["W129"] = list(over[:1]) * (N - 12) + list(over)
    for rep, mat, gap, native in (("W16", narrow, 128, True), ("W16", narrow, 129, False), ("W128", wide, 16, True),
                                  ("W128", wide, 17, False), ("W129", over, 1, False)):
        dist = alignment(C, gap)
        del fake_aln_native.calls[:]
        gi, gw = _arrays(P.build_graph(k=3, distance=dist, representation=rep, idxs=rows))
        assert bool(fake_aln_native.calls) is native, (rep, gap)
        wi, wd = knn_of(definition(C, gap, mat, mat), 3, 1)
        assert np.array_equal(gi, wi) and np.array_equal(gw, wd), (rep, gap)
    # a comp outside the five orderings, tokens outside the table, a representation that is not integer tokens
    dist = alignment(C, 4)
    D = definition(C, 4, tok[sub], tok[sub])
    got, native = route(dist, eps=12, comp=lambda d, e: d <= e)
    assert not native
    ip, ix, w = csr_of(D, operator.le, 12)
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    del fake_aln_native.calls[:]
    with pytest.raises(ValueError):
        P.build_graph(k=3, distance=alignment(table(rng, 12, [1, 2]), 4), idxs=sub)
    assert not fake_aln_native.calls
    P.graph["F"] = list(tok.astype(np.float64))
    del fake_aln_native.calls[:]
    gi, gw = _arrays(P.build_graph(k=2, distance=dist, representation="F", idxs=sub))
    wi, wd = knn_of(D, 2, 1)
    assert not fake_aln_native.calls and np.array_equal(gi, wi) and np.array_equal(gw, wd)


def test_block_rows(pg, monkeypatch):
    P, tok = pg
    dist = alignment(table(np.random.default_rng(6), 21, 2 * np.arange(1, 7)), 5)
    monkeypatch.setattr(type(P), "_BLOCK_ELEMS", N * 3)
    P.build_graph(k=4, distance=dist)
    assert [c[1] for c in fake_aln_native.calls if c[0] == "dense"] == [64, 56]                 # never below 64 rows
    del fake_aln_native.calls[:]
    P.search(tok[:7], k=4, distance=dist)
    assert [c[1] for c in fake_aln_native.calls if c[0] == "dense"] == [3, 3, 1]                # queries: down to one row
    monkeypatch.setattr(type(P), "_BLOCK_ELEMS", N * 100)
    del fake_aln_native.calls[:]
    P.build_graph(eps=12, distance=dist)
    assert [c[1] for c in fake_aln_native.calls if c[0] == "dense"] == [100, 20]
    del fake_aln_native.calls[:]
    P.search(tok[:7], eps=12, distance=dist)
    assert [c[1] for c in fake_aln_native.calls if c[0] == "dense"] == [7]


def test_search_routes(pg):
    from prograph_amd import _native
    P, tok = pg
    rng = np.random.default_rng(7)
    C = table(rng, 21, 2 * np.arange(1, 7))
    dist = alignment(C, 5)
    lut = np.array([""] + list(synth.AMINO))
    rows = tok[[3, 50, 99, 100, 8]].copy()
    rows[0, 4], rows[1, 9] = 0, 0                                 # unknown letters below
    strings = ["".join(np.where(r[:lengths(r[None])[0]] > 0, lut[r[:lengths(r[None])[0]]], "X")) for r in rows]
    strings[2] = strings[2][:11]                                  # shorter than the dataset
    strings[3] = strings[3] + "ACDEFGHIKL"                        # longer than it
    Q = P.tokenize(strings)
    W = Q.shape[1]
    assert W > L and Q[0, 4] == 0 and (Q[2, 11:] == 0).all()
    DQ = definition(C, 5, tok, Q)
    for q in (strings, Q, torch.from_numpy(Q)):
        del fake_aln_native.calls[:]
        gi, gw = _arrays(P.search(q, k=6, distance=dist))
        assert fake_aln_native.calls == [("operand", N, L, 21), ("operand", 5, W, 21), ("dense", 5, 2, 5), ("f16_knn", 6, 0, False)]
        wi, wd = knn_of(DQ, 6, 0)
        assert gi.dtype == np.int64 and gw.dtype == np.int64 and np.array_equal(gi, wi) and np.array_equal(gw, wd)
        assert wd[4, 0] == 0 and set(wi[4, :2]) == {7, 8}         # a dataset row: rank 0 kept, ties to the lower index
        for comp, eps, code, thr in ((operator.le, 0, _native.CMP_LE, 0.0), (operator.le, 20, _native.CMP_LE, 20.0),
                                     (operator.ge, 80.5, _native.CMP_GE, 81.0)):
            del fake_aln_native.calls[:]
            got = P.search(q, eps=eps, distance=dist, comp=comp)
            assert fake_aln_native.calls[-1] == ("f16_eps", code, thr, False, True)              # d = 0 kept
            ip, ix, w = csr_of(DQ, comp, eps, keep_zero=True)
            for i, (gi, gw) in enumerate(got):
                assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    assert list(P.search(strings[4], eps=0, distance=dist)[0][0]) == [7, 8]
    del fake_aln_native.calls[:]
    gi, gw = _arrays(P.search(Q, k=N + 9, distance=dist))         # min(k, N) ranks
    assert gi.shape == (5, N) and ("f16_knn", N, 0, False) in fake_aln_native.calls
    G = P.search(Q, k=3, distance=dist, output="csr")
    assert G.first == 0 and G.nrows == 5 and G.ncols == N and G.dist.dtype == torch.int16
    S = P.search(Q, eps=20, distance=dist, output="csr")
    assert S.weights.dtype == torch.int16 and S.nrows == 5
    hit, dmin = P.nearest_neighbour(strings[1], distance=dist)
    wi, wd = knn_of(DQ, 1, 0)
    assert list(hit.index) == [int(wi[1, 0])] and dmin == wd[1, 0]
    # neighbourhood and calc_neighbours go through search with the instance
    del fake_aln_native.calls[:]
    seq = P("Sequence")[8]
    assert list(P.neighbourhood(seq, 20, distance=dist).index) == list(np.nonzero(definition(C, 5, tok, tok[8:9])[0] <= 20)[0])
    assert "dense" in _names()
    got = P.calc_neighbours(seq, eps=10, distance=dist, comp=operator.le)
    assert np.array_equal(np.sort(np.asarray(got)), np.nonzero(definition(C, 5, tok, tok[8:9])[0] <= 10)[0])
    # a query of 129 letters: beyond the kernel, the generic loop with the operator, the same answer
    long = "ACDEFGHIKLMNPQRSTVWY" * 6 + "ACDEFGHIK"
    del fake_aln_native.calls[:]
    gi, gw = _arrays(P.search(long, k=4, distance=dist))
    wi, wd = knn_of(definition(C, 5, tok, P.tokenize([long])), 4, 0)
    assert len(long) == 129 and not fake_aln_native.calls and np.array_equal(gi, wi) and np.array_equal(gw, wd)
    del fake_aln_native.calls[:]
    got = P.search(Q, eps=20, distance=dist, comp=lambda d, e: d <= e)
    assert not fake_aln_native.calls
    ip, ix, w = csr_of(DQ, operator.le, 20, keep_zero=True)
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    del fake_aln_native.calls[:]
    with pytest.raises(ValueError):
        P.search(strings, k=2, eps=2, distance=dist)
    for q in (strings, Q, torch.from_numpy(Q)):                   # k <= 0: refused before anything is staged
        for k in (0, -1, -70):
            with pytest.raises(ValueError):
                P.search(q, k=k, distance=dist)
            with pytest.raises(ValueError):
                P.search(q, k=k, distance=dist, output="csr")
    assert not fake_aln_native.calls
