"""
Substitution-matrix distance without a GPU: the table's validation and helpers, the operator on CPU tensors against the
definition in numpy, the table 1 - I against the reference's Hamming known answers, and the host logic of the graph /
search routes through tests/fake_sub_native.py.
"""
import ctypes
import operator
import os
import re

import numpy as np
import pandas as pd
import pytest
import torch

import fake_sub_native
from conftest import REPO, load_golden
from prograph_amd import synth
from prograph_amd.distance import substitution


def definition(C, X, Y):
    C, X, Y = np.asarray(C, dtype=np.int64), np.atleast_2d(np.asarray(X, dtype=np.intp)), np.atleast_2d(np.asarray(Y, dtype=np.intp))
    w = max(X.shape[1], Y.shape[1])
    X, Y = np.pad(X, ((0, 0), (0, w - X.shape[1]))), np.pad(Y, ((0, 0), (0, w - Y.shape[1])))
    return C[Y[:, None, :], X[None, :, :]].sum(-1)


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


# ---------------------------------------------------------------- the table
def test_table_validation():
    good = table(np.random.default_rng(0), 5, np.arange(1, 256))
    assert substitution(good).symbols == 5 and substitution(good.astype(np.float64)).max_cost == good.max()
    assert substitution(torch.from_numpy(good)).symbols == 5 and substitution(good.tolist()).symbols == 5
    bad = {
        "1-D": good[0], "not square": good[:, :4], "one symbol": np.zeros((1, 1), dtype=int),
        "33 symbols": np.zeros((33, 33), dtype=int), "fraction": good + np.where(np.eye(5), 0, 0.5), "negative": -good,
        "above 255": good * 0 + np.where(np.eye(5), 0, 256), "nan": np.where(np.eye(5), 0, np.nan),
    }
    asym = good.copy()
    asym[1, 2] += 1
    bad["asymmetric"] = asym
    diag = good.copy()
    diag[3, 3] = 1
    bad["diagonal"] = diag
    for what, C in bad.items():
        with pytest.raises(ValueError):
            substitution(C)
            pytest.fail(what)
    assert substitution(np.zeros((32, 32), dtype=int)).symbols == 32 and substitution(np.zeros((2, 2))).symbols == 2
    mine = good.copy()
    dist = substitution(mine)
    mine[0, 1] = mine[1, 0] = 0                                   # the table was copied
    assert np.array_equal(dist.table, good) and dist.table.dtype == np.uint8
    X = torch.tensor([[0, 1]])
    assert int(dist(X, torch.tensor([[1, 0]]))) == 2 * good[0, 1]
    with pytest.raises(ValueError):
        dist.table[0, 1] = 9


def test_from_scores():
    S = np.array([[4, -1, -2, 0], [-1, 5, 0, -3], [-2, 0, 6, 1], [0, -3, 1, 3]])
    dist = substitution.from_scores(S)
    want = np.array([[0, 11, 14, 7], [11, 0, 11, 14], [14, 11, 0, 7], [7, 14, 7, 0]])
    assert np.array_equal(dist.table, want)
    bad = S.copy()
    bad[0, 1] = bad[1, 0] = 5                                     # 4 + 5 - 10 < 0
    with pytest.raises(ValueError):
        substitution.from_scores(bad)
    far = S.copy()
    far[0, 1] = far[1, 0] = -124                                  # 4 + 5 + 248 > 255
    with pytest.raises(ValueError):
        substitution.from_scores(far)
    asym = S.copy()
    asym[0, 1] = 0
    with pytest.raises(ValueError):
        substitution.from_scores(asym)
    with pytest.raises(ValueError):
        substitution.from_scores(S + 0.5)


def test_for_alphabet():
    letters = "WYACD"
    M = np.arange(25).reshape(5, 5)
    M = M + M.T
    out = substitution.for_alphabet(M, letters, "ACD", pad=9)
    assert out.shape == (4, 4) and out[0, 0] == 0 and (out[0, 1:] == 9).all() and (out[1:, 0] == 9).all()
    for i, a in enumerate("ACD", start=1):
        for j, b in enumerate("ACD", start=1):
            assert out[i, j] == M[letters.index(a), letters.index(b)]
    with pytest.raises(ValueError):
        substitution.for_alphabet(M, letters, "ACDE", pad=9)
    np.fill_diagonal(M, 0)
    full = substitution.for_alphabet(M, letters, "ACDWY", pad=3)
    assert substitution(full).symbols == 6


# ---------------------------------------------------------------- the operator on the host
@pytest.mark.parametrize("a", [21, 32])
def test_operator_against_the_definition_on_cpu_tensors(a):
    rng = np.random.default_rng(a)
    C = table(rng, a, np.arange(256))
    dist = substitution(C)
    X, Y = rng.integers(0, a, (40, 50)), rng.integers(0, a, (7, 31))             # unequal widths
    X[3] = 0
    d = dist(torch.from_numpy(X), torch.from_numpy(Y))
    assert d.shape == (7, 40) and d.dtype == torch.int64 and d.device.type == "cpu"
    assert np.array_equal(d.numpy(), definition(C, X, Y))
    wide = dist(torch.from_numpy(Y), torch.from_numpy(X))                        # the first operand is the narrower one
    assert np.array_equal(wide.numpy(), definition(C, Y, X))
    one = dist(torch.from_numpy(X), torch.from_numpy(Y[2]))                      # a 1-D operand
    assert one.shape == (1, 40) and np.array_equal(one.numpy(), definition(C, X, Y[2]))
    for dt in (torch.uint8, torch.int32, torch.float16, torch.float64):
        assert np.array_equal(dist(torch.from_numpy(X).to(dt), torch.from_numpy(Y).to(dt)).numpy(), definition(C, X, Y))
    s = dist(torch.from_numpy(X), torch.from_numpy(Y), similarity=True)
    assert s.dtype == torch.float32 and torch.equal(s, 1 / (1 + d))
    import sys
    mod = sys.modules["prograph_amd.distance.substitution"]      # (the package attribute of that name is the class)
    old = mod._GATHER_ELEMS
    try:
        mod._GATHER_ELEMS = 50 * 9                                 # blocks of the gather do not change the result
        assert np.array_equal(dist(torch.from_numpy(X), torch.from_numpy(Y)).numpy(), definition(C, X, Y))
    finally:
        mod._GATHER_ELEMS = old


def test_operator_errors():
    dist = substitution(1 - np.eye(21, dtype=int))
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


def test_one_minus_identity_is_hamming():
    g = load_golden("hamming_kats")
    dist = substitution(1 - np.eye(32, dtype=int))
    X, Y = torch.Tensor([[1, 2, 3], [4, 5, 6]]), torch.Tensor([[1, 2, 3], [7, 8, 9]])     # the reference's literal answers
    assert np.array_equal(dist(X, Y).numpy(), g["kat_2d2d"])
    assert np.array_equal(dist(X, torch.Tensor([1, 2, 3])).numpy(), g["kat_2d1d"])
    assert np.array_equal(dist(torch.Tensor([4, 5, 6]), torch.Tensor([1, 2, 3])).numpy(), g["kat_1d1d"])
    for i in range(6):                                            # tokens 0..20, unequal widths, up to 200 positions
        got = dist(torch.from_numpy(g[f"r{i}_X"].astype(np.int64)), torch.from_numpy(g[f"r{i}_Y"].astype(np.int64)))
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), g[f"r{i}_out"]), i
    sim = dist(torch.from_numpy(g["r0_X"]), torch.from_numpy(g["r0_Y"]), similarity=True).numpy()
    assert sim.dtype == g["sim_out"].dtype and np.array_equal(sim, g["sim_out"])


# ---------------------------------------------------------------- the boundary
def test_new_symbols_are_declared_and_bound():
    from prograph_amd import _native
    text = open(os.path.join(REPO, "include", "prograph_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("pg_substitution_dense", "pg_sub_pack"):
        assert name in _native.SYMBOLS and re.search(r"\b" + name + r"\s*\(", text)
        assert hasattr(_native.lib(), name)
    assert _native.ABI_VERSION == 3 and _native.lib().pg_version() == 3


def test_new_c_entries_reject_bad_arguments_without_a_launch():
    from prograph_amd import _native
    lib = _native.lib()
    p = ctypes.c_void_p(16)
    bad = lib.pg_last_error
    assert lib.pg_substitution_dense(None, 1, 256, p, 1, 256, 8, p, p, 1, 8, 0, None) == -1        # null pointer
    assert lib.pg_substitution_dense(p, 1, 256, p, 1, 256, 8, None, p, 1, 8, 0, None) == -1        # no table
    assert lib.pg_substitution_dense(p, 1, 256, p, 1, 256, 2049, p, p, 1, 8, 0, None) == -2 and b"2048" in bad()
    assert lib.pg_substitution_dense(p, 1, 256, p, 1, 256, 0, p, p, 1, 8, 0, None) == -1           # no positions
    assert lib.pg_substitution_dense(p, 1, 256, p, 1, 256, 8, p, p, 1, 1, 0, None) == -1 and b"out_elem_bytes" in bad()
    assert lib.pg_substitution_dense(p, 300, 256, p, 1, 256, 8, p, p, 300, 8, 0, None) == -1 and b"npad" in bad()
    assert lib.pg_substitution_dense(p, 9, 256, p, 1, 256, 8, p, p, 8, 8, 0, None) == -1           # ldo < n
    assert lib.pg_sub_pack(p, 1, 8, 8, 33, p, 256, p, None) == -1                                  # 33 symbols
    assert lib.pg_sub_pack(p, 1, 2049, 2049, 21, p, 256, p, None) == -2
    assert lib.pg_sub_pack(p, 1, 8, 7, 21, p, 256, p, None) == -1                                  # ld < l
    assert lib.pg_sub_pack(p, 1, 8, 8, 21, p, 100, p, None) == -1 and b"npad" in bad()


# ---------------------------------------------------------------- host logic through the stand-in
N, L = 300, 32


@pytest.fixture()
def pg(tmp_path, monkeypatch):
    fake_sub_native.install(monkeypatch)
    from prograph_amd import Prograph
    tok = synth.clustered_tokens(N, L, seed=5, members=30)
    tok[7] = tok[8]
    f = tmp_path / "sub.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    del fake_sub_native.calls[:]
    return P, tok


def _names():
    return [c[0] for c in fake_sub_native.calls]


def _arrays(got):
    return np.array([i for i, _ in got]), np.array([w for _, w in got])


def test_graph_routes(pg):
    from prograph_amd import _native
    P, tok = pg
    rng = np.random.default_rng(3)
    C = table(rng, 21, 8 * np.arange(1, 9))
    assert C.max() == 64 and L * C.max() == 2048                  # the bound itself is native
    dist = substitution(C)
    D = definition(C, tok, tok)
    G = P.build_graph(k=5, distance=dist, output="csr")
    assert fake_sub_native.calls == [("operand", N, L, 21), ("dense", N, 2), ("f16_knn", 5, 1, False)]
    wi, wd = knn_of(D, 5, 1)
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.first == 1
    assert np.array_equal(G.idx.numpy(), wi) and np.array_equal(G.dist.numpy(), wd)
    gi, gw = _arrays(P.build_graph(k=5, distance=dist))
    assert gi.dtype == np.int64 and gw.dtype == np.int64 and np.array_equal(gi, wi) and np.array_equal(gw, wd)
    gi, gw = _arrays(P.build_graph(k=5, distance=dist, similarity=True))
    assert gw.dtype == np.float32 and np.array_equal(gi, wi) and np.array_equal(gw, (1 / (1 + torch.from_numpy(wd))).numpy())
    # every ordering: the integer threshold, d = 0 excluded, no keep_zero
    for name, comp, eps, thr in (("le", operator.le, 96, 96.0), ("lt", operator.lt, 96.5, 97.0), ("eq", operator.eq, 64, 64.0),
                                 ("ge", operator.ge, 900.5, 901.0), ("gt", operator.gt, 900, 900.0), ("eq", operator.eq, 64.5, -1.0)):
        del fake_sub_native.calls[:]
        G = P.build_graph(eps=eps, distance=dist, comp=comp, output="csr")
        assert fake_sub_native.calls[-1] == ("f16_eps", _native.CMP_LE if name == "le" else getattr(_native, "CMP_" + name.upper()),
                                             thr, False, False), fake_sub_native.calls
        ip, ix, w = csr_of(D, comp, eps)
        assert G.weights.dtype == torch.int16 and G.indices.dtype == torch.int32 and G.indptr.dtype == torch.int64
        assert np.array_equal(G.indptr.numpy(), ip) and np.array_equal(G.indices.numpy(), ix) and np.array_equal(G.weights.numpy(), w)
    sub = np.arange(50, 120)
    del fake_sub_native.calls[:]
    got = P.build_graph(eps=96, distance=dist, idxs=sub)
    assert fake_sub_native.calls[:2] == [("operand", 70, L, 21), ("dense", 70, 2)]
    ip, ix, w = csr_of(D[np.ix_(sub, sub)], operator.le, 96)
    assert ip[-1] > 0
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
        assert not len(gi) or (gi.dtype == np.int64 and gw.dtype == np.int64)
    # an equal table in another instance takes the same route
    del fake_sub_native.calls[:]
    P.build_graph(k=2, distance=substitution(C.copy()))
    assert "dense" in _names()
    # k beyond n - 1 is clamped; one row asks for nothing
    gi, gw = _arrays(P.build_graph(k=N + 5, distance=dist))
    assert gi.shape == (N, N - 1)
    with pytest.raises(ValueError):
        P.build_graph(k=3, eps=3, distance=dist)


def test_routes_outside_the_native_conditions_take_the_generic_loop(pg):
    from prograph_amd import _native
    P, tok = pg
    rng = np.random.default_rng(4)
    C = table(rng, 21, 8 * np.arange(1, 9))
    over = C.copy()
    over[1, 2] = over[2, 1] = 65                                  # 32 * 65 = 2080 > 2048
    sub = np.arange(40)

    def generic(**kw):
        del fake_sub_native.calls[:]
        got = P.build_graph(idxs=sub, **kw)
        assert not fake_sub_native.calls, fake_sub_native.calls
        return got

    D = definition(over, tok[sub], tok[sub])
    gi, gw = _arrays(generic(k=3, distance=substitution(over)))
    wi, wd = knn_of(D, 3, 1)
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd) and gw.dtype == np.int64
    D = definition(C, tok[sub], tok[sub])
    got = generic(eps=100, distance=substitution(C), comp=lambda d, e: d <= e)        # a comp outside the five orderings
    ip, ix, w = csr_of(D, operator.le, 100)
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    assert _native.MAX_K_ROUNDS == 1023
    # 683 positions at cost 3 = 2049: generic; 512 positions at cost 4 = 2048: native
    wide = rng.integers(1, 21, (12, 683))
    P.graph["W683"] = list(wide)[:1] * (len(P) - 12) + list(wide)
    P.graph["W512"] = list(wide[:, :512])[:1] * (len(P) - 12) + list(wide[:, :512])
    rows = np.arange(len(P) - 12, len(P))
    c3, c4 = table(rng, 21, [1, 2, 3]), table(rng, 21, [1, 2, 3, 4])
    assert 683 * c3.max() == 2049 and 512 * c4.max() == 2048
    del fake_sub_native.calls[:]
    gi, gw = _arrays(P.build_graph(k=3, distance=substitution(c3), representation="W683", idxs=rows))
    wi, wd = knn_of(definition(c3, wide, wide), 3, 1)
    assert not fake_sub_native.calls and np.array_equal(gi, wi) and np.array_equal(gw, wd)
    gi, gw = _arrays(P.build_graph(k=3, distance=substitution(c4), representation="W512", idxs=rows))
    wi, wd = knn_of(definition(c4, wide[:, :512], wide[:, :512]), 3, 1)
    assert _names() == ["operand", "dense", "f16_knn"] and np.array_equal(gi, wi) and np.array_equal(gw, wd)
    # tokens outside the table: the generic loop, where the operator refuses them
    small = substitution(table(rng, 12, [1, 2]))
    del fake_sub_native.calls[:]
    with pytest.raises(ValueError):
        P.build_graph(k=3, distance=small, idxs=sub)
    assert not fake_sub_native.calls
    # a representation that is not integer tokens
    P.graph["F"] = list(tok.astype(np.float64))
    del fake_sub_native.calls[:]
    gi, gw = _arrays(P.build_graph(k=2, distance=substitution(C), representation="F", idxs=sub))
    wi, wd = knn_of(D, 2, 1)
    assert not fake_sub_native.calls and np.array_equal(gi, wi) and np.array_equal(gw, wd)


def test_block_rows(pg, monkeypatch):
    P, tok = pg
    dist = substitution(table(np.random.default_rng(6), 21, 8 * np.arange(1, 9)))
    monkeypatch.setattr(type(P), "_BLOCK_ELEMS", N * 3)
    P.build_graph(k=4, distance=dist)
    assert [c[1] for c in fake_sub_native.calls if c[0] == "dense"] == [64, 64, 64, 64, 44]      # never below 64 rows
    del fake_sub_native.calls[:]
    P.search(tok[:7], k=4, distance=dist)
    assert [c[1] for c in fake_sub_native.calls if c[0] == "dense"] == [3, 3, 1]                 # queries: down to one row
    monkeypatch.setattr(type(P), "_BLOCK_ELEMS", N * 100)
    del fake_sub_native.calls[:]
    P.build_graph(eps=50, distance=dist)
    assert [c[1] for c in fake_sub_native.calls if c[0] == "dense"] == [100, 100, 100]
    del fake_sub_native.calls[:]
    P.search(tok[:7], eps=50, distance=dist)
    assert [c[1] for c in fake_sub_native.calls if c[0] == "dense"] == [7]


def test_search_routes(pg):
    from prograph_amd import _native
    P, tok = pg
    rng = np.random.default_rng(7)
    C = table(rng, 21, 8 * np.arange(1, 7))                       # up to 48: queries of up to 42 positions stay native
    dist = substitution(C)
    lut = np.array([""] + list(synth.AMINO))
    rows = tok[[3, 50, 99, 200, 8]].copy()
    rows[0, 4], rows[1, 9] = 0, 0                                 # unknown letters below
    strings = ["".join(lut[r[r > 0]] if i > 1 else np.where(r > 0, lut[r], "X")) for i, r in enumerate(rows)]
    strings[2] = strings[2][:20]
    strings[3] = strings[3] + "ACDEFGHIKL"
    Q = P.tokenize(strings)
    assert Q.shape == (5, 42) and Q[0, 4] == 0 and (Q[2, 20:] == 0).all()
    DQ = definition(C, tok, Q)
    for q in (strings, Q, torch.from_numpy(Q)):
        del fake_sub_native.calls[:]
        gi, gw = _arrays(P.search(q, k=6, distance=dist))
        assert fake_sub_native.calls == [("operand", N, 42, 21), ("operand", 5, 42, 21), ("dense", 5, 2), ("f16_knn", 6, 0, False)]
        wi, wd = knn_of(DQ, 6, 0)
        assert gi.dtype == np.int64 and gw.dtype == np.int64 and np.array_equal(gi, wi) and np.array_equal(gw, wd)
        assert wd[4, 0] == 0 and set(wi[4, :2]) == {7, 8}         # a dataset row: rank 0 kept, ties to the lower index
        for comp, eps, code, thr in ((operator.le, 0, _native.CMP_LE, 0.0), (operator.le, 100, _native.CMP_LE, 100.0),
                                     (operator.ge, 800.5, _native.CMP_GE, 801.0)):
            del fake_sub_native.calls[:]
            got = P.search(q, eps=eps, distance=dist, comp=comp)
            assert fake_sub_native.calls[-1] == ("f16_eps", code, thr, False, True)              # d = 0 kept
            ip, ix, w = csr_of(DQ, comp, eps, keep_zero=True)
            for i, (gi, gw) in enumerate(got):
                assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    assert list(P.search(strings[4], eps=0, distance=dist)[0][0]) == [7, 8]
    del fake_sub_native.calls[:]
    gi, gw = _arrays(P.search(Q, k=N + 9, distance=dist))         # min(k, N) ranks
    assert gi.shape == (5, N) and ("f16_knn", N, 0, False) in fake_sub_native.calls
    G = P.search(Q, k=3, distance=dist, output="csr")
    assert G.first == 0 and G.nrows == 5 and G.ncols == N and G.dist.dtype == torch.int16
    hit, dmin = P.nearest_neighbour(strings[1], distance=dist)
    wi, wd = knn_of(DQ, 1, 0)
    assert list(hit.index) == [int(wi[1, 0])] and dmin == wd[1, 0]
    # 43 positions at cost 48 = 2064: the generic loop, the same answer
    longer = strings[3] + "A"
    del fake_sub_native.calls[:]
    gi, gw = _arrays(P.search(longer, k=4, distance=dist))
    wi, wd = knn_of(definition(C, tok, P.tokenize([longer])), 4, 0)
    assert not fake_sub_native.calls and np.array_equal(gi, wi) and np.array_equal(gw, wd)
    del fake_sub_native.calls[:]
    got = P.search(Q, eps=100, distance=dist, comp=lambda d, e: d <= e)
    assert not fake_sub_native.calls
    ip, ix, w = csr_of(DQ, operator.le, 100, keep_zero=True)
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    with pytest.raises(ValueError):
        P.search(strings, k=2, eps=2, distance=dist)
