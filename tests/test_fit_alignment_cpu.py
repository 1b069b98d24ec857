"""
Fit alignment scores without a GPU: the yardstick of tests/fit_testdata.py against a brute force over the worded
definition, the operator's torch expression against the yardstick, the properties the module text states, the bound of
the 16-bit cells, the host logic of the graph / search routes on the stand-in of tests/fake_fit_native.py (shifted blocks,
unshifted weights), the host traceback against the canonical rule, the C entries' argument checks, and the stand-alone
sanitizer program of tests/capi_fit.  Every comparison is exact.
"""
import ctypes
import operator
import os
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

import fake_aln_native
import fake_fit_native
from conftest import REPO
from fit_testdata import brute_force, canonical, definition, fragments, lengths, rows_of, score_table, seq
from local_testdata import csr_of, knn_of
from prograph_amd import alignments, synth
from prograph_amd.distance import alignment, fit_alignment


@pytest.mark.parametrize("gap,gap_open", [(1, 0), (2, 3), (5, 1), (255, 255)])
def test_the_recurrence_is_the_best_global_score_over_all_substrings(gap, gap_open):
    rng = np.random.default_rng(gap)
    n = 0
    for _ in range(90):
        a = int(rng.integers(2, 6))
        S = score_table(rng, a, -128 if gap == 255 else -5, 127 if gap == 255 else 6)
        lx, ly = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        X, Y = rows_of(rng, a, [lx], 7, low=0), rows_of(rng, a, [ly], 7, low=0)
        want = brute_force(S, gap, gap_open, seq(X[0]), seq(Y[0]))
        assert definition(S, gap, gap_open, X, Y)[0, 0] == want, (S, X, Y)
        n += 1
    assert n == 90


def test_constructor_rules_and_a_score_is_a_similarity():
    S = np.where(np.eye(4, dtype=bool), 3, -2)
    op = fit_alignment(S, 2, gap_open=5)
    assert (op.gap, op.gap_open, op.symbols, op.max_score) == (2, 5, 4, 3) and "fit_alignment" in repr(op)
    for bad in (np.zeros((4, 4)), np.arange(16).reshape(4, 4), np.full((4, 4), 200), np.ones((33, 33)), np.ones((1, 1)), np.ones((2, 3))):
        with pytest.raises(ValueError):
            fit_alignment(bad, 1)
    for gap, gap_open in ((0, 0), (256, 0), (1, -1), (1, 256)):
        with pytest.raises(ValueError):
            fit_alignment(S, gap, gap_open)
    X = torch.tensor([[1, 2, 3, 1]])
    with pytest.raises(ValueError, match="similarity"):
        op(X, X, similarity=False)
    with pytest.raises(ValueError):
        op(X, torch.tensor([[1, 4]]))                             # a token outside the table
    assert int(op(X, X, similarity=True)[0, 0]) == 12


@pytest.mark.parametrize("a,gap,gap_open", [(5, 1, 0), (21, 3, 0), (21, 1, 11), (32, 2, 1), (8, 255, 255)])
def test_operator_against_the_definition_on_cpu_tensors(a, gap, gap_open):
    rng = np.random.default_rng(a + gap)
    S = score_table(rng, a, -9, 7)
    X = rows_of(rng, a, list(range(41)) + [0, 40, 17], 40, low=0)         # lengths 0..40, interior zeros, empty rows
    Y = rows_of(rng, a, [0, 1, 2, 7, 16, 17, 33, 40, 0, 25, 40], 44, low=0)[:, :44]    # unequal widths
    Y[9, :25] = X[40, 10:35]                                      # a fragment of the longest row
    want = definition(S, gap, gap_open, X, Y)
    op = fit_alignment(S, gap, gap_open)
    got = op(torch.from_numpy(X), torch.from_numpy(Y))
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
    assert want.min() < 0 < want.max()
    back = op(torch.from_numpy(Y), torch.from_numpy(X)).numpy()
    assert np.array_equal(back, definition(S, gap, gap_open, Y, X)) and not np.array_equal(back, want.T)      # not symmetric


def test_the_properties_of_the_module_text():
    rng = np.random.default_rng(11)
    S = score_table(rng, 21, -6, 2, diag=[4, 5, 6])               # the diagonal is every row's maximum
    X = rows_of(rng, 21, [40, 33, 0, 12, 25], 40)
    Y = rows_of(rng, 21, [25, 0, 40, 9, 12], 40)
    Y[0, :25] = X[0, 8:33]                                        # a fragment cut from x
    Y[0, 24] = X[0, 32] = 7
    Y[4, :12] = X[3, :12]
    self_score = lambda r: int(S[r[r > 0], r[r > 0]].sum())
    for gap, gap_open in ((1, 0), (2, 7), (255, 255)):
        op = fit_alignment(S, gap, gap_open)
        s = op(torch.from_numpy(X), torch.from_numpy(Y)).numpy()
        lx, ly = lengths(X)[None, :], lengths(Y)[:, None]
        assert (s >= -(gap_open + gap * ly) * (ly > 0)).all() and (s <= np.minimum(lx, ly) * 6).all()       # the range
        assert (s[1] == 0).all()                                  # an empty y: 0 against everything
        assert np.array_equal(s[:, 2], np.where(ly[:, 0] > 0, -(gap_open + gap * ly[:, 0]), 0))             # an empty x: the lower bound
        assert s[0, 0] == self_score(Y[0]) and s[4, 3] == self_score(Y[4])                                  # a fragment: its self score
        own = op(torch.from_numpy(X), torch.from_numpy(X)).numpy()
        assert np.array_equal(np.diag(own), [self_score(r) for r in X])                                     # a sequence against itself
        assert not np.array_equal(own, own.T) and (s < 0).any()
        # the upper bound is attained: 6 a symbol
        Z = np.full((1, 9), 3)
        assert int(fit_alignment(np.where(np.eye(4, dtype=bool), 6, -6), gap, gap_open)(torch.from_numpy(np.full((1, 30), 3)),
                                                                                          torch.from_numpy(Z))[0, 0]) == 54
    # the global distance charges for the whole parent: 15 symbols of x beyond the fragment
    C = np.where(np.eye(21, dtype=bool), 0, 3)
    assert int(alignment(C, 1)(torch.from_numpy(X[:1]), torch.from_numpy(Y[:1]))[0, 0]) == 15


def test_the_bound_of_the_cells():
    """gap_open + width_y * (gap + 2 max(0, max S)) + 255 <= 65 535, for the short kernel as for the long one; at most 2048
    positions a side; the X operand's width does not enter."""
    from prograph_amd import _native
    fits = _native.aln_fit_fits
    assert 255 + 128 * (255 + 2 * 127) + 255 == 65662 and not fits(128, 128, 127, 255, 255) and fits(128, 127, 127, 255, 255)
    assert 255 + 128 * (255 + 2 * 9) + 255 == 35454 and fits(128, 128, 9, 255, 255)
    assert fits(2048, 2048, 11, 1, 11) and 11 + 2048 * 23 + 255 == 47370                  # BLOSUM62 at full width
    assert fits(2048, 2048, 15, 1, 24) and 24 + 2048 * 31 + 255 == 63767 and not fits(2048, 2048, 15, 2, 0)
    assert fits(2048, 2040, 15, 2, 0) and 2040 * 32 + 255 == 65535 and not fits(2048, 2040, 15, 2, 1)
    assert fits(2048, 256, 127, 1, 0) and 256 * 255 + 255 == 65535 and not fits(2048, 257, 127, 1, 0) and not fits(256, 2048, 127, 1, 0)
    assert not fits(2049, 1, 1, 1, 0) and not fits(1, 2049, 1, 1, 0)
    assert fits(16, 16, -3, 1, 0) == fits(16, 16, 0, 1, 0)        # max(0, max S)
    op = fit_alignment(np.where(np.eye(4, dtype=bool), 127, -128), 255, 255)
    assert not op._short_fits(128, 128) and not op._long_fits(128, 128) and op._short_fits(128, 127)
    assert op._select_bias(128) == 255 + 255 * 128 and not op._f16_route(128, 128) and not op._i32_route(128, 128)


# ---------------------------------------------------------------- host logic through the stand-in
N, L = 60, 24


@pytest.fixture()
def pg(tmp_path, monkeypatch):
    fake_fit_native.install(monkeypatch)
    from prograph_amd import Prograph
    tok = fragments(np.random.default_rng(5), 21, N, L, least=1)
    tok[0] = np.random.default_rng(6).integers(1, 21, L)
    f = tmp_path / "fit.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    del fake_aln_native.calls[:]
    return P, tok


def _arrays(got):
    return np.array([i for i, _ in got]), np.array([w for _, w in got])


def _same_csr(got, ip, ix, w):
    assert len(got) == len(ip) - 1
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]]), i


def test_graph_and_search_routes(pg):
    from prograph_amd import _native
    P, tok = pg
    calls = fake_aln_native.calls
    rng = np.random.default_rng(3)
    S = score_table(rng, 21, -4, 1, diag=np.arange(2, 6))
    op = fit_alignment(S, 3, gap_open=2)
    K = 2 + 3 * L
    D = definition(S, 3, 2, tok, tok)
    assert op._select_bias(L) == K and D.min() < -40 and not np.array_equal(D, D.T)
    # every rank there is: most are negative, and they are ranked by the scores themselves
    G = P.build_graph(k=N - 1, distance=op, output="csr")
    assert calls == [("operand", N, L, 21), ("score", 21), ("fit_dense", N, 2, 3, 2, K), ("f16_knn", N - 1, 1, True)]
    wi, wd = knn_of(D, N - 1, 1)
    assert (wd < 0).mean() > 0.3 and (wd > 0).any()
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.first == 1 and G.similarity is False
    assert np.array_equal(G.idx.numpy(), wi) and np.array_equal(G.dist.numpy(), wd)
    for sim in (False, True):                                     # `similarity` is not consulted: the weights are the scores
        gi, gw = _arrays(P.build_graph(k=5, distance=op, similarity=sim))
        assert gw.dtype == np.int64 and np.array_equal(gi, wi[:, :5]) and np.array_equal(gw, wd[:, :5])
    # eps: comp(eps, s) & s > 0 without the diagonal.  The kernels test (value, threshold): the comparator is mirrored, the
    # threshold shifted by K, v = 0 kept (it is s = -K), and s > 0 applied to the CSR afterwards
    mid = int(np.median(D[D > 0]))
    for name, comp, eps, thr in (("ge", operator.le, mid, float(mid + K)), ("gt", operator.lt, mid - 0.5, float(mid - 1 + K)),
                                 ("eq", operator.eq, mid, float(mid + K)), ("le", operator.ge, 3.5, 3.0 + K),
                                 ("lt", operator.gt, 4, 4.0 + K), ("eq", operator.eq, 10.5, -1.0), ("ge", operator.le, -7, float(K - 7)),
                                 ("le", operator.ge, -7, float(K - 7))):
        del calls[:]
        G = P.build_graph(eps=eps, distance=op, comp=comp, output="csr")
        assert calls[:2] == [("operand", N, L, 21), ("fit_dense", N, 2, 3, 2, K)]
        assert calls[-1] == ("f16_eps", getattr(_native, "CMP_" + name.upper()), thr, False, True), calls
        want = np.where(comp(eps, D) & (D > 0) & ~np.eye(N, dtype=bool))      # a plain `where` over the definition
        assert np.array_equal(G.indptr.numpy(), np.concatenate([[0], np.cumsum(np.bincount(want[0], minlength=N))]))
        assert np.array_equal(G.indices.numpy(), want[1]) and np.array_equal(G.weights.numpy(), D[want])
        assert G.weights.dtype == torch.int16 and G.similarity is False and (len(want[0]) > 0 or eps in (10.5, -7))
    _same_csr(P.build_graph(eps=mid, distance=op), *csr_of(D, operator.le, mid, diagonal=False))      # the default comp: s >= eps
    sub = np.arange(20, 60)
    del calls[:]
    got = P.build_graph(eps=mid, distance=op, idxs=sub)
    assert calls[:2] == [("operand", 40, L, 21), ("fit_dense", 40, 2, 3, 2, K)]
    _same_csr(got, *csr_of(D[np.ix_(sub, sub)], operator.le, mid, diagonal=False))
    # search: rank 0 kept; the queries are the whole ones and NARROWER than the dataset: the shift follows their width
    Q = np.zeros((5, 9), dtype=np.int64)
    Q[:, :9] = tok[[0, 3, 6, 9, 12], :9]
    Q[4] = 0                                                      # an empty query: 0 against everything
    DQ = definition(S, 3, 2, tok, Q)
    KQ = 2 + 3 * 9
    del calls[:]
    gi, gw = _arrays(P.search(Q, k=N, distance=op))
    assert calls == [("operand", N, L, 21), ("operand", 5, 9, 21), ("fit_dense", 5, 2, 3, 2, KQ), ("f16_knn", N, 0, True)]
    wi, wd = knn_of(DQ, N, 0)
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd) and wi[0, 0] == 0 and (wd[4] == 0).all() and (wd < 0).any()
    del calls[:]
    for comp, eps in ((operator.le, 5), (operator.lt, 4.5), (operator.eq, 6), (operator.ge, 9), (operator.gt, 9.5)):
        _same_csr(P.search(Q, eps=eps, distance=op, comp=comp), *csr_of(DQ, comp, eps))
    assert calls[-1] == ("f16_eps", _native.CMP_LT, 10.0 + KQ, False, True)
    hit, best = P.nearest_neighbour(synth.tokens_to_strings(tok[3:4, :9])[0], distance=op)
    assert list(hit.index) == [int(wi[1, 0])] and best == wd[1, 0]
    with pytest.raises(ValueError, match="fit_alignment"):
        P.search(np.array([[1, 21]]), k=1, distance=op)           # a token outside the table: no generic loop
    P.build_graph(k=4, distance=op, store="Fit", output="csr")
    assert "Fit" in P.csr_graphs and np.array_equal(P.degree("Fit"), knn_of(D, 4, 1)[1].sum(1).astype(np.float32))
    assert not [c for c in calls if "local" in c[0] or "semiglobal" in c[0]]


def test_routes_at_and_beyond_the_bounds(pg, monkeypatch):
    from prograph_amd import _native
    P, tok = pg
    calls = fake_aln_native.calls
    rng = np.random.default_rng(4)
    rows = np.arange(N - 12, N)
    wide = fragments(rng, 21, 12, 128, least=100)
    over = fragments(rng, 21, 12, 129, least=100)
    over[0] = rng.integers(1, 21, 129)                            # 129 positions in use
    P.graph["W128"] = list(wide[:1]) * (N - 12) + list(wide)
    P.graph["W129"] = list(over[:1]) * (N - 12) + list(over)

    def table(top):
        S = score_table(rng, 21, -5, 2, diag=[3, 4])
        S[3, 3] = top
        return S
    # gap 1 / 0 at 128 positions: K = 128, and 128 + 128 * 15 = 2048 is the last fp16 case; one more a symbol: the int32
    # blocks of the strip-mined kernel, at ANY width inside the cells; 129 positions: the same; outside the cells: torch
    for rep, mat, top, gaps, route in (("W128", wide, 15, (1, 0), "fit_dense"), ("W128", wide, 16, (1, 0), "fit_long_dense"),
                                       ("W129", over, 4, (2, 1), "fit_long_dense"), ("W128", wide, 127, (255, 255), None)):
        S = table(top)
        op = fit_alignment(S, *gaps)
        K = gaps[1] + gaps[0] * mat.shape[1]
        del calls[:]
        gi, gw = _arrays(P.build_graph(k=11, distance=op, representation=rep, idxs=rows))
        assert [c[0] for c in calls if "dense" in c[0]] == ([route] if route else []), (rep, top, calls)
        if route == "fit_dense":
            assert calls[-1] == ("f16_knn", 11, 1, True) and calls[-2][2] == 2 and calls[-2][5] == K
        elif route:
            assert calls[-1] == ("i32_knn", 11, 1, True) and calls[-2][2] == 4 and calls[-2][5] == K and calls[0][0] == "long_operand"
        else:
            assert not calls                                      # the operator's torch blocks, no native call
        D = definition(S, *gaps, mat, mat)
        wi, wd = knn_of(D, 11, 1)
        assert np.array_equal(gi, wi) and np.array_equal(gw, wd) and (wd < 0).any(), (rep, top)
        del calls[:]
        _same_csr(P.build_graph(eps=6, distance=op, representation=rep, idxs=rows), *csr_of(D, operator.le, 6, diagonal=False))
        if route == "fit_long_dense":
            assert calls[-1] == ("i32_eps", _native.CMP_GE, 6 + K, True)
    # the long route switched off: the torch selection, the same answers
    S = table(4)
    op = fit_alignment(S, 2, 1)
    D = definition(S, 2, 1, over, over)
    monkeypatch.setattr(_native, "aln_long_ready", lambda: False)
    del calls[:]
    gi, gw = _arrays(P.build_graph(k=3, distance=op, representation="W129", idxs=rows))
    assert not calls and np.array_equal(gi, knn_of(D, 3, 1)[0]) and np.array_equal(gw, knn_of(D, 3, 1)[1])
    monkeypatch.setattr(_native, "aln_long_ready", lambda: True)
    # a comp outside the five orderings: the torch selection, the same edge set
    got = P.build_graph(eps=5, distance=op, comp=lambda t, s: t <= s, idxs=np.arange(30))
    assert not calls
    _same_csr(got, *csr_of(definition(op.table, 2, 1, tok[:30], tok[:30]), operator.le, 5, diagonal=False))


# ---------------------------------------------------------------- tracebacks on the host
@pytest.mark.parametrize("gap,gap_open", [(1, 0), (2, 5), (4, 1)])
def test_host_trace_is_the_canonical_alignment(gap, gap_open):
    rng = np.random.default_rng(gap)
    S = score_table(rng, 6, -4, 4)
    T = fragments(rng, 6, 60, 30, low=0)
    xi, yi = rng.integers(0, 60, 200), rng.integers(0, 60, 200)
    *fields, ops = alignments.host_trace(alignments.FIT, S, gap, gap_open, T, T, xi, yi)
    D = definition(S, gap, gap_open, T, T)
    for p in range(200):
        want = canonical(S, gap, gap_open, seq(T[xi[p]]), seq(T[yi[p]]))
        assert tuple(int(f[p]) for f in fields) == want[:7], (p, want)
        assert ops[p, :want[5]].tolist() == want[7] and not ops[p, want[5]:].any()
        assert want[0] == D[yi[p], xi[p]] and want[3] == 0 and want[4] == len(seq(T[yi[p]]))
        assert want[5] == (want[2] - want[1]) + want[4] - want[7].count(1)          # every y symbol, the x range once
    op = fit_alignment(S, gap, gap_open)
    A = op.align(torch.from_numpy(T[xi[:20]]), torch.from_numpy(T[yi[:20]]))       # CPU tensors: the host expression
    assert np.array_equal(A.score.numpy(), fields[0][:20]) and np.array_equal(A.ops.numpy(), ops[:20])
    assert alignments._mode_of(op) == alignments.FIT == 3


def test_prograph_align_hands_the_column_in_as_x(pg, monkeypatch):
    from prograph_amd import _native
    P, tok = pg
    monkeypatch.setattr(_native, "aln_long_ready", lambda: False)  # the host expression
    rng = np.random.default_rng(2)
    S = score_table(rng, 21, -4, 1, diag=np.arange(2, 6))
    op = fit_alignment(S, 3, 2)
    D = definition(S, 3, 2, tok, tok)
    r, c = rng.integers(0, N, 30), rng.integers(0, N, 30)
    A = P.align(rows=r, cols=c, distance=op)
    for p in range(30):
        want = canonical(S, 3, 2, seq(tok[c[p]]), seq(tok[r[p]]))
        assert tuple(int(getattr(A, f)[p]) for f in ("score", "x_begin", "x_end", "y_begin", "y_end", "n_ops", "identities")) == want[:7]
        assert int(A.score[p]) == D[r[p], c[p]]                   # the edge (r, c): row r whole within column c
    Q = tok[[3, 9], :9]
    A = P.align(rows=[0, 1, 1], cols=[5, 3, 9], queries=Q, distance=op)
    DQ = definition(S, 3, 2, tok, Q)
    assert [int(s) for s in A.score] == [DQ[0, 5], DQ[1, 3], DQ[1, 9]] and [int(e) for e in A.y_end] == list(lengths(Q)[[0, 1, 1]])


# ---------------------------------------------------------------- the C entries' argument checks
def test_argument_checks_of_the_c_entries_without_a_gpu():
    """The four entries return their PG_E_* before any launch, and the old trace entries go on rejecting mode 3."""
    from prograph_amd import _native
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                      # never dereferenced on the host
    ok = dict(x=p, n=4, xnpad=256, xl=16, y=p, m=3, ynpad=256, yl=16, score=p, gap=2, gap_open=5, bias=0, out=p, ldo=4, ob=8,
              stream=None, ws=p, wsb=1 << 30)

    def short(**kw):
        a = dict(ok, **kw)
        return lib.pg_alignment_fit_dense(a["x"], a["n"], a["xnpad"], a["xl"], a["y"], a["m"], a["ynpad"], a["yl"], a["score"],
                                          a["gap"], a["gap_open"], a["bias"], a["out"], a["ldo"], a["ob"], a["stream"])

    def long(**kw):
        a = dict(ok, **kw)
        return lib.pg_alignment_fit_long_dense(a["x"], a["n"], a["xnpad"], a["xl"], a["y"], a["m"], a["ynpad"], a["yl"],
                                               a["score"], a["gap"], a["gap_open"], a["bias"], a["out"], a["ldo"], a["ob"],
                                               a["ws"], a["wsb"], a["stream"])

    BADARG, TOOLONG = -1, -2
    common = (dict(x=None), dict(y=None), dict(score=None), dict(out=None), dict(n=0), dict(m=0), dict(xl=0), dict(yl=0),
              dict(ldo=3), dict(gap=0), dict(gap=256), dict(gap_open=-1), dict(gap_open=256), dict(xnpad=255), dict(xnpad=3),
              dict(ynpad=2), dict(bias=-1))
    for kw in common + (dict(ob=4),):
        assert short(**kw) == BADARG, kw
        assert b"pg_alignment_fit_dense" in lib.pg_last_error()
    for kw in (dict(xl=129), dict(yl=129)):
        assert short(**kw) == TOOLONG, kw
        assert b"at most 128 positions" in lib.pg_last_error()
    for kw in common + (dict(ob=2), dict(ws=None), dict(wsb=256 * 16 * 4 - 1), dict(xl=300, wsb=256 * 300 * 4 - 1)):
        assert long(**kw) == BADARG, kw
        assert b"pg_alignment_fit_long_dense" in lib.pg_last_error()
    for kw in (dict(xl=2049), dict(yl=2049)):
        assert long(**kw) == TOOLONG, kw
        assert b"at most 2048 positions" in lib.pg_last_error()

    tok = dict(x=p, n=4, xnpad=256, xl=16, y=p, m=3, ynpad=256, yl=16, xi=p, yi=p, np=5, table=p, gap=2, gap_open=5, head=p, ops=p,
               ldo=32, ws=p, wsb=1 << 30, stream=None)
    order = ("x", "n", "xnpad", "xl", "y", "m", "ynpad", "yl", "xi", "yi", "np", "table", "gap", "gap_open", "head", "ops", "ldo", "ws",
             "wsb", "stream")
    for name, top, share in (("pg_alignment_fit_trace", 128, 64 * 16 * 2 * 4), ("pg_alignment_fit_trace_long", 2048, 64 * 16 * 2 * 4 + 64 * 16 * 8)):
        fn = getattr(lib, name)
        call = lambda **kw: fn(*(dict(tok, **kw)[k] for k in order))
        for kw in (dict(x=None), dict(y=None), dict(xi=None), dict(yi=None), dict(table=None), dict(head=None), dict(ops=None),
                   dict(ws=None), dict(n=0), dict(m=0), dict(xl=0), dict(yl=0), dict(np=0), dict(gap=0), dict(gap=256),
                   dict(gap_open=-1), dict(gap_open=256), dict(xnpad=3), dict(ynpad=2), dict(ldo=31), dict(wsb=share - 1)):
            assert call(**kw) == BADARG, (name, kw)
            assert name.encode() + b":" in lib.pg_last_error()
        for kw in (dict(xl=top + 1), dict(yl=top + 1)):
            assert call(**kw) == TOOLONG, (name, kw)
    # mode 3 stays outside the entries that take a mode
    for name in ("pg_alignment_trace", "pg_alignment_trace_long"):
        assert getattr(lib, name)(3, *(tok[k] for k in order)) == BADARG and b"mode must be" in lib.pg_last_error()
    assert lib.pg_version() == 3
    for s in ("pg_alignment_fit_dense", "pg_alignment_fit_long_dense", "pg_alignment_fit_trace", "pg_alignment_fit_trace_long"):
        assert s in _native.SYMBOLS
    with pytest.raises(ValueError):
        _native.alignment_fit_dense(None, None, None, 1, 1, out_bytes=4)
    with pytest.raises(ValueError):
        _native.alignment_fit_long_dense(None, None, None, 1, 1, out_bytes=2)


def test_trace_routines_in_fit_mode_under_the_sanitizers():
    """tests/capi_fit/fit_check.cpp: pg_aln_trace.h's row routine, as one strip and as several, and walk in mode PG_TR_FIT, compiled for
    the host with the address and undefined-behaviour sanitizers, against a brute force over substrings and paths on
    random pairs, strips included, and the hand-made pairs of its header.  Runs on the CPU."""
    capi = os.path.join(REPO, "tests", "capi_fit")
    subprocess.check_call(["make", "-s", "-C", capi])
    out = subprocess.run([os.path.join(capi, "_build", "fit_check")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fit trace OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
