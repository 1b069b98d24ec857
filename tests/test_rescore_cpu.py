"""
Filter-and-refine alignment graphs without a GPU (`Prograph.rescore`, `candidates=` / `pool=`).

The host logic on the stand-in of tests/fake_list_native.py: which route scores the edges and which selects (the list
kernel plus the int32 selection at up to 128 positions, inside fit's bound, under the five orderings and k within the
rounds; `align(..., ops=False)` plus torch otherwise), the error cases, the validation of `pool` and `candidates`, and
that the defaults leave `build_graph` and `search` as they were.  Every result is held against tests/rescore_testdata.py
over values from the definitions.  The header and the library's export list are read too.  The kernel itself:
tests/test_alignment_list_gpu.py.
"""
import ctypes
import operator
import os

import numpy as np
import pandas as pd
import pytest
import torch

import fake_aln_native
import fake_list_native
import rescore_testdata as ref
from conftest import REPO
from fake_list_native import value_of
from fake_stats_native import FIT
from trace_testdata import GLOBAL, LOCAL, SEMIGLOBAL
from prograph_amd import _native, synth
from prograph_amd.distance import (alignment, fit_alignment, hamming, local_alignment, profile_alignment,
                                   semiglobal_alignment)
from prograph_amd.graph import CSRGraph, KNNGraph

N, L, A = 24, 20, 21


def _score_table(seed, top=5):
    rng = np.random.default_rng(seed)
    S = rng.integers(-4, 2, (A, A))
    S = np.triu(S) + np.triu(S, 1).T
    S[np.arange(A), np.arange(A)] = rng.integers(2, top + 1, A)
    return S


def _cost_table(seed):
    C = np.random.default_rng(seed).integers(1, 4, (A, A))
    return np.triu(C, 1) + np.triu(C, 1).T


S, C = _score_table(3), _cost_table(4)
OPERATORS = ((alignment(C, 2, gap_open=1), GLOBAL, C, 2, 1), (local_alignment(S, 3, gap_open=2), LOCAL, S, 3, 2),
             (semiglobal_alignment(S, 2), SEMIGLOBAL, S, 2, 0), (fit_alignment(S, 2, gap_open=1), FIT, S, 2, 1))


def _tokens(width):
    """N short sequences, the last one `width` symbols long: the width of the token matrix."""
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=8, seed=5, members=4)
    wide = np.zeros((N, width), dtype=tok.dtype)
    wide[:, :L] = tok
    wide[N - 1] = np.random.default_rng(9).integers(1, A, width)
    return wide


def _prograph(tmp_path, tok):
    from prograph_amd import Prograph
    f = tmp_path / f"rescore_{tok.shape[1]}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P


def _graph(seed, most=6, nrows=N):
    """A small candidate graph; the wide last row has an edge and is a column."""
    indptr, cols = ref.random_csr(np.random.default_rng(seed), nrows, N, most)
    cols[0] = N - 1
    g = CSRGraph(torch.from_numpy(indptr), torch.from_numpy(cols).to(torch.int32), torch.zeros(len(cols), dtype=torch.int32), N)
    return g, indptr, cols


def _values(mode, T, gap, gap_open, rows, tok, indptr, cols):
    r = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return np.array([value_of(mode, T, gap, gap_open, rows[a], tok[b]) for a, b in zip(r, cols)], dtype=np.int64)


def _calls(kind):
    return [c for c in fake_aln_native.calls if c[0] == kind]


@pytest.fixture()
def pg(tmp_path, monkeypatch):
    fake_list_native.install(monkeypatch)
    tok = _tokens(L)
    return _prograph(tmp_path, tok), tok


# ---------------------------------------------------------------- the header and the library
def test_the_entry_is_declared_and_exported():
    text = open(os.path.join(REPO, "include", "prograph_hip.h")).read()
    proto = ("int pg_alignment_list_scores(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, const void *y_packed, "
             "int64_t m, int64_t y_npad, int yl, const int64_t *indptr, const int32_t *indices, const void *table, int gap, "
             "int gap_open, int32_t *scores, void *stream);")
    assert proto in " ".join(text.split())
    assert "pg_alignment_list_scores" in _native.SYMBOLS
    lib = _native.lib()
    assert hasattr(lib, "pg_alignment_list_scores") and lib.pg_version() == 3
    assert len(lib.pg_alignment_list_scores.argtypes) == 16


def test_c_abi_argument_errors_without_gpu():
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                              # never dereferenced: every check is on the host

    def call(mode=0, x=p, n=4, xnpad=256, xl=20, y=p, m=4, ynpad=256, yl=9, indptr=p, indices=p, table=p, gap=1, gap_open=0,
             scores=p):
        return lib.pg_alignment_list_scores(mode, x, n, xnpad, xl, y, m, ynpad, yl, indptr, indices, table, gap, gap_open, scores, None)
    for bad in (dict(mode=4), dict(mode=-1), dict(gap=0), dict(gap=256), dict(gap_open=-1), dict(gap_open=256), dict(x=None),
                dict(y=None), dict(indptr=None), dict(indices=None), dict(table=None), dict(scores=None), dict(n=0), dict(m=0),
                dict(xl=0), dict(yl=0), dict(xnpad=3), dict(xnpad=300), dict(ynpad=3)):
        assert call(**bad) == -1, bad
        assert b"pg_alignment_list_scores" in lib.pg_last_error()
    for mode in (0, 1, 2, 3):
        assert call(mode=mode, xl=129) == -2 and call(mode=mode, yl=129) == -2


# ---------------------------------------------------------------- routes
def _check_all(P, tok, g, indptr, cols, op, mode, T, gap, gap_open, k=3, eps=4, comp=operator.le, **kw):
    """rescore's three forms against the yardstick; returns nothing, asserts everything."""
    rows = kw.pop("rows", tok)
    vals = _values(mode, T, gap, gap_open, rows, tok, indptr, cols)
    score, query = mode != GLOBAL, "queries" in kw
    plain = P.rescore(g, op, **kw)
    assert isinstance(plain, CSRGraph) and plain.weights.dtype == torch.int32 and plain.ncols == N
    ref.csr_equals(plain, (indptr, cols, vals))
    got = P.rescore(g, op, k=k, **kw)
    assert isinstance(got, KNNGraph) and got.dist.dtype == torch.int32 and got.idx.dtype == torch.int32
    ref.knn_equals(got, ref.knn(indptr, cols, vals, k, score), 0 if query else 1)
    keep = (lambda v: (v > 0) & comp(eps, v)) if score else (lambda v: comp(v, eps) & ((v > 0) | query))
    got = P.rescore(g, op, eps=eps, comp=comp, **kw)
    assert isinstance(got, CSRGraph) and got.weights.dtype == torch.int32
    ref.csr_equals(got, ref.eps(indptr, cols, vals, keep))


def test_the_list_kernel_and_the_int32_selection_take_128_positions(tmp_path, monkeypatch):
    fake_list_native.install(monkeypatch)
    tok = _tokens(128)
    P = _prograph(tmp_path, tok)
    g, indptr, cols = _graph(11, most=3)
    for op, mode, T, gap, gap_open in OPERATORS:
        del fake_aln_native.calls[:]
        _check_all(P, tok, g, indptr, cols, op, mode, T, gap, gap_open)
        assert _calls("list_scores") == [("list_scores", mode, N, len(cols), gap, gap_open)] * 3
        assert not _calls("stats") and not _calls("trace") and not _calls("ops_buffer")
        assert [c[1:] for c in _calls("i32_knn")] == [(3, 0, mode != GLOBAL)] and len(_calls("i32_eps")) == 1


@pytest.mark.parametrize("width", [129, 2049])
def test_wider_operands_take_the_scores_of_align(tmp_path, monkeypatch, width):
    fake_list_native.install(monkeypatch)
    tok = _tokens(width)
    P = _prograph(tmp_path, tok)
    g, indptr, cols = _graph(12, most=2)
    # (the strip kernel's stand-in has no fit mode: fit goes the host's way, at 2049)
    for op, mode, T, gap, gap_open in (OPERATORS[:3] if width == 129 else OPERATORS[:2] + OPERATORS[3:]):
        del fake_aln_native.calls[:]
        _check_all(P, tok, g, indptr, cols, op, mode, T, gap, gap_open)
        assert not _calls("list_scores") and not _calls("i32_knn") and not _calls("i32_eps") and not _calls("stats")
        assert bool(_calls("ops_buffer")) == (width == 129)               # the strip kernel's stand-in, or the host expression


def test_fit_outside_its_bound_takes_the_scores_of_align(tmp_path, monkeypatch):
    """128 positions at 255 / 255 / 127: 255 + 128 * (255 + 254) + 255 = 65 662 > 65 535."""
    fake_list_native.install(monkeypatch)
    tok = _tokens(128)
    P = _prograph(tmp_path, tok)
    g, indptr, cols = _graph(13, most=2)
    T = _score_table(6, top=127)
    T[1, 1] = 127
    assert not _native.aln_fit_fits(128, 128, 127, 255, 255) and _native.aln_fit_fits(128, 128, 127, 254, 255)
    for gap, fast in ((255, False), (254, True)):
        del fake_aln_native.calls[:]
        _check_all(P, tok, g, indptr, cols, fit_alignment(T, gap, gap_open=255), FIT, T, gap, 255, eps=1)
        assert bool(_calls("list_scores")) == fast and bool(_calls("stats")) != fast and bool(_calls("i32_knn")) == fast


def test_the_selection_limits_take_the_fallback(pg):
    P, tok = pg
    g, indptr, cols = _graph(14)
    odd = lambda a, b: operator.le(a, b)                                  # noqa: E731 - the same test, not one of the five
    for op, mode, T, gap, gap_open in OPERATORS:
        del fake_aln_native.calls[:]
        vals = _values(mode, T, gap, gap_open, tok, tok, indptr, cols)
        got = P.rescore(g, op, eps=4, comp=odd)
        keep = (lambda v: (v > 0) & (v >= 4)) if mode != GLOBAL else (lambda v: (v <= 4) & (v > 0))
        ref.csr_equals(got, ref.eps(indptr, cols, vals, keep))
        assert not _calls("list_scores") and not _calls("i32_eps") and len(_calls("stats")) == 1
        same = P.rescore(g, op, eps=4)                                    # ... and the device route gives the same graph
        assert _calls("list_scores") and _calls("i32_eps")
        ref.csr_equals(same, (got.indptr.numpy(), got.indices.numpy(), got.weights.numpy()))
        del fake_aln_native.calls[:]
        k = _native.MAX_K_ROUNDS + 1
        got = P.rescore(g, op, k=k)
        ref.knn_equals(got, ref.knn(indptr, cols, vals, k, mode != GLOBAL), 1)
        assert not _calls("list_scores") and not _calls("i32_knn") and len(_calls("stats")) == 1


def test_without_a_device_everything_is_the_fallback(tmp_path, monkeypatch):
    fake_list_native.install(monkeypatch, ready=False, list_ready=False, long_ready=False)
    tok = _tokens(L)
    P = _prograph(tmp_path, tok)
    g, indptr, cols = _graph(15, most=3)
    for op, mode, T, gap, gap_open in OPERATORS:
        del fake_aln_native.calls[:]
        _check_all(P, tok, g, indptr, cols, op, mode, T, gap, gap_open)
        assert not _calls("list_scores") and not _calls("stats") and not _calls("i32_knn")


def test_graph_forms_row0_queries_and_idxs(pg):
    P, tok = pg
    op, mode, T, gap, gap_open = OPERATORS[1]
    g, indptr, cols = _graph(16)
    want = P.rescore(g, op, k=4)
    # a kNN table with unfilled slots, and a tuple list, say the same as the CSR
    width = int(np.diff(indptr).max())
    idx = np.full((N, width), -1, dtype=np.int64)
    for r in range(N):
        idx[r, :indptr[r + 1] - indptr[r]] = cols[indptr[r]:indptr[r + 1]]
    knn = KNNGraph(torch.from_numpy(idx).to(torch.int32), torch.zeros(idx.shape, dtype=torch.int32), N, first=0)
    tuples = [(cols[indptr[r]:indptr[r + 1]], np.zeros(indptr[r + 1] - indptr[r])) for r in range(N)]
    for form in (knn, tuples):
        got = P.rescore(form, op, k=4)
        assert torch.equal(got.idx, want.idx) and torch.equal(got.dist, want.dist)
    assert P.rescore(g, op, k=4, output="tuples")[3][0].tolist() == want.to_tuples()[3][0].tolist()
    P.rescore(g, op, k=4, store="Refined")
    assert torch.equal(P.rescore("Refined", op).indices, want.as_csr().indices[want.as_csr().indices >= 0])
    # row0: rows 5..12 of the same graph
    part = CSRGraph(torch.from_numpy(indptr[5:14] - indptr[5]), torch.from_numpy(cols[indptr[5]:indptr[13]]).to(torch.int32),
                    torch.zeros(int(indptr[13] - indptr[5]), dtype=torch.int32), N, row0=5)
    got = P.rescore(part, op, k=4)
    assert got.row0 == 5 and torch.equal(got.idx, want.idx[5:13]) and torch.equal(got.dist, want.dist[5:13])
    # queries: the rows are the queries (of another width), d = 0 is kept under an eps
    queries = np.ascontiguousarray(tok[::-1][:7, :L - 3])
    gq, ip, cq = _graph(17, nrows=7)
    for o, m, Tm, e, go in OPERATORS:
        _check_all(P, tok, gq, ip, cq, o, m, Tm, e, go, rows=queries, queries=queries)
    # idxs: both ends go through the selection
    sel = np.arange(N)[::-1].copy()
    vals = _values(mode, T, gap, gap_open, tok[sel], tok[sel], indptr, cols)
    ref.knn_equals(P.rescore(g, op, k=4, idxs=sel), ref.knn(indptr, cols, vals, 4, True), 1)


def test_errors(pg):
    P, tok = pg
    g, _, _ = _graph(18)
    op = OPERATORS[1][0]
    with pytest.raises(TypeError):
        P.rescore(g, hamming)
    with pytest.raises(ValueError, match="queries only"):
        P.rescore(g, profile_alignment("local", 1))
    with pytest.raises(ValueError):
        P.rescore(g, op, k=3, eps=2)
    with pytest.raises(TypeError):
        P.rescore(g, op, k=2.5)
    with pytest.raises(ValueError):
        P.rescore(g, op, k=0)
    with pytest.raises(TypeError):
        P.rescore(g, op, eps="1")
    with pytest.raises(TypeError):
        P.rescore(3.5, op)
    beyond = CSRGraph(torch.tensor([0, 1]), torch.tensor([N], dtype=torch.int32), torch.zeros(1, dtype=torch.int32), N)
    with pytest.raises(IndexError):
        P.rescore(beyond, op)
    for call, who in ((lambda **kw: P.build_graph(distance=op, **kw), "build_graph"),
                      (lambda **kw: P.search(tok[:2], distance=op, **kw), "search")):
        with pytest.raises(ValueError, match="pool"):
            call(k=3, candidates=hamming)                                 # a distance needs its pool
        with pytest.raises(ValueError, match="pool"):
            call(k=3, pool=5)                                             # ... and a pool its candidates
        with pytest.raises(ValueError, match="at least k"):
            call(k=6, candidates=hamming, pool=5)
        for pool in (0, _native.MAX_K_ROUNDS + 1):
            with pytest.raises(ValueError, match="pool"):
                call(eps=2, candidates=hamming, pool=pool)
        with pytest.raises(TypeError):
            call(k=3, candidates=hamming, pool=5.0)
        with pytest.raises(ValueError, match="pool"):
            call(k=3, candidates=g, pool=5)                               # a ready graph takes none
        with pytest.raises(ValueError, match="similarity"):
            call(k=3, candidates=hamming, pool=5, similarity=True)
        with pytest.raises(ValueError):
            call(candidates=hamming, pool=5)                              # k or eps
    with pytest.raises(TypeError):
        P.build_graph(distance=hamming, k=3, candidates=hamming, pool=5)
    with pytest.raises(ValueError, match="queries only"):
        P.build_graph(distance=profile_alignment("local", 1), k=3, candidates=hamming, pool=5)


# ---------------------------------------------------------------- candidates= / pool=
def test_the_defaults_leave_build_graph_and_search_alone(pg):
    P, tok = pg
    for op, *_ in OPERATORS:
        for kw in (dict(k=3), dict(eps=3)):
            del fake_aln_native.calls[:]
            a = P.build_graph(distance=op, output="csr", **kw)
            b = P.build_graph(distance=op, output="csr", candidates=None, pool=None, **kw)
            assert not _calls("list_scores") and not _calls("stats")
            for name in (("idx", "dist") if "k" in kw else ("indptr", "indices", "weights")):
                assert torch.equal(getattr(a, name), getattr(b, name)), name
            a = P.search(tok[:3], distance=op, output="csr", **kw)
            b = P.search(tok[:3], distance=op, output="csr", candidates=None, pool=None, **kw)
            assert not _calls("list_scores") and not _calls("stats")
            for name in (("idx", "dist") if "k" in kw else ("indptr", "indices", "weights")):
                assert torch.equal(getattr(a, name), getattr(b, name)), name
    a, b = P.build_graph(k=2), P.build_graph(k=2, candidates=None, pool=None)
    assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def test_candidates_of_a_distance_and_of_a_graph(pg):
    P, tok = pg
    pool = P.build_graph(k=5, distance=hamming, output="csr")
    pidx = pool.idx.numpy().astype(np.int64)
    for op, mode, T, gap, gap_open in OPERATORS:
        score = mode != GLOBAL
        # the pool of a distance: its kNN table without the row itself (a duplicate of lower index may put it there)
        lists = [pidx[r][(pidx[r] >= 0) & (pidx[r] != r)] for r in range(N)]
        indptr = np.concatenate([[0], np.cumsum([len(c) for c in lists])]).astype(np.int64)
        cols = np.concatenate(lists)
        vals = _values(mode, T, gap, gap_open, tok, tok, indptr, cols)
        got = P.build_graph(distance=op, k=3, candidates=hamming, pool=5, output="csr")
        ref.knn_equals(got, ref.knn(indptr, cols, vals, 3, score), 1)
        same = P.build_graph(distance=op, k=3, candidates=pool, output="csr")      # the ready graph says the same
        assert torch.equal(same.idx, got.idx) and torch.equal(same.dist, got.dist)
        tuples = P.build_graph(distance=op, k=3, candidates=hamming, pool=5)
        assert [t[0].tolist() for t in tuples] == [t[0].tolist() for t in got.to_tuples()]
        keep = (lambda v: (v > 0) & (v >= 6)) if score else (lambda v: (v <= 30) & (v > 0))
        got = P.build_graph(distance=op, eps=6 if score else 30, candidates=hamming, pool=5, output="csr")
        ref.csr_equals(got, ref.eps(indptr, cols, vals, keep))
        # every other row as the pool, the row itself among the candidates: it is removed before the selection
        everyone = CSRGraph(torch.arange(0, N * N + 1, N), torch.arange(N, dtype=torch.int32).repeat(N),
                            torch.zeros(N * N, dtype=torch.int32), N)
        others = np.concatenate([np.delete(np.arange(N), r) for r in range(N)])
        ip = np.arange(0, N * (N - 1) + 1, N - 1)
        got = P.build_graph(distance=op, k=4, candidates=everyone, output="csr")
        ref.knn_equals(got, ref.knn(ip, others, _values(mode, T, gap, gap_open, tok, tok, ip, others), 4, score), 1)
        # search: the pool of every query, rank 0 kept (the stand-ins have no Hamming search: an `alignment` finds the pool)
        queries, finder = np.ascontiguousarray(tok[[3, 0, 7]]), OPERATORS[0][0]
        qpool = P.search(queries, k=5, distance=finder, output="csr").idx.numpy().astype(np.int64)
        ip = np.arange(0, 16, 5)
        vals = _values(mode, T, gap, gap_open, queries, tok, ip, qpool.reshape(-1))
        got = P.search(queries, distance=op, k=2, candidates=finder, pool=5, output="csr")
        ref.knn_equals(got, ref.knn(ip, qpool.reshape(-1), vals, 2, score), 0)
        tuples = P.search(queries, distance=op, k=2, candidates=finder, pool=5)
        assert [t[0].tolist() for t in tuples] == [t[0].tolist() for t in got.to_tuples()]


def test_the_identity_cut_runs_on_the_rescored_graph(pg):
    P, tok = pg
    op = OPERATORS[1][0]
    whole = P.build_graph(distance=op, k=3, candidates=hamming, pool=5, output="csr")
    cut = P.build_graph(distance=op, k=3, candidates=hamming, pool=5, output="csr", min_identity=0.8)
    loose = P.build_graph(distance=op, k=3, candidates=hamming, pool=5, output="csr", min_identity=0.0)
    assert isinstance(cut, CSRGraph) and 0 < cut.nnz < loose.nnz == int((whole.idx >= 0).sum())
    ident = P.align(whole, distance=op, ops=False).identity().numpy()
    kept = whole.idx.numpy()[whole.idx.numpy() >= 0][ident >= 0.8]
    assert np.array_equal(cut.indices.numpy(), kept)
