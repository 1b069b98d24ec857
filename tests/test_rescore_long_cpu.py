"""
Filter-and-refine beyond 128 positions without a GPU (`pg_alignment_list_long_scores`, `Prograph.rescore`, `candidates=` /
`pool=`).

The header, the export list and the host-only argument checks of the C entry, then the route on the stand-in of
tests/fake_list_long_native.py: the long list kernel plus the int32 selection at 129..2048 positions inside the mode's own
16-bit bound, under the five orderings and k within the rounds, where `aln_list_long_ready()`; today's routes everywhere
else.  Every result is held against tests/rescore_testdata.py over values from the definitions.  The kernel itself:
tests/test_alignment_list_long_gpu.py.
"""
import ctypes
import operator
import os

import numpy as np
import pandas as pd
import pytest
import torch

import fake_aln_native
import fake_list_long_native
import rescore_testdata as ref
from conftest import REPO
from fake_list_native import value_of
from fake_stats_native import FIT
from trace_testdata import GLOBAL, LOCAL, SEMIGLOBAL
from prograph_amd import _native, synth
from prograph_amd.distance import alignment, fit_alignment, local_alignment, semiglobal_alignment
from prograph_amd.graph import CSRGraph, KNNGraph

N, L, A = 24, 20, 21


def _score_table(seed, top=5):
    rng = np.random.default_rng(seed)
    S = rng.integers(-4, 2, (A, A))
    S = np.triu(S) + np.triu(S, 1).T
    S[np.arange(A), np.arange(A)] = rng.integers(2, top + 1, A)
    return S


def _cost_table(seed, top=3):
    C = np.random.default_rng(seed).integers(1, top + 1, (A, A))
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
    f = tmp_path / f"rescore_long_{tok.shape[1]}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P


def _graph(seed, most=3, nrows=N):
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


# ---------------------------------------------------------------- the header and the library
def test_the_entry_is_declared_and_exported():
    text = open(os.path.join(REPO, "include", "prograph_hip.h")).read()
    proto = ("int pg_alignment_list_long_scores(int mode, const void *x_packed, int64_t n, int64_t x_npad, int xl, "
             "const void *y_packed, int64_t m, int64_t y_npad, int yl, const int64_t *indptr, const int32_t *indices, "
             "const void *table, int gap, int gap_open, int32_t *scores, void *workspace, int64_t workspace_bytes, void *stream);")
    assert proto in " ".join(text.split())
    assert "pg_alignment_list_long_scores" in _native.SYMBOLS
    lib = _native.lib()
    assert hasattr(lib, "pg_alignment_list_long_scores") and lib.pg_version() == 3
    assert len(lib.pg_alignment_list_long_scores.argtypes) == 18
    assert callable(_native.aln_list_long_ready) and callable(_native.alignment_list_long_scores)


def test_c_abi_argument_errors_without_gpu():
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                              # never dereferenced: every check is on the host
    share = lambda xl: 256 * ((xl + 3) // 4 * 4) * 4                      # noqa: E731 - pg_alignment_long_workspace's `one`
    one = ctypes.c_int64(0)
    assert lib.pg_alignment_long_workspace(300, ctypes.byref(one), None) == 0 and one.value == share(300)

    def call(mode=0, x=p, n=4, xnpad=256, xl=300, y=p, m=4, ynpad=256, yl=9, indptr=p, indices=p, table=p, gap=1, gap_open=0,
             scores=p, ws=p, ws_bytes=None):
        return lib.pg_alignment_list_long_scores(mode, x, n, xnpad, xl, y, m, ynpad, yl, indptr, indices, table, gap, gap_open,
                                                 scores, ws, share(min(xl, 2048)) - 1 if ws_bytes is None else ws_bytes, None)
    # every call here fails: the default workspace is one byte short of a share, so no call reaches a launch
    for bad in (dict(mode=4), dict(mode=-1), dict(gap=0), dict(gap=256), dict(gap_open=-1), dict(gap_open=256), dict(x=None),
                dict(y=None), dict(indptr=None), dict(indices=None), dict(table=None), dict(scores=None), dict(n=0), dict(m=0),
                dict(xl=0), dict(yl=0), dict(xnpad=3), dict(xnpad=300), dict(ynpad=3), dict(n=1 << 31, xnpad=1 << 31)):
        assert call(ws_bytes=share(300), **bad) == -1, bad
        assert b"pg_alignment_list_long_scores" in lib.pg_last_error()
    for mode in (0, 1, 2, 3):
        assert call(mode=mode, xl=2049, ws_bytes=1 << 40) == -2 and call(mode=mode, yl=2049, ws_bytes=1 << 40) == -2
        assert b"2048" in lib.pg_last_error()
        assert call(mode=mode, ws=None, ws_bytes=share(300)) == -1
        for xl in (129, 300, 2048):                                       # widths the entry takes, one byte short of a share
            assert call(mode=mode, xl=xl) == -1 and b"workspace" in lib.pg_last_error()
        assert call(mode=mode, ws_bytes=0) == -1 and call(mode=mode, ws_bytes=-5) == -1
    # the short entry still refuses these widths
    assert lib.pg_alignment_list_scores(0, p, 4, 256, 129, p, 4, 256, 9, p, p, p, 1, 0, p, None) == -2


# ---------------------------------------------------------------- routes
@pytest.mark.parametrize("width", [129, 2048])
def test_the_long_list_kernel_and_the_int32_selection_take_129_to_2048_positions(tmp_path, monkeypatch, width):
    fake_list_long_native.install(monkeypatch)
    tok = _tokens(width)
    P = _prograph(tmp_path, tok)
    g, indptr, cols = _graph(11)
    for op, mode, T, gap, gap_open in OPERATORS:
        del fake_aln_native.calls[:]
        _check_all(P, tok, g, indptr, cols, op, mode, T, gap, gap_open)
        assert _calls("list_long_scores") == [("list_long_scores", mode, N, len(cols), gap, gap_open)] * 3
        assert not _calls("list_scores") and not _calls("stats") and not _calls("trace") and not _calls("trace_long")
        assert not _calls("ops_buffer")
        assert [c[1:] for c in _calls("i32_knn")] == [(3, 0, mode != GLOBAL)] and len(_calls("i32_eps")) == 1


def test_2049_positions_do_not_take_the_long_list_kernel(tmp_path, monkeypatch):
    fake_list_long_native.install(monkeypatch)
    tok = _tokens(2049)
    P = _prograph(tmp_path, tok)
    g, indptr, cols = _graph(12, most=2)
    for op, mode, T, gap, gap_open in OPERATORS[:2]:
        del fake_aln_native.calls[:]
        _check_all(P, tok, g, indptr, cols, op, mode, T, gap, gap_open)
        assert not _calls("list_long_scores") and not _calls("list_scores") and not _calls("i32_knn") and not _calls("i32_eps")


def test_128_positions_still_take_the_short_list_kernel(tmp_path, monkeypatch):
    fake_list_long_native.install(monkeypatch)
    tok = _tokens(128)
    P = _prograph(tmp_path, tok)
    g, indptr, cols = _graph(13)
    for op, mode, T, gap, gap_open in OPERATORS:
        del fake_aln_native.calls[:]
        _check_all(P, tok, g, indptr, cols, op, mode, T, gap, gap_open)
        assert _calls("list_scores") == [("list_scores", mode, N, len(cols), gap, gap_open)] * 3
        assert not _calls("list_long_scores")


def test_without_the_long_list_kernel_the_route_is_todays(tmp_path, monkeypatch):
    fake_list_long_native.install(monkeypatch, list_long_ready=False)
    tok = _tokens(129)
    P = _prograph(tmp_path, tok)
    g, indptr, cols = _graph(14, most=2)
    for op, mode, T, gap, gap_open in OPERATORS[:3]:                      # (the strip tracer's stand-in has no fit mode)
        del fake_aln_native.calls[:]
        _check_all(P, tok, g, indptr, cols, op, mode, T, gap, gap_open)
        assert not _calls("list_long_scores") and not _calls("list_scores") and not _calls("i32_knn") and not _calls("i32_eps")
        assert _calls("ops_buffer")                                       # the scores of align(..., ops=False)


def _bound_cases():
    """Per mode (operator just inside its bound, operator one beyond, mode, the two (T, gap, gap_open), width): the sums
    of the `_native.*_fits` predicates at 65 535 or one step below, and one step over."""
    T = _score_table(6, top=127)
    T[1, 1] = 127
    Cw = _cost_table(7, top=253)
    Cw[1, 2] = Cw[2, 1] = 253
    # global, 257 positions: 257 * 253 + 2 * (gap_open + 253) = 65 021 + 514 at gap_open 4
    assert _native.aln_long_fits(257, 253, 253, 4) and not _native.aln_long_fits(257, 253, 253, 5)
    yield (GLOBAL, 257, (alignment(Cw, 253, gap_open=4), Cw, 253, 4), (alignment(Cw, 253, gap_open=5), Cw, 253, 5))
    # local: 514 * 127 + 255 = 65 533, 515 * 127 + 255 = 65 660: the width is what moves
    assert _native.aln_local_long_fits(514, 514, 127) and not _native.aln_local_long_fits(515, 515, 127)
    yield (LOCAL, (514, 515), (local_alignment(T, 3, gap_open=2), T, 3, 2), (local_alignment(T, 3, gap_open=2), T, 3, 2))
    # semi-global: 2 * 257 * 127 + 255 = 65 533, 2 * 258 * 127 + 255 = 65 787
    assert _native.aln_semiglobal_long_fits(257, 257, 127) and not _native.aln_semiglobal_long_fits(258, 258, 127)
    yield (SEMIGLOBAL, (257, 258), (semiglobal_alignment(T, 2), T, 2, 0), (semiglobal_alignment(T, 2), T, 2, 0))
    # fit, 129 positions: gap_open + 129 * (252 + 254) + 255 = 65 529 + gap_open
    assert _native.aln_fit_fits(129, 129, 127, 252, 6) and not _native.aln_fit_fits(129, 129, 127, 252, 7)
    yield (FIT, 129, (fit_alignment(T, 252, gap_open=6), T, 252, 6), (fit_alignment(T, 252, gap_open=7), T, 252, 7))


@pytest.mark.parametrize("case", list(_bound_cases()), ids=("global", "local", "semiglobal", "fit"))
def test_a_bound_violated_by_one_takes_the_fallback(tmp_path, monkeypatch, case):
    mode, width, inside, beyond = case
    # fit: the strip tracer's stand-in has no fit mode, so its fallback is the host's tracer
    fake_list_long_native.install(monkeypatch, long_ready=mode != FIT)
    widths = width if isinstance(width, tuple) else (width, width)
    g, indptr, cols = _graph(15, most=2)
    for w, (op, T, gap, gap_open), fast in zip(widths, (inside, beyond), (True, False)):
        tok = _tokens(w)
        P = _prograph(tmp_path, tok)
        del fake_aln_native.calls[:]
        _check_all(P, tok, g, indptr, cols, op, mode, T, gap, gap_open, eps=1)
        assert bool(_calls("list_long_scores")) == fast and bool(_calls("i32_knn")) == fast == bool(_calls("i32_eps"))
        assert not _calls("list_scores")
        if mode != FIT:
            assert bool(_calls("ops_buffer")) != fast


def test_the_selection_limits_take_the_fallback(tmp_path, monkeypatch):
    fake_list_long_native.install(monkeypatch)
    tok = _tokens(129)
    P = _prograph(tmp_path, tok)
    g, indptr, cols = _graph(16)
    odd = lambda a, b: operator.le(a, b)                                  # noqa: E731 - the same test, not one of the five
    for op, mode, T, gap, gap_open in OPERATORS[:3]:
        del fake_aln_native.calls[:]
        vals = _values(mode, T, gap, gap_open, tok, tok, indptr, cols)
        got = P.rescore(g, op, eps=4, comp=odd)
        keep = (lambda v: (v > 0) & (v >= 4)) if mode != GLOBAL else (lambda v: (v <= 4) & (v > 0))
        ref.csr_equals(got, ref.eps(indptr, cols, vals, keep))
        assert not _calls("list_long_scores") and not _calls("i32_eps") and _calls("ops_buffer")
        same = P.rescore(g, op, eps=4)                                    # ... and the device route gives the same graph
        assert _calls("list_long_scores") and _calls("i32_eps")
        ref.csr_equals(same, (got.indptr.numpy(), got.indices.numpy(), got.weights.numpy()))
        del fake_aln_native.calls[:]
        k = _native.MAX_K_ROUNDS + 1
        got = P.rescore(g, op, k=k)
        ref.knn_equals(got, ref.knn(indptr, cols, vals, k, mode != GLOBAL), 1)
        assert not _calls("list_long_scores") and not _calls("i32_knn") and _calls("ops_buffer")


# ---------------------------------------------------------------- candidates= / pool=
def _same(a, b):
    assert type(a) is type(b)
    for name in (("idx", "dist") if isinstance(a, KNNGraph) else ("indptr", "indices", "weights")):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and torch.equal(x, y), name


def test_candidates_reach_the_long_list_kernel_at_129_positions(tmp_path, monkeypatch):
    fake_list_long_native.install(monkeypatch)
    tok = _tokens(129)
    P = _prograph(tmp_path, tok)
    g, _, _ = _graph(17, most=6)
    queries, finder = np.ascontiguousarray(tok[[3, 0, 7]]), OPERATORS[0][0]
    for op, mode, T, gap, gap_open in OPERATORS[:3]:
        runs = lambda: [P.build_graph(distance=op, k=3, candidates=g, output="csr"),                # noqa: E731
                        P.build_graph(distance=op, eps=4, candidates=g, output="csr"),
                        P.search(queries, distance=op, k=2, candidates=finder, pool=5, output="csr")]
        del fake_aln_native.calls[:]
        fast = runs()
        assert len(_calls("list_long_scores")) == 3 and not _calls("ops_buffer")
        assert _calls("list_long_scores")[2][1:4] == (mode, 3, 15)
        with monkeypatch.context() as m:
            m.setattr(_native, "aln_list_long_ready", lambda: False)
            del fake_aln_native.calls[:]
            slow = runs()
            assert not _calls("list_long_scores") and _calls("ops_buffer")
        for a, b in zip(fast, slow):
            _same(a, b)
        assert (fast[0].idx >= 0).any() and fast[2].idx.shape == (3, 2)
