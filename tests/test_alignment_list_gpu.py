"""
The edge-list kernel (`pg_alignment_list_scores`, prograph_amd/csrc/pg_aln_list.h) and what stands on it (`Prograph.rescore`,
`candidates=` / `pool=`) on the GPU.  Every comparison is of integers and exact.

The kernel: 19 Y rows (two row groups and a partial one) against 300 X columns (npad 512), rows and columns of every length
the row routines dispatch on, lists of 0 .. 600 entries with repeated columns, the row's own number and entries that name
no column; every entry against the dense entry's int64 block computed in the same test, a seeded subset against the
suite's Python definitions and `pg_alignment_stats`.  Then guard words, empty lists and the argument checks.
`rescore` against a NumPy selection over the operator's CPU values; `candidates=` with the whole data set as the pool against
the exact graph; the device route against the fallback at 128 positions.
"""
import ctypes
import functools
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import aln_lengths_testdata as ald
import fit_testdata
import rescore_testdata as ref
from long_testdata import rows_of
from prograph_amd import _native, synth
from prograph_amd.distance import alignment, fit_alignment, hamming, local_alignment, semiglobal_alignment
from prograph_amd.graph import CSRGraph, KNNGraph

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

GLOBAL, LOCAL, SEMIGLOBAL, FIT = range(4)
MODES = (GLOBAL, LOCAL, SEMIGLOBAL, FIT)
INT32_MIN = -(1 << 31)
M, N = 19, 300
WIDTHS = ((128, 128), (47, 128), (33, 20), (20, 128))                      # (xl, yl)
Y_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 3, 4, 5, 96, 97, 112)
LIST_LENS = (0, 1, 63, 64, 65, 255, 256, 257, 600, 0, 600, 1, 64, 65, 257, 0, 63, 256, 255)
DEFINITION = dict(zip(MODES, (ald.DEFINITION["global"], ald.DEFINITION["local"], ald.DEFINITION["semiglobal"],
                              fit_testdata.definition)))
DENSE = {GLOBAL: _native.alignment_affine_dense, LOCAL: _native.alignment_local_dense,
         SEMIGLOBAL: _native.alignment_semiglobal_dense, FIT: _native.alignment_fit_dense}


def table(mode):
    return ald.cost(15) if mode == GLOBAL else ald.score()


def device_table(mode, T):
    return _native.sub_cost(T) if mode == GLOBAL else _native.aln_local_score(T)


@functools.lru_cache(maxsize=None)
def problem(xl, yl):
    """(X, Y, indptr, indices): columns of every length 0..xl, rows of the lengths of Y_LENS that fit yl (the rest from
    yl - 3..yl), and per row a list of LIST_LENS entries: random columns (600 of 300: repeats), the row's own number, -1, n and
    n + 5."""
    rng = np.random.default_rng(100 * xl + yl)
    xlens = [c % (xl + 1) for c in range(N)]
    ylens = [l if l <= yl else yl - r % 4 for r, l in enumerate(Y_LENS)]
    assert {0, 1, 15, 16, 17, xl} <= set(xlens) and {0, 1, 15, 16, 17, yl} <= set(ylens)
    X = rows_of(rng, ald.SYMS, [xlens[i] for i in rng.permutation(N)], xl).astype(np.uint8)
    Y = rows_of(rng, ald.SYMS, ylens, yl).astype(np.uint8)
    lists = []
    for r, n in enumerate(LIST_LENS):
        c = rng.integers(0, N, n)
        if n >= 63:
            c[[2, 17, 40, 61, n - 1]] = (r, -1, N, N + 5, -1)
        elif n == 1 and r > 5:
            c[0] = N
        lists.append(c)
    indptr = np.concatenate([[0], np.cumsum(LIST_LENS)]).astype(np.int64)
    return X, Y, indptr, np.concatenate(lists).astype(np.int32)


def operands(X, Y):
    return _native.aln_operand(torch.from_numpy(X), ald.SYMS), _native.aln_operand(torch.from_numpy(Y), ald.SYMS)


def expected(D, indptr, indices):
    """The list's values from a (M, N) block."""
    r = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    ok = (indices >= 0) & (indices < D.shape[1])
    return np.where(ok, D[r, np.where(ok, indices, 0)], INT32_MIN)


@pytest.mark.parametrize("xl,yl", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_every_entry_is_the_dense_entry(mode, xl, yl):
    X, Y, indptr, indices = problem(xl, yl)
    xo, yo = operands(X, Y)
    assert xo.npad == 512
    T = table(mode)
    for gap, gap_open in ald.GAPS:
        assert mode != FIT or _native.aln_fit_fits(xl, yl, int(T.max()), gap, gap_open)
        dense = DENSE[mode](xo, yo, device_table(mode, T), gap, gap_open, out_bytes=8)
        got = _native.alignment_list_scores(xo, yo, indptr, indices, mode, device_table(mode, T), gap, gap_open)
        assert got.dtype == torch.int32 and got.shape == (len(indices),)
        want = expected(dense.cpu().numpy(), indptr, indices)
        assert (want == INT32_MIN).sum() >= 30 and (want != INT32_MIN).sum() > 3000
        bad = np.flatnonzero(got.cpu().numpy() != want)
        assert not len(bad), (bad[:8], got.cpu().numpy()[bad[:8]], want[bad[:8]])
    assert xo.valid() and yo.valid()


@pytest.mark.parametrize("mode", MODES)
def test_a_subset_is_the_definition_and_the_statistics_kernel(mode):
    """19 rows x 10 columns = 190 pairs of the (47, 128) problem, gap 3, gap_open 11."""
    X, Y, _, _ = problem(47, 128)
    cols = np.random.default_rng(7).permutation(N)[:10]
    T = table(mode)
    indptr = np.arange(0, M * 10 + 1, 10, dtype=np.int64)
    indices = np.tile(cols, M).astype(np.int32)
    xo, yo = operands(X, Y)
    got = _native.alignment_list_scores(xo, yo, indptr, indices, mode, device_table(mode, T), 3, 11).cpu().numpy()
    D = DEFINITION[mode](T, 3, 11, X[cols].astype(np.int64), Y.astype(np.int64))      # (M, 10)
    assert np.array_equal(got, D.reshape(-1))
    rows = np.repeat(np.arange(M), 10)
    head = _native.alignment_stats(xo, yo, indices, rows, mode, device_table(mode, T), 3, 11)      # x: the side with the free ends
    assert np.array_equal(got, head[:, 0].cpu().numpy())


def _raw(mode, xo, yo, indptr, indices, T, scores_ptr):
    return _native.lib().pg_alignment_list_scores(mode, _native._ptr(xo.buf), xo.n, xo.npad, xo.l, _native._ptr(yo.buf), yo.n,
                                                  yo.npad, yo.l, _native._ptr(indptr), _native._ptr(indices), _native._ptr(T), 3, 11,
                                                  scores_ptr, _native._stream())


def test_memory_around_the_scores_is_untouched():
    X, Y, indptr, indices = problem(33, 20)
    xo, yo = operands(X, Y)
    dev = xo.buf.device
    ip, ix = torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev)
    nnz, guard, mark = len(indices), 64, 0x5A5A5A5A
    for mode in MODES:
        T = device_table(mode, table(mode))
        buf = torch.full((nnz + 2 * guard,), mark, dtype=torch.int32, device=dev)
        assert _raw(mode, xo, yo, ip, ix, T, ctypes.c_void_p(buf.data_ptr() + 4 * guard)) == 0
        out = buf.cpu().numpy()
        assert (out[:guard] == mark).all() and (out[-guard:] == mark).all()
        want = _native.alignment_list_scores(xo, yo, indptr, indices, mode, T, 3, 11).cpu().numpy()
        assert np.array_equal(out[guard:-guard], want) and (want != mark).all()
        # rows without a list write nothing: every list empty, and all but the last row's
        buf.fill_(mark)
        assert _raw(mode, xo, yo, torch.zeros(M + 1, dtype=torch.int64, device=dev), ix, T, _native._ptr(buf)) == 0
        assert bool((buf == mark).all())
        last = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        last[M] = 3
        assert _raw(mode, xo, yo, last, ix, T, ctypes.c_void_p(buf.data_ptr() + 4 * guard)) == 0
        out = buf.cpu().numpy()
        assert (np.delete(out, np.arange(guard, guard + 3)) == mark).all()
        one = torch.tensor([0] * M + [3])
        assert np.array_equal(out[guard:guard + 3], _native.alignment_list_scores(xo, yo, one, indices[:3], mode, T, 3, 11).cpu().numpy())


def test_argument_errors_return_before_any_launch():
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                              # never dereferenced

    def call(mode=0, x=p, n=4, xnpad=256, xl=20, y=p, m=4, ynpad=256, yl=9, indptr=p, indices=p, table=p, gap=1, gap_open=0,
             scores=p):
        return lib.pg_alignment_list_scores(mode, x, n, xnpad, xl, y, m, ynpad, yl, indptr, indices, table, gap, gap_open, scores,
                                            _native._stream())
    for bad in (dict(x=None), dict(y=None), dict(indptr=None), dict(indices=None), dict(table=None), dict(scores=None),
                dict(mode=4), dict(mode=-1), dict(gap=0), dict(gap=256), dict(gap_open=-1), dict(xnpad=3), dict(ynpad=3)):
        assert call(**bad) == -1, bad
    assert call(xl=129) == -2 and call(yl=129) == -2
    torch.cuda.synchronize()


# ---------------------------------------------------------------- rescore against brute force
A4 = 5                                                                      # tokens 1..4 and the padding


def _prograph(tmp_path, tok, name):
    from prograph_amd import Prograph
    f = tmp_path / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P


def _tables(a):
    rng = np.random.default_rng(21)
    C = np.triu(rng.integers(1, 3, (a, a)), 1)
    S = np.triu(rng.integers(-2, 1, (a, a)), 1)
    S = S + S.T
    S[np.arange(a), np.arange(a)] = rng.integers(1, 3, a)
    return C + C.T, S


def _operators(a):
    C, S = _tables(a)
    return (alignment(C, 1, gap_open=1), local_alignment(S, 1, gap_open=1), semiglobal_alignment(S, 1),
            fit_alignment(S, 1, gap_open=2))


def _mixed(rng, n, most, symbols, width=None):
    lens = rng.integers(1, most + 1, n)
    lens[0] = most
    return rows_of(rng, symbols + 1, lens, width or most).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def brute():
    """150 sequences of 1..40 symbols out of 4, a candidate graph of 0..70 edges a row, 9 queries at another width, and the
    operators' values on the CPU: D[op][r, c] over the data, Dq[op][q, c] for the queries."""
    rng = np.random.default_rng(31)
    tok = _mixed(rng, 150, 40, 4)
    queries = _mixed(rng, 9, 33, 4)
    short = int(np.flatnonzero((tok > 0).sum(1) <= 33)[0])
    queries[1] = tok[short, :33]                                          # a query that is a data row
    indptr, cols = ref.random_csr(rng, 150, 150, 70)
    qptr, qcols = ref.random_csr(rng, 9, 150, 70, own_row=False)
    if short not in qcols[qptr[1]:qptr[2]]:                               # ... and has it among its 70 candidates
        qcols[qptr[1]] = short
    X, Q = torch.from_numpy(tok), torch.from_numpy(queries)
    ops = _operators(A4)
    D = [op(X, X).numpy() for op in ops]
    Dq = [op(X, Q).numpy() for op in ops]
    return tok, queries, (indptr, cols), (qptr, qcols), ops, D, Dq


@pytest.fixture()
def pg150(tmp_path):
    return _prograph(tmp_path, brute()[0], "brute")


def _graph(indptr, cols, ncols, row0=0):
    return CSRGraph(torch.from_numpy(indptr), torch.from_numpy(cols).to(torch.int32), torch.zeros(len(cols), dtype=torch.int32),
                    ncols, row0=row0)


def _edge_values(D, indptr, cols, rows=None):
    r = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return D[r if rows is None else rows[r], cols]


COMPS = (operator.le, operator.ge, operator.lt, operator.gt, operator.eq)


@pytest.mark.parametrize("which", range(4))
def test_rescore_is_the_brute_force_selection(pg150, which):
    tok, _, (indptr, cols), _, ops, D, _ = brute()
    op, score = ops[which], which != GLOBAL
    vals = _edge_values(D[which], indptr, cols)
    if which == FIT:
        assert (vals < 0).any() and (vals > 0).any()
    assert len(np.unique(vals)) < len(vals) // 4                           # ties are the rule
    g = _graph(indptr, cols, 150)
    plain = pg150.rescore(g, op)
    assert plain.weights.dtype == torch.int32 and plain.weights.is_cuda
    ref.csr_equals(plain, (indptr, cols, vals))
    for k in (1, 5, 64, 70):
        got = pg150.rescore(g, op, k=k)
        assert isinstance(got, KNNGraph) and got.dist.dtype == torch.int32
        ref.knn_equals(got, ref.knn(indptr, cols, vals, k, score), 1)
    thr = int(np.median(vals[vals > 0]))
    for comp in COMPS:
        got = pg150.rescore(g, op, eps=thr, comp=comp)
        keep = (lambda v: (v > 0) & comp(thr, v)) if score else (lambda v: comp(v, thr) & (v > 0))
        want = ref.eps(indptr, cols, vals, keep)
        assert want[0][-1] > 0 or comp not in (operator.le, operator.ge)
        ref.csr_equals(got, want)
    got = pg150.rescore(g, op, eps=thr + 0.5)                              # a radius between two values
    keep = (lambda v: (v > 0) & (thr + 0.5 <= v)) if score else (lambda v: (v <= thr + 0.5) & (v > 0))
    ref.csr_equals(got, ref.eps(indptr, cols, vals, keep))


@pytest.mark.parametrize("which", range(4))
def test_rescore_of_queries_and_of_a_selection(pg150, which):
    tok, queries, (indptr, cols), (qptr, qcols), ops, D, Dq = brute()
    op, score = ops[which], which != GLOBAL
    vals = _edge_values(Dq[which], qptr, qcols)
    g = _graph(qptr, qcols, 150)
    got = pg150.rescore(g, op, k=5, queries=queries)
    ref.knn_equals(got, ref.knn(qptr, qcols, vals, 5, score), 0)
    if not score:
        assert (vals == 0).any()                                           # a query that is a data row: d = 0 is kept
    for comp, thr in ((operator.le, 6), (operator.ge, 3)):
        got = pg150.rescore(g, op, eps=thr, comp=comp, queries=queries)
        keep = (lambda v: (v > 0) & comp(thr, v)) if score else (lambda v: comp(v, thr))
        ref.csr_equals(got, ref.eps(qptr, qcols, vals, keep))
    # idxs: the graph is over a selection of 100 rows, both ends go through it
    sel = np.random.default_rng(41).permutation(150)[:100]
    sptr, scols = ref.random_csr(np.random.default_rng(42), 100, 100, 30)
    vals = D[which][sel][:, sel][np.repeat(np.arange(100), np.diff(sptr)), scols]
    got = pg150.rescore(_graph(sptr, scols, 100), op, k=6, idxs=sel)
    ref.knn_equals(got, ref.knn(sptr, scols, vals, 6, score), 1)
    # row0: rows 40..99 of the data's graph
    part = _graph(indptr[40:101] - indptr[40], cols[indptr[40]:indptr[100]], 150, row0=40)
    want = ref.knn(indptr, cols, _edge_values(D[which], indptr, cols), 4, score)
    got = pg150.rescore(part, op, k=4)
    assert got.row0 == 40
    ref.knn_equals(got, (want[0][40:100], want[1][40:100]), 1)


# ---------------------------------------------------------------- the whole data set as the pool: the exact graph
@functools.lru_cache(maxsize=None)
def distinct():
    """120 random sequences of 40 symbols out of 8 whose exact rank 0 is the row itself under every operator."""
    ops = _operators(9)[:3]
    for seed in range(50, 60):
        tok = np.random.default_rng(seed).integers(1, 9, (120, 40)).astype(np.uint8)
        X = torch.from_numpy(tok)
        firsts = [np.argsort(op(X, X).numpy() * (1 if i == 0 else -1), axis=1, kind="stable")[:, 0] for i, op in enumerate(ops)]
        if len(np.unique(tok, axis=0)) == 120 and all(np.array_equal(f, np.arange(120)) for f in firsts):
            return tok, ops
    raise AssertionError("no seed gives distinct rows that rank first in their own lists")


def _same_knn(a, b):
    assert a.idx.shape == b.idx.shape
    assert torch.equal(a.idx, b.idx) and torch.equal(a.dist.to(torch.int64), b.dist.to(torch.int64))


def test_the_whole_data_set_as_the_pool_gives_the_exact_graph(tmp_path):
    tok, ops = distinct()
    P = _prograph(tmp_path, tok, "distinct")
    others = np.concatenate([np.delete(np.arange(120), r) for r in range(120)])
    everyone_else = _graph(np.arange(0, 120 * 119 + 1, 119, dtype=np.int64), others, 120)
    queries = np.concatenate([tok[[7, 100]], np.random.default_rng(61).integers(1, 9, (3, 40)).astype(np.uint8)])
    for op in ops:
        exact = P.build_graph(distance=op, k=7, output="csr")
        _same_knn(P.build_graph(distance=op, k=7, candidates=everyone_else, output="csr"), exact)
        _same_knn(P.build_graph(distance=op, k=7, candidates=hamming, pool=119, output="csr"), exact)
        hits = P.search(queries, distance=op, k=7, output="csr")
        _same_knn(P.search(queries, distance=op, k=7, candidates=hamming, pool=120, output="csr"), hits)


# ---------------------------------------------------------------- the device route against the fallback
def test_the_device_route_and_the_fallback_agree_at_128_positions(tmp_path, monkeypatch):
    rng = np.random.default_rng(71)
    tok = _mixed(rng, 40, 128, 4)
    P = _prograph(tmp_path, tok, "wide")
    assert P.tokenized.shape[1] == 128
    indptr, cols = ref.random_csr(rng, 40, 40, 30)
    g = _graph(indptr, cols, 40)
    for op in _operators(A4):
        thr = int(P.rescore(g, op).weights.median())
        forms = lambda: [P.rescore(g, op), P.rescore(g, op, k=5), P.rescore(g, op, k=70), P.rescore(g, op, eps=thr),     # noqa: E731
                         P.rescore(g, op, eps=thr, comp=operator.gt)]
        fast = forms()
        with monkeypatch.context() as m:
            m.setattr(_native, "aln_list_ready", lambda: False)
            slow = forms()
        for a, b in zip(fast, slow):
            assert type(a) is type(b)
            for name in (("idx", "dist") if isinstance(a, KNNGraph) else ("indptr", "indices", "weights")):
                x, y = getattr(a, name), getattr(b, name)
                assert x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu()), name
        assert fast[0].nnz and (fast[3].nnz or fast[4].nnz)
