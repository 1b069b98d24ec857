"""
The long edge-list kernel (`pg_alignment_list_long_scores`, prograph_amd/csrc/pg_aln_list_long.h) and the route of
`Prograph.rescore` / `candidates=` onto it at 129..2048 positions on the GPU.  Every comparison is of
integers and exact.

The kernel: the 19 Y rows x 300 X columns (npad 512) and the lists of tests/test_alignment_list_gpu.py - 0 .. 600 entries,
repeated columns, the row's own number and entries that name no column - at widths on both sides of every strip and
strip-group seam; every entry against the mode's LONG dense entry computed in the same test.  Three of the 19 lists are
empty, so every width runs twice, the Y lengths shifted against the lists by seven rows the second time: every planted Y
length meets a list.  Then the short list entry at widths it shares, a seeded subset against the suite's Python
definitions and the int32-cell strip tracer (`pg_alignment_stats` stops at 128 positions, so the heads are
`alignment_trace_long_heads`'), one problem per mode at its 16-bit bound, a workspace of one and of three shares, guard
words, empty lists, and `rescore` / `build_graph(candidates=)` against brute force and the fallback.
"""
import ctypes
import functools
import operator

import numpy as np
import pytest
import torch

import aln_lengths_testdata as ald
import fit_testdata
import rescore_testdata as ref
from long_testdata import rows_of
from test_alignment_list_gpu import (COMPS, INT32_MIN, LIST_LENS, M, MODES, N, _edge_values, _graph, _mixed, _operators,
                                     _prograph, _same_knn, device_table, expected, table)
from prograph_amd import _native
from prograph_amd.distance import fit_alignment, local_alignment, semiglobal_alignment, alignment, spectrum
from prograph_amd.graph import KNNGraph

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

GLOBAL, LOCAL, SEMIGLOBAL, FIT = MODES
WIDTHS = ((129, 129), (300, 260), (47, 1100), (1030, 100), (140, 2048), (2048, 140))      # (xl, yl)
Y_MUST = (0, 1, 127, 128, 129, 143, 144, 145, 255, 256, 257, 1023, 1024, 1025, 1040, 1041, 2047, 2048)
X_MUST = (0, 1, 3, 4, 5, 127, 128, 129)
DEFINITION = dict(zip(MODES, (ald.DEFINITION["global"], ald.DEFINITION["local"], ald.DEFINITION["semiglobal"],
                              fit_testdata.definition)))
DENSE = {GLOBAL: _native.alignment_long_dense, LOCAL: _native.alignment_local_long_dense,
         SEMIGLOBAL: _native.alignment_semiglobal_long_dense, FIT: _native.alignment_fit_long_dense}
FITS = {GLOBAL: lambda xl, yl, T, e, o: _native.aln_long_fits(max(xl, yl), max(int(T.max()), e), e, o),
        LOCAL: lambda xl, yl, T, e, o: _native.aln_local_long_fits(xl, yl, int(T.max())),
        SEMIGLOBAL: lambda xl, yl, T, e, o: _native.aln_semiglobal_long_fits(xl, yl, int(T.max())),
        FIT: lambda xl, yl, T, e, o: _native.aln_fit_fits(xl, yl, int(T.max()), e, o)}


def y_lengths(yl, shift):
    """19 lengths: those of Y_MUST that fit yl, the rest from yl - 3 .. yl (yl first), rotated by `shift` rows."""
    lens = [l for l in Y_MUST if l <= yl]
    lens += [yl - r % 4 for r in range(M - len(lens))]
    assert len(lens) == M and yl in lens
    return lens[shift:] + lens[:shift]


def x_lengths(rng, xl):
    """300 lengths: X_MUST where they fit, xl - 1 and xl, chosen explicitly; the rest drawn from 0 .. xl."""
    lens = [l for l in X_MUST if l <= xl] + [xl - 1, xl]
    return lens + list(rng.integers(0, xl + 1, N - len(lens)))


@functools.lru_cache(maxsize=None)
def problem(xl, yl, shift=0, most=600):
    """(X, Y, indptr, indices, xlens, ylens): the lists of tests/test_alignment_list_gpu.py's `problem` (LIST_LENS entries
    a row, at most `most`: random columns with repeats, the row's own number, -1, n and n + 5) over columns and rows of the
    lengths above."""
    rng = np.random.default_rng(100 * xl + yl + shift)
    xlens = [int(x) for x in np.array(x_lengths(rng, xl))[rng.permutation(N)]]
    ylens = y_lengths(yl, shift)
    X = rows_of(rng, ald.SYMS, xlens, xl).astype(np.uint8)
    Y = rows_of(rng, ald.SYMS, ylens, yl).astype(np.uint8)
    lens = [min(n, most) for n in LIST_LENS]
    lists = []
    for r, n in enumerate(lens):
        c = rng.integers(0, N, n)
        if n >= 63:
            c[[2, 17, 40, 61, n - 1]] = (r, -1, N, N + 5, -1)
        elif n == 1 and r > 5:
            c[0] = N
        lists.append(c)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return X, Y, indptr, np.concatenate(lists).astype(np.int32), xlens, ylens


def operands(X, Y):
    return _native.aln_long_operand(torch.from_numpy(X), ald.SYMS), _native.aln_long_operand(torch.from_numpy(Y), ald.SYMS)


def check_against_dense(mode, xl, yl, gaps, most=600):
    met = set()                                                           # Y lengths that met a list with entries
    for shift in (0, 7):
        X, Y, indptr, indices, xlens, ylens = problem(xl, yl, shift, most)
        assert {l for l in X_MUST if l <= xl} | {xl - 1, xl} <= set(xlens)
        met |= {l for r, l in enumerate(ylens) if indptr[r + 1] > indptr[r]}
        xo, yo = operands(X, Y)
        assert xo.npad == 512 and (xo.l, yo.l) == (xl, yl)
        T = table(mode)
        for gap, gap_open in gaps:
            assert FITS[mode](xl, yl, T, gap, gap_open)
            dense = DENSE[mode](xo, yo, device_table(mode, T), gap, gap_open, out_bytes=8)
            got = _native.alignment_list_long_scores(xo, yo, indptr, indices, mode, device_table(mode, T), gap, gap_open)
            assert got.dtype == torch.int32 and got.shape == (len(indices),)
            want = expected(dense.cpu().numpy(), indptr, indices)
            assert (want == INT32_MIN).sum() >= 30 and (want != INT32_MIN).sum() > (3000 if most == 600 else 500)
            bad = np.flatnonzero(got.cpu().numpy() != want)
            assert not len(bad), (shift, gap, gap_open, bad[:8], got.cpu().numpy()[bad[:8]], want[bad[:8]])
        assert xo.valid() and yo.valid()
    assert {l for l in Y_MUST if l <= yl} | {yl} <= met


@pytest.mark.parametrize("xl,yl", WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_every_entry_is_the_long_dense_entry(mode, xl, yl):
    check_against_dense(mode, xl, yl, ald.GAPS)


@pytest.mark.parametrize("mode", MODES)
def test_every_entry_is_the_long_dense_entry_at_2048_by_2048(mode):
    check_against_dense(mode, 2048, 2048, ald.GAPS[1:], most=65)


@pytest.mark.parametrize("xl,yl", [(128, 128), (33, 20)])
def test_up_to_128_positions_the_short_list_entry_says_the_same(xl, yl):
    X, Y, indptr, indices, _, _ = problem(xl, yl)
    xo, yo = operands(X, Y)
    xs, ys = _native.aln_operand(torch.from_numpy(X), ald.SYMS), _native.aln_operand(torch.from_numpy(Y), ald.SYMS)
    for mode in MODES:
        T = device_table(mode, table(mode))
        for gap, gap_open in ald.GAPS:
            short = _native.alignment_list_scores(xs, ys, indptr, indices, mode, T, gap, gap_open)
            assert torch.equal(_native.alignment_list_long_scores(xo, yo, indptr, indices, mode, T, gap, gap_open), short)
        assert int((short == INT32_MIN).sum()) >= 30


@pytest.mark.parametrize("mode", MODES)
def test_a_subset_is_the_definition_and_the_strip_tracer(mode):
    """19 rows x 10 columns = 190 pairs of the (300, 260) problem, gap 3, gap_open 11."""
    X, Y, _, _, _, _ = problem(300, 260)
    cols = np.random.default_rng(7).permutation(N)[:10]
    T = table(mode)
    indptr = np.arange(0, M * 10 + 1, 10, dtype=np.int64)
    indices = np.tile(cols, M).astype(np.int32)
    xo, yo = operands(X, Y)
    got = _native.alignment_list_long_scores(xo, yo, indptr, indices, mode, device_table(mode, T), 3, 11).cpu().numpy()
    D = DEFINITION[mode](T, 3, 11, X[cols].astype(np.int64), Y.astype(np.int64))      # (M, 10)
    assert np.array_equal(got, D.reshape(-1))
    rows = np.repeat(np.arange(M), 10)
    head = _native.alignment_trace_long_heads(xo, yo, indices, rows, mode, device_table(mode, T), 3, 11)      # x: the free ends
    assert np.array_equal(got, head[:, 0].cpu().numpy())


# ---------------------------------------------------------------- the 16-bit cells at their bounds
def _list_of_all(m, n):
    return np.arange(0, m * n + 1, n, dtype=np.int64), np.tile(np.arange(n), m).astype(np.int32)


def _at_the_bound(mode, op, T, gap, gap_open, X, Y):
    """Every pair of X x Y through the list kernel against the operator's CPU value (its torch expression: no kernel) and
    the long dense entry."""
    want = op(torch.from_numpy(X), torch.from_numpy(Y)).numpy()          # (len(Y), len(X))
    xo, yo = (_native.aln_long_operand(torch.from_numpy(t), T.shape[0]) for t in (X, Y))
    indptr, indices = _list_of_all(len(Y), len(X))
    Td = device_table(mode, T)
    got = _native.alignment_list_long_scores(xo, yo, indptr, indices, mode, Td, gap, gap_open).cpu().numpy()
    assert np.array_equal(got.reshape(want.shape), want)
    assert np.array_equal(DENSE[mode](xo, yo, Td, gap, gap_open, out_bytes=8).cpu().numpy(), want)
    return want


def test_global_cells_at_the_bound():
    """257 positions at cost 253, gap 253, gap_open 4: 257 * 253 + 2 * 4 + 2 * 253 = 65 535.  Constant rows reach the largest
    H: 257 substitutions (65 021), and one pair plus a run of 256 through E and through F."""
    C = np.zeros((21, 21), dtype=np.int64)
    C[3, 7] = C[7, 3] = 253
    assert _native.aln_long_fits(257, 253, 253, 4) and not _native.aln_long_fits(257, 253, 253, 5)
    X, Y = np.full((5, 257), 3, dtype=np.uint8), np.full((3, 257), 7, dtype=np.uint8)
    Y[1, 1:] = 0
    X[1, 1:] = 0
    X[2, :] = 0
    want = _at_the_bound(GLOBAL, alignment(C, 253, gap_open=4), C, 253, 4, X, Y)
    assert want[0, 0] == 257 * 253 and want[1, 0] == want[0, 1] == 253 + 4 + 256 * 253 and want[0, 2] == 4 + 257 * 253


def _diagonal_table(top):
    S = np.full((4, 4), -128)
    S[np.arange(4), np.arange(4)] = (3, top, 7, 9)
    return S


def test_local_cells_at_the_bound():
    """544 positions at max S = 120: 544 * 120 + 255 = 65 535, reached by 544 ones against 544 ones."""
    S = _diagonal_table(120)
    assert _native.aln_local_long_fits(544, 544, 120) and not _native.aln_local_long_fits(545, 545, 120)
    rng = np.random.default_rng(5)
    X = rows_of(rng, 4, (544, 544, 300, 0), 544).astype(np.uint8)
    Y = rows_of(rng, 4, (544, 544, 129), 544).astype(np.uint8)
    X[0], Y[0] = 1, 1
    want = _at_the_bound(LOCAL, local_alignment(S, 2, gap_open=1), S, 2, 1, X, Y)
    assert want[0, 0] == 544 * 120 and (want[:, 3] == 0).all()


def test_semiglobal_cells_at_the_bound():
    """272 positions at max S = 120: 2 * 272 * 120 + 255 = 65 535; 272 ones against 272 ones reach Z + Z."""
    S = _diagonal_table(120)
    assert _native.aln_semiglobal_long_fits(272, 272, 120) and not _native.aln_semiglobal_long_fits(273, 273, 120)
    rng = np.random.default_rng(6)
    X = rows_of(rng, 4, (272, 272, 200, 0), 272).astype(np.uint8)
    Y = rows_of(rng, 4, (272, 272, 129), 272).astype(np.uint8)
    X[0], Y[0] = 1, 1
    want = _at_the_bound(SEMIGLOBAL, semiglobal_alignment(S, 2, gap_open=1), S, 2, 1, X, Y)
    assert want[0, 0] == 272 * 120 and (want[:, 3] == 0).all()


def test_fit_cells_at_the_bound():
    """129 positions of y at max S = 127, gap 252, gap_open 6: 6 + 129 * (252 + 254) + 255 = 65 535; 129 ones within 140
    ones reach the largest cell, an empty x the smallest score."""
    S = _diagonal_table(127)
    assert _native.aln_fit_fits(140, 129, 127, 252, 6) and not _native.aln_fit_fits(140, 129, 127, 252, 7)
    rng = np.random.default_rng(7)
    X = rows_of(rng, 4, (140, 140, 129, 0), 140).astype(np.uint8)
    Y = rows_of(rng, 4, (129, 129, 60), 129).astype(np.uint8)
    X[0], Y[0] = 1, 1
    want = _at_the_bound(FIT, fit_alignment(S, 252, gap_open=6), S, 252, 6, X, Y)
    assert want[0, 0] == 129 * 127 and want[0, 3] == -(6 + 129 * 252)


# ---------------------------------------------------------------- the workspace, guard words, empty lists
def _raw(mode, xo, yo, indptr, indices, T, scores_ptr, ws_ptr, ws_bytes):
    return _native.lib().pg_alignment_list_long_scores(mode, _native._ptr(xo.buf), xo.n, xo.npad, xo.l, _native._ptr(yo.buf), yo.n,
                                                       yo.npad, yo.l, _native._ptr(indptr), _native._ptr(indices), _native._ptr(T),
                                                       3, 11, scores_ptr, ws_ptr, ws_bytes, _native._stream())


def _share(xl):
    one = ctypes.c_int64(0)
    assert _native.lib().pg_alignment_long_workspace(xl, ctypes.byref(one), None) == 0
    return one.value


@pytest.mark.parametrize("xl,yl", [(300, 260), (140, 2048)])
def test_a_workspace_of_one_share_and_of_three(xl, yl):
    """One workgroup walks all 19 rows over one slice; three share them 7 / 6 / 6: the same scores as one slice a row."""
    X, Y, indptr, indices, _, _ = problem(xl, yl)
    xo, yo = operands(X, Y)
    one = _share(xl)
    for mode in MODES:
        T = device_table(mode, table(mode))
        full = _native.alignment_list_long_scores(xo, yo, indptr, indices, mode, T, 3, 11)
        for shares in (1, 3):
            got = _native.alignment_list_long_scores(xo, yo, indptr, indices, mode, T, 3, 11, workspace_bytes=shares * one)
            assert torch.equal(got, full), (mode, shares)
        with pytest.raises(RuntimeError, match="workspace"):
            _native.alignment_list_long_scores(xo, yo, indptr, indices, mode, T, 3, 11, workspace_bytes=one - 1)


def test_memory_around_the_scores_and_the_workspace_is_untouched():
    X, Y, indptr, indices, _, _ = problem(300, 260)
    xo, yo = operands(X, Y)
    dev = xo.buf.device
    ip, ix = torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev)
    nnz, guard, mark, one = len(indices), 64, 0x5A5A5A5A, _share(300)
    shares = 3
    for mode in MODES:
        T = device_table(mode, table(mode))
        buf = torch.full((nnz + 2 * guard,), mark, dtype=torch.int32, device=dev)
        ws = torch.full((shares * one // 4 + 2 * guard,), mark, dtype=torch.int32, device=dev)
        args = (ctypes.c_void_p(ws.data_ptr() + 4 * guard), shares * one + 3)       # (three bytes are no fourth share)
        assert _raw(mode, xo, yo, ip, ix, T, ctypes.c_void_p(buf.data_ptr() + 4 * guard), *args) == 0
        out, w = buf.cpu().numpy(), ws.cpu().numpy()
        assert (out[:guard] == mark).all() and (out[-guard:] == mark).all()
        assert (w[:guard] == mark).all() and (w[-guard:] == mark).all() and (w[guard:-guard] != mark).any()
        want = _native.alignment_list_long_scores(xo, yo, indptr, indices, mode, T, 3, 11).cpu().numpy()
        assert np.array_equal(out[guard:-guard], want) and (want != mark).all()
        # rows without a list write nothing, not to the workspace either: every list empty
        buf.fill_(mark)
        ws.fill_(mark)
        assert _raw(mode, xo, yo, torch.zeros(M + 1, dtype=torch.int64, device=dev), ix, T, _native._ptr(buf), *args) == 0
        assert bool((buf == mark).all()) and bool((ws == mark).all())
        # one row of 600 entries between empty rows
        alone = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        alone[6:] = 600
        assert _raw(mode, xo, yo, alone, ix, T, ctypes.c_void_p(buf.data_ptr() + 4 * guard), *args) == 0
        out = buf.cpu().numpy()
        assert (out[:guard] == mark).all() and (out[guard + 600:] == mark).all()
        one_row = _native.alignment_list_long_scores(xo, yo, alone, indices[:600], mode, T, 3, 11).cpu().numpy()
        assert np.array_equal(out[guard:guard + 600], one_row)
        dense = DENSE[mode](xo, yo, T, 3, 11, out_bytes=8, rows=(5, 6)).cpu().numpy()
        assert np.array_equal(one_row, expected(dense, np.array([0, 600]), indices[:600]))
    assert xo.valid() and yo.valid()
    assert _native.alignment_list_long_scores(xo, yo, np.zeros(M + 1, dtype=np.int64), indices[:0], GLOBAL, T, 3, 11).numel() == 0


def test_argument_errors_return_before_any_launch():
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                              # never dereferenced
    one = _share(300)

    def call(mode=0, x=p, n=4, xnpad=256, xl=300, y=p, m=4, ynpad=256, yl=9, indptr=p, indices=p, table=p, gap=1, gap_open=0,
             scores=p, ws=p, ws_bytes=one):
        return lib.pg_alignment_list_long_scores(mode, x, n, xnpad, xl, y, m, ynpad, yl, indptr, indices, table, gap, gap_open,
                                                 scores, ws, ws_bytes, _native._stream())
    for bad in (dict(x=None), dict(y=None), dict(indptr=None), dict(indices=None), dict(table=None), dict(scores=None),
                dict(mode=4), dict(mode=-1), dict(gap=0), dict(gap=256), dict(gap_open=-1), dict(xnpad=3), dict(ynpad=3),
                dict(ws=None), dict(ws_bytes=one - 1)):
        assert call(**bad) == -1, bad
    assert call(xl=2049, ws_bytes=1 << 40) == -2 and call(yl=2049) == -2
    torch.cuda.synchronize()


# ---------------------------------------------------------------- rescore against brute force
A4 = 5                                                                      # tokens 1..4 and the padding


@functools.lru_cache(maxsize=None)
def brute(width):
    """Sequences of 1..width symbols out of 4 (most of them short, so that the CPU values stay cheap), a candidate graph,
    queries at another width, and the operators' values on the CPU: D[op][r, c] over the data, Dq[op][q, c]."""
    rng = np.random.default_rng(31 + width)
    n = 40 if width <= 200 else 10
    tok = _mixed(rng, n, 60, 4, width=width)
    tok[1] = rows_of(rng, 5, [width], width)[0]                            # one row as wide as the matrix, one a little shorter
    tok[2] = rows_of(rng, 5, [width - 70], width)[0]
    queries = _mixed(rng, 3, 50, 4, width=width - 9)
    queries[0] = rows_of(rng, 5, [width - 9], width - 9)[0]
    queries[1, :50] = tok[5, :50]
    indptr, cols = ref.random_csr(rng, n, n, n - 5)
    qptr, qcols = ref.random_csr(rng, 3, n, n - 5, own_row=False)
    X, Q = torch.from_numpy(tok), torch.from_numpy(queries)
    ops = _operators(A4)
    D = [op(X, X).numpy() for op in ops]
    Dq = [op(X, Q).numpy() for op in ops]
    return tok, queries, (indptr, cols), (qptr, qcols), ops, D, Dq


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("width", [200, 1100])
def test_rescore_is_the_brute_force_selection(tmp_path, monkeypatch, width, which):
    tok, queries, (indptr, cols), (qptr, qcols), ops, D, Dq = brute(width)
    P = _prograph(tmp_path, tok, f"brute{width}")
    n = len(tok)
    calls = []
    real = _native.alignment_list_long_scores
    monkeypatch.setattr(_native, "alignment_list_long_scores", lambda *a, **k: calls.append(1) or real(*a, **k))
    op, score = ops[which], which != GLOBAL
    vals = _edge_values(D[which], indptr, cols)
    g = _graph(indptr, cols, n)
    plain = P.rescore(g, op)
    assert plain.weights.dtype == torch.int32 and plain.weights.is_cuda and len(calls) == 1
    ref.csr_equals(plain, (indptr, cols, vals))
    for k in (1, 5, n):
        got = P.rescore(g, op, k=k)
        assert isinstance(got, KNNGraph) and got.dist.dtype == torch.int32
        ref.knn_equals(got, ref.knn(indptr, cols, vals, k, score), 1)
    thr = int(np.median(vals[vals > 0]))
    for comp in COMPS:
        got = P.rescore(g, op, eps=thr, comp=comp)
        keep = (lambda v: (v > 0) & comp(thr, v)) if score else (lambda v: comp(v, thr) & (v > 0))
        ref.csr_equals(got, ref.eps(indptr, cols, vals, keep))
    # queries (of another width) and a selection
    qvals = _edge_values(Dq[which], qptr, qcols)
    gq = _graph(qptr, qcols, n)
    ref.knn_equals(P.rescore(gq, op, k=4, queries=queries), ref.knn(qptr, qcols, qvals, 4, score), 0)
    keep = (lambda v: (v > 0) & (v >= 3)) if score else (lambda v: v <= thr)
    ref.csr_equals(P.rescore(gq, op, eps=3 if score else thr, queries=queries),
                   ref.eps(qptr, qcols, qvals, keep))
    sel = np.random.default_rng(41).permutation(n)[:n - 3]
    sel[0] = 1                                                             # the widest row stays in
    sel = np.unique(sel)[::-1].copy()
    sptr, scols = ref.random_csr(np.random.default_rng(42), len(sel), len(sel), 5)
    svals = D[which][sel][:, sel][np.repeat(np.arange(len(sel)), np.diff(sptr)), scols]
    ref.knn_equals(P.rescore(_graph(sptr, scols, len(sel)), op, k=3, idxs=sel), ref.knn(sptr, scols, svals, 3, score), 1)
    assert len(calls) == 4 + len(COMPS) + 3                                # every call above took the long list kernel


def test_the_device_route_and_the_fallback_agree_at_129_positions(tmp_path, monkeypatch):
    rng = np.random.default_rng(71)
    tok = _mixed(rng, 40, 129, 4)
    P = _prograph(tmp_path, tok, "wide129")
    assert P.tokenized.shape[1] == 129
    indptr, cols = ref.random_csr(rng, 40, 40, 30)
    g = _graph(indptr, cols, 40)
    calls = []
    real = _native.alignment_list_long_scores
    monkeypatch.setattr(_native, "alignment_list_long_scores", lambda *a, **k: calls.append(1) or real(*a, **k))
    for op in _operators(A4):
        thr = int(P.rescore(g, op).weights.median())
        forms = lambda: [P.rescore(g, op), P.rescore(g, op, k=5), P.rescore(g, op, k=70), P.rescore(g, op, eps=thr),     # noqa: E731
                         P.rescore(g, op, eps=thr, comp=operator.gt)]
        del calls[:]
        fast = forms()
        assert len(calls) == 5
        with monkeypatch.context() as m:
            m.setattr(_native, "aln_list_long_ready", lambda: False)
            slow = forms()
        assert len(calls) == 5
        for a, b in zip(fast, slow):
            assert type(a) is type(b)
            for name in (("idx", "dist") if isinstance(a, KNNGraph) else ("indptr", "indices", "weights")):
                x, y = getattr(a, name), getattr(b, name)
                assert x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu()), name
        assert fast[0].nnz and (fast[3].nnz or fast[4].nnz)


def test_the_whole_data_set_as_the_pool_gives_the_exact_graph_at_200_positions(tmp_path, monkeypatch):
    """60 random rows of 200 symbols out of 8: every row ranks first in its own list, so the exact graph (rank 0 dropped)
    and the rescored pool of everyone else (the row itself left out) are the same graph."""
    tok = np.random.default_rng(50).integers(1, 9, (60, 200)).astype(np.uint8)
    P = _prograph(tmp_path, tok, "distinct200")
    op = _operators(9)[1]                                                  # local_alignment, gap 1, gap_open 1
    X = torch.from_numpy(tok).cuda()
    assert np.array_equal(np.argsort(-op(X, X).cpu().numpy(), axis=1, kind="stable")[:, 0], np.arange(60))
    calls = []
    real = _native.alignment_list_long_scores
    monkeypatch.setattr(_native, "alignment_list_long_scores", lambda *a, **k: calls.append(1) or real(*a, **k))
    exact = P.build_graph(distance=op, k=7, output="csr")
    assert not calls
    _same_knn(P.build_graph(distance=op, k=7, candidates=spectrum(k=3, symbols=8), pool=59, output="csr"), exact)
    assert len(calls) == 1

