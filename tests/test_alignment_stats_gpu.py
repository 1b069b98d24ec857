"""
The statistics kernel (`pg_alignment_stats`, prograph_amd/csrc/pg_aln_stats.hip) on the GPU: all eight columns of every
pair's head against `definition` of tests/trace_testdata.py (fit: `canonical` of tests/fit_testdata.py), exactly; against
the traceback kernel's head on the same pairs, device against device; and the percent-identity cuts of `build_graph` /
`search` against the host filter of the unfiltered result.  The problem sizes are tests/test_alignment_trace_gpu.py's: one
list of 200 pairs per (mode, gap, gap_open, widths) serves every list length, the reference is computed once.
"""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from fit_testdata import canonical, seq
from trace_testdata import FIELDS, GLOBAL, LOCAL, SEMIGLOBAL, definition
from prograph_amd import _native, alignments, synth
from prograph_amd.distance import alignment, fit_alignment, local_alignment, semiglobal_alignment
from prograph_amd.graph import CSRGraph, KNNGraph

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

FIT = 3
LENS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)       # around the 4-token dwords and the three kernels
A, ROWS, PAIRS = 6, 48, 200
MODES = (GLOBAL, LOCAL, SEMIGLOBAL, FIT)
EXTREME = "extreme"


def table(mode, kind=None):
    rng = np.random.default_rng(11 + mode)
    if kind == EXTREME:                                                     # cost 255; scores 127 and -128
        return (255 * (1 - np.eye(A, dtype=np.int64))) if mode == GLOBAL else np.where(np.eye(A, dtype=bool), 127, -128)
    if mode == GLOBAL:
        T = rng.integers(1, 4, (A, A))
        return np.triu(T, 1) + np.triu(T, 1).T
    T = rng.integers(-3, 2, (A, A))
    T = np.triu(T) + np.triu(T, 1).T
    T[np.arange(A), np.arange(A)] = rng.integers(1, 5, A)
    T[0, 1] = T[1, 0] = 2                                                   # S[a][0] > 0: padding must not pair
    return T


def operand(rng, width):
    """(ROWS, width) tokens: the lengths of LENS that fit, mixed row by row (so within every wave), zeros inside."""
    lens = [l for l in LENS if l <= width]
    M = np.zeros((ROWS, width), dtype=np.uint8)
    for r in range(ROWS):
        l = lens[r % len(lens)] if r < 2 * len(lens) else int(rng.choice(lens))
        M[r, :l] = rng.integers(0, A, l)
        if l:
            M[r, l - 1] = rng.integers(1, A)
    return M[rng.permutation(ROWS)]


def head_of(mode, T, gap, gap_open, x, y):
    if mode == FIT:
        return list(canonical(T, gap, gap_open, seq(x), seq(y))[:7]) + [0]
    d = definition(mode, T, gap, gap_open, x, y)
    return [d[f] for f in FIELDS] + [0]


@functools.lru_cache(maxsize=None)
def problem(mode, gap, gap_open, xw, yw, kind=None, count=PAIRS):
    """Two operands, a random pair list over their rows (200 pairs over 48 rows: rows and whole pairs repeat), and the
    definition's head of the first `count` pairs."""
    rng = np.random.default_rng(1000 * mode + 10 * gap + gap_open + xw + 7 * yw)
    X, Y = operand(rng, xw), operand(rng, yw)
    xi, yi = rng.integers(0, ROWS, PAIRS), rng.integers(0, ROWS, PAIRS)
    xi[1], yi[1] = xi[0], yi[0]                                             # the same pair twice, the same row in two pairs
    xi[2] = xi[0]
    T = table(mode, kind)
    want = np.array([head_of(mode, T, gap, gap_open, X[xi[p]], Y[yi[p]]) for p in range(count)], dtype=np.int32)
    return X, Y, xi[:count], yi[:count], T, want


def device_table(mode, T):
    return _native.sub_cost(T) if mode == GLOBAL else _native.aln_local_score(T)


def operands(X, Y):
    return _native.aln_operand(torch.from_numpy(X), A), _native.aln_operand(torch.from_numpy(Y), A)


def same(head, want):
    head = head.cpu().numpy()
    assert head.shape == want.shape and head.dtype == np.int32
    bad = np.flatnonzero((head != want).any(1))
    assert not len(bad), (bad[:5], head[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("gap_open", [0, 11])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("xw,yw", [(128, 128), (20, 128)])
def test_every_column_is_the_definition(xw, yw, mode, gap_open):
    X, Y, xi, yi, T, want = problem(mode, 2, gap_open, xw, yw)
    xo, yo = operands(X, Y)
    for pairs in (1, 63, 64, 65, 200):
        head = _native.alignment_stats(xo, yo, xi[:pairs], yi[:pairs], mode, device_table(mode, T), 2, gap_open)
        same(head, want[:pairs])
    assert xo.valid() and yo.valid()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("xw,yw", [(128, 64), (128, 32), (33, 20)])
def test_the_narrow_kernels(xw, yw, mode):
    """y operands of at most 64 and at most 32 positions run the kernels with the shorter column."""
    X, Y, xi, yi, T, want = problem(mode, 2, 3, xw, yw)
    xo, yo = operands(X, Y)
    same(_native.alignment_stats(xo, yo, xi, yi, mode, device_table(mode, T), 2, 3), want)


@pytest.mark.parametrize("mode", MODES)
def test_the_largest_penalties_and_tables(mode):
    for kind in (EXTREME, None):
        X, Y, xi, yi, T, want = problem(mode, 255, 255, 128, 128, kind, 65)
        xo, yo = operands(X, Y)
        same(_native.alignment_stats(xo, yo, xi, yi, mode, device_table(mode, T), 255, 255), want)


@pytest.mark.parametrize("mode", MODES)
def test_the_head_is_the_traceback_kernels(mode):
    """Device against device: pg_alignment_trace / pg_alignment_fit_trace on the same pairs."""
    for xw, yw, gap_open in ((128, 128, 11), (20, 128, 0), (128, 64, 3)):
        X, Y, xi, yi, T, want = problem(mode, 2, gap_open, xw, yw)
        xo, yo = operands(X, Y)
        traced, _ = _native.alignment_trace(xo, yo, xi, yi, mode, device_table(mode, T), 2, gap_open)
        assert torch.equal(_native.alignment_stats(xo, yo, xi, yi, mode, device_table(mode, T), 2, gap_open), traced)


def test_a_list_longer_than_the_grid_and_an_index_outside():
    """More than 1024 waves' worth of pairs: the grid strides over the list.  Short sequences keep it quick; the list is the
    200 pairs over and over, so every 200 rows of the result are the first 200."""
    X, Y, xi, yi, T, want = problem(LOCAL, 2, 3, 33, 20)
    xo, yo = operands(X, Y)
    reps = 1024 * 64 // PAIRS + 3
    head = _native.alignment_stats(xo, yo, np.tile(xi, reps), np.tile(yi, reps), LOCAL, device_table(LOCAL, T), 2, 3)
    assert head.shape == (reps * PAIRS, 8) and reps * PAIRS > 1024 * 64
    assert torch.equal(head.reshape(reps, PAIRS, 8), torch.from_numpy(want).cuda().expand(reps, PAIRS, 8))
    # the wrapper refuses an index outside its operand; the kernel, asked directly, marks the pair and touches nothing
    with pytest.raises(IndexError):
        _native.alignment_stats(xo, yo, [0, ROWS], [0, 0], LOCAL, device_table(LOCAL, T), 2, 3)
    bx = torch.tensor([int(xi[0]), ROWS, -1, int(xi[3])], dtype=torch.int32, device="cuda")
    by = torch.tensor([int(yi[0]), 0, 0, int(yi[3])], dtype=torch.int32, device="cuda")
    raw = torch.full((4, 8), 77, dtype=torch.int32, device="cuda")
    _native._stats_launch(xo, yo, bx, by, LOCAL, device_table(LOCAL, T), 2, 3, raw)
    assert raw.cpu().tolist() == [want[0].tolist(), [0, 0, 0, 0, 0, -1, 0, 1], [0, 0, 0, 0, 0, -1, 0, 1], want[3].tolist()]


# ---------------------------------------------------------------- through Prograph
@pytest.fixture(scope="module")
def pg(tmp_path_factory):
    from prograph_amd import Prograph
    tok, _ = synth.clustered_varlen_tokens(150, Lmax=40, Lmin=8, seed=9, members=10)
    f = tmp_path_factory.mktemp("stats") / "stats.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P, tok


def _operators():
    rng = np.random.default_rng(5)
    S = rng.integers(-4, 2, (21, 21))
    S = np.triu(S) + np.triu(S, 1).T
    S[np.arange(21), np.arange(21)] = rng.integers(2, 6, 21)
    C = rng.integers(1, 5, (21, 21))
    C = np.triu(C, 1) + np.triu(C, 1).T
    return (alignment(C, 2, gap_open=3), local_alignment(S, 1, gap_open=4), semiglobal_alignment(S, 2), fit_alignment(S, 2, gap_open=1))


def _queries(tok):
    Q = tok[[4, 77, 149, 30, 31]].copy()
    Q[1, 3:6] = 0
    return Q


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_align_without_ops_is_align(pg, which):
    P, tok = pg
    op = _operators()[which]
    G = P.build_graph(k=3, distance=op, output="csr")
    full, got = P.align(G, distance=op), P.align(G, distance=op, ops=False)
    assert len(got) == len(full) == 450 and got.ops is None and got.score.is_cuda
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(full, f)), f
    assert torch.equal(got.identity(), full.identity())
    with pytest.raises(ValueError, match="built without ops"):
        got.cigar(0)
    Q = _queries(tok)
    R = P.search(Q, k=4, distance=op, output="csr")
    full, got = P.align(R, queries=Q, distance=op), P.align(R, queries=Q, distance=op, ops=False)
    assert len(got) == 20 and got.ops is None
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(full, f)), f
    # op.align: row p with row p
    X, Y = torch.from_numpy(tok[:70]).cuda(), torch.from_numpy(tok[70:140]).cuda()
    full, got = op.align(X, Y), op.align(X, Y, ops=False)
    assert got.ops is None and all(torch.equal(getattr(got, f), getattr(full, f)) for f in FIELDS)


def _host_filter(g, tb, t, min_columns=0):
    """The cut on the host from the unfiltered graph and its full alignments: (rows, cols, weights) of the survivors."""
    if isinstance(g, KNNGraph):
        g = g.as_csr()
    ip, c, w = g.indptr.cpu().numpy(), g.indices.cpu().numpy(), g.weights.cpu().numpy()
    r = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
    n_ops, ident = tb.n_ops.cpu().numpy(), tb.identities.cpu().numpy()
    assert len(n_ops) == len(c) and (c >= 0).all()
    keep = (n_ops >= min_columns) & (ident.astype(np.float64) / np.maximum(n_ops, 1).astype(np.float64) >= t)
    return r[keep], c[keep], w[keep], len(c)


def _same_graph(F, want, nrows):
    assert isinstance(F, CSRGraph) and F.nrows == nrows and F.indptr.is_cuda
    ip = F.indptr.cpu().numpy()
    assert np.array_equal(np.repeat(np.arange(nrows), np.diff(ip)), want[0])
    assert np.array_equal(F.indices.cpu().numpy(), want[1]) and np.array_equal(F.weights.cpu().numpy(), want[2])
    assert 0 < len(want[0]) < want[3]                                       # both sides of the cut are non-empty


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_min_identity_is_the_host_filter(pg, which):
    P, tok = pg
    op = _operators()[which]
    G = P.build_graph(k=3, distance=op, output="csr")
    tb = P.align(G, distance=op)
    t = float(np.median(tb.identity().cpu().numpy()))
    want = _host_filter(G, tb, t)
    F = P.build_graph(k=3, distance=op, output="csr", min_identity=t)
    _same_graph(F, want, 150)
    tuples = P.build_graph(k=3, distance=op, min_identity=t)
    assert [len(e[0]) for e in tuples] == np.bincount(want[0], minlength=150).tolist()
    assert np.array_equal(np.concatenate([e[0] for e in tuples]), want[1])
    Q = _queries(tok)
    eps = 3 if which == 0 else 20
    R = P.search(Q, eps=eps, distance=op, output="csr")
    tb = P.align(R, queries=Q, distance=op)
    t = float(np.median(tb.identity().cpu().numpy()))
    _same_graph(P.search(Q, eps=eps, distance=op, output="csr", min_identity=t), _host_filter(R, tb, t), 5)
