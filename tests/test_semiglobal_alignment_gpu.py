"""
Semi-global alignment scores on the GPU: `pg_alignment_semiglobal_dense` (prograph_amd/csrc/pg_aln_semiglobal.hip), the
operator and the graph / search routes, every entry against `definition` of tests/semiglobal_testdata.py (the recurrence
as a numpy double loop, held against a brute force over the worded definition in tests/test_semiglobal_alignment_cpu.py).
"""
import functools
import operator

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import load_golden
from semiglobal_testdata import csr_of, definition, knn_of, lengths, rows_of, score_table
from prograph_amd import _native, synth
from prograph_amd.distance import semiglobal_alignment

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

LENS = (0, 1, 15, 16, 17, 33, 127, 128)         # sequence lengths: around the 16-score read and the chunk counts
GAPS = ((1, 0), (3, 11), (2, 1), (255, 255))


def dense(S, gap, gap_open, X, Y, out_bytes=8, rows=None):
    a = len(S)
    xo = _native.aln_operand(torch.from_numpy(np.ascontiguousarray(X.astype(np.uint8))), a)
    yo = _native.aln_operand(torch.from_numpy(np.ascontiguousarray(Y.astype(np.uint8))), a)
    out = _native.alignment_semiglobal_dense(xo, yo, _native.aln_local_score(S), gap, gap_open, out_bytes=out_bytes, rows=rows)
    assert xo.valid() and yo.valid()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def shapes(a):
    """The operands of the dense cases for an alphabet of `a` symbols, built once: (name, X, Y)."""
    rng = np.random.default_rng(a)
    every = rows_of(rng, a, list(LENS) * 9 + [128, 64, 3], 128)                # 75 columns: every length, several times
    ylens = rows_of(rng, a, list(LENS) + [40], 128)                          # 9 rows: two workgroups of Y rows
    every[8:16] = ylens[:8]                                                   # equal pairs of every length
    every[20, :33] = ylens[6, 60:93]                                          # a fragment of a long row
    every[21, :33] = ylens[6, 94:127]                                         # its end
    every[22, :50] = np.concatenate([rng.integers(1, a, 17), ylens[6, :33]])  # ends as the long row begins
    lanes = rows_of(rng, a, list(rng.permutation(129)) + [77], 128)           # 130 columns: every lane its own length
    lanes[::5, 3] = 0                                                         # interior zeros (and shorter rows where l <= 4)
    many_x = rows_of(rng, a, rng.integers(0, 41, 600), 40)                    # 600 columns: three column tiles, the last partial
    many_y = rows_of(rng, a, rng.integers(0, 34, 70), 33)                     # 70 rows: nine workgroups, the last partial
    many_x[::7, 5], many_y[::3, 2] = 0, 0
    many_x[100:170, :33] = many_y                                             # something to find
    return (("every length", every, ylens), ("a lane a length", lanes, rows_of(rng, a, [128, 100, 17], 128)),
            ("70 x 600", many_x, many_y), ("1 x 1", rows_of(rng, a, [9], 9), rows_of(rng, a, [12], 12)))


@functools.lru_cache(maxsize=None)
def table_of(a):
    rng = np.random.default_rng(100 + a)
    S = score_table(rng, a, -11, 4, diag=np.arange(2, 10))
    S[0, :] = S[:, 0] = -2
    S[0, 0] = 3
    return S


@pytest.mark.parametrize("a", [5, 32])
@pytest.mark.parametrize("gap,gap_open", GAPS)
def test_kernel_equals_the_recurrence_on_every_entry(a, gap, gap_open):
    S = table_of(a)
    for name, X, Y in shapes(a):
        want = definition(S, gap, gap_open, X, Y)
        got = dense(S, gap, gap_open, X, Y)
        assert got.shape == want.shape and got.dtype == np.int64
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        assert want.max() > 0 or name == "1 x 1"
    assert lengths(shapes(a)[0][1]).max() == 128 and len(set(lengths(shapes(a)[1][1]))) == 129


@functools.lru_cache(maxsize=None)
def every_y_length():
    """Y rows of every length 0..128 against 130 X rows of mixed lengths, overlaps among them; the recurrence once."""
    rng = np.random.default_rng(77)
    S = score_table(rng, 21, -7, 3, diag=np.arange(2, 9))
    Y = rows_of(rng, 21, list(range(129)), 128)
    X = rows_of(rng, 21, list(rng.integers(0, 129, 120)) + [128, 127, 1, 0, 16, 17, 112, 113, 64, 128], 128)
    for c in range(0, 120, 3):                                    # x ends as a y row begins / begins as it ends / lies inside it
        r = 9 + 3 * c // 3
        l = min(lengths(Y)[r], 30)
        if c % 9 == 0:
            X[c] = 0
            X[c, :20 + l] = np.concatenate([rng.integers(1, 21, 20), Y[r, :l]])
        elif c % 9 == 3:
            X[c, :l] = Y[r, lengths(Y)[r] - l:lengths(Y)[r]]
        else:
            X[c] = 0
            X[c, :l] = Y[r, (lengths(Y)[r] - l) // 2:(lengths(Y)[r] - l) // 2 + l]
    return S, X, Y, definition(S, 2, 3, X, Y)


def test_the_last_column_at_every_position_of_every_chunk_count():
    """len y = 0..128: the pick of column len y inside the last chunk sits at each of its 16 positions for each of the
    eight chunk counts; both operand orders, so that the same lengths also end the outer loop of a lane."""
    S, X, Y, want = every_y_length()
    assert (want > 40).sum() > 100 and np.array_equal(lengths(Y), np.arange(129))
    got = dense(S, 2, 3, X, Y)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    got = dense(S, 2, 3, Y, X)
    assert np.array_equal(got, want.T), np.argwhere(got != want.T)[:5]


@pytest.mark.parametrize("width", [32, 128])
def test_padding_never_scores(width):
    """S[0][0] = 127 and S[a][0] > 0: a kernel that lets a padded cell - past len y in the last chunk, or an outer step past
    a lane's len x - raise a cell that is read reports more than the recurrence."""
    rng = np.random.default_rng(width)
    S = score_table(rng, 6, -9, -1, diag=[1, 2])
    S[0, :] = S[:, 0] = 9
    S[0, 0] = 127
    X = rows_of(rng, 6, [15, 17, 15, 17, 1, 0, width] * 10, width)
    Y = rows_of(rng, 6, [15, 17, 17, 15, 2, 0, 1, 16, width], width)
    X[0, 3] = 0                                                   # a real symbol 0 does score: 9 against any symbol
    for gap, gap_open in ((1, 0), (2, 3)):
        want = definition(S, gap, gap_open, X, Y)
        assert 0 < want.max() < 127                               # no two real zeros to meet
        assert np.array_equal(dense(S, gap, gap_open, X, Y), want)
        assert np.array_equal(dense(S, gap, gap_open, Y, X), want.T)


def test_the_floor_at_work():
    """min(S) = -128, max(S) = 1, 128 positions, unrelated rows: the cells of the recurrence pass -16 000 while the
    kernel's stop at -Z = -128; the scores are the same."""
    rng = np.random.default_rng(6)
    S = np.full((8, 8), -128)
    S[np.arange(8), np.arange(8)] = 1
    X, Y = rows_of(rng, 8, [128] * 60 + [100, 64, 3, 0], 128), rows_of(rng, 8, [128, 128, 127, 90, 128, 17, 128, 128, 128], 128)
    X[:4] = np.arange(128) % 3 + 1                                # nothing in common with
    Y[:2] = np.arange(128) % 3 + 4                                # these: every aligned pair costs 128
    X[5, :40], X[6, 88:] = Y[4, 88:], Y[4, :40]                   # overlaps: 40 at 1 each
    for gap, gap_open in ((255, 255), (1, 0), (100, 7)):
        want = definition(S, gap, gap_open, X, Y)
        assert want[0, 0] == 0 and want[4, 5] >= 40 and want[4, 6] >= 40 and want.max() < 128
        assert np.array_equal(dense(S, gap, gap_open, X, Y), want)
        assert np.array_equal(dense(S, gap, gap_open, Y, X), want.T)


def test_the_largest_score_fp16_and_a_row_range():
    S = np.full((32, 32), -128)
    S[np.arange(32), np.arange(32)] = 127
    rng = np.random.default_rng(1)
    X = rows_of(rng, 32, [128, 128, 100, 64], 128)
    X[1] = X[0]
    X[2, :100] = X[0, 28:]
    got = dense(S, 255, 255, X, X)
    assert got[0, 1] == got[0, 0] == 16256 == 128 * 127 and got[0, 2] == 100 * 127      # a cell of 2 Z + 255 = 32 767 on the way
    assert np.array_equal(got, definition(S, 255, 255, X, X))
    # fp16 blocks are the int64 scores while they stay within 2048: 128 positions at 16 a symbol
    S = score_table(rng, 21, -7, 3, diag=[8, 12, 16])
    S[7, 7] = 16
    X = rows_of(rng, 21, list(rng.integers(0, 129, 298)) + [128, 128], 128)
    X[298:] = 7                                                   # 128 symbols at 16 each
    Y = X[[298, 5, 17, 40, 41, 42, 43, 44, 45, 46, 200]]
    full = dense(S, 4, 6, X, Y)
    assert full.max() == 2048 == 128 * 16 and np.array_equal(full, definition(S, 4, 6, X, Y))
    half = dense(S, 4, 6, X, Y, out_bytes=2)
    assert half.dtype == np.float16 and np.array_equal(half.astype(np.int64), full)
    part = dense(S, 4, 6, X, Y, out_bytes=2, rows=(3, 10))
    assert part.shape == (7, 300) and np.array_equal(part, half[3:10])
    assert np.array_equal(dense(S, 4, 6, X, Y, rows=(10, 11)), full[10:11])


def test_operator_on_the_device_equals_the_host():
    rng = np.random.default_rng(2)
    S = score_table(rng, 21, -6, 3, diag=np.arange(3, 9))
    X, Y = rows_of(rng, 21, rng.integers(0, 61, 90), 60), rows_of(rng, 21, rng.integers(0, 45, 13), 44)
    X[::6, 4] = 0
    r, l = int(np.argmax(lengths(Y))), int(lengths(Y).max())
    X[7, :20] = Y[r, l - 20:l]                                    # begins as the longest row ends
    for gap, gap_open in ((2, 0), (1, 7)):
        op = semiglobal_alignment(S, gap, gap_open)
        host = op(torch.from_numpy(X), torch.from_numpy(Y))
        dev = op(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
        assert dev.is_cuda and dev.dtype == torch.int64 and torch.equal(dev.cpu(), host)
        assert np.array_equal(host.numpy(), definition(S, gap, gap_open, X, Y))
    with pytest.raises(ValueError):
        op(torch.from_numpy(X).cuda(), torch.tensor([[1, 21]]).cuda())        # a token outside the table
    with pytest.raises(ValueError):
        op(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), similarity=False)


def _prograph(tmp, tok, name):
    from prograph_amd import Prograph
    f = tmp / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P


def _arrays(got):
    return np.array([i for i, _ in got]), np.array([w for _, w in got])


def _same_csr(got, ip, ix, w):
    assert len(got) == len(ip) - 1
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]]), i


@functools.lru_cache(maxsize=None)
def varlen():
    """The N = 300 variable-length set, a score table and gaps, and the recurrence over all pairs: computed once."""
    tok = load_golden("synth_n300_varlen24")["tokens"].astype(np.int64)
    S = score_table(np.random.default_rng(9), 21, -4, 1, diag=np.arange(2, 6))
    return tok, S, definition(S, 3, 2, tok, tok)


def test_graphs_equal_a_stable_descending_sort_of_the_recurrence(tmp_path):
    tok, S, D = varlen()
    P = _prograph(tmp_path, tok, "varlen24")
    op = semiglobal_alignment(S, 3, 2)
    for k in (5, 70):
        G = P.build_graph(k=k, distance=op, output="csr")
        wi, wd = knn_of(D, k, 1)
        assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.similarity is False
        assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    gi, gw = _arrays(P.build_graph(k=5, distance=op, similarity=True))          # not consulted
    assert gw.dtype == np.int64 and np.array_equal(gi, knn_of(D, 5, 1)[0]) and np.array_equal(gw, knn_of(D, 5, 1)[1])
    mid = int(np.median(D[D > 0]))
    for comp, eps in ((operator.le, mid), (operator.lt, mid + 2.5), (operator.eq, mid), (operator.ge, 4), (operator.gt, 3.5)):
        G = P.build_graph(eps=eps, distance=op, comp=comp, output="csr")
        ip, ix, w = csr_of(D, comp, eps, diagonal=False)
        assert G.weights.dtype == torch.int16 and ip[-1] > 0 and np.array_equal(G.indptr.cpu().numpy(), ip)
        assert np.array_equal(G.indices.cpu().numpy(), ix) and np.array_equal(G.weights.cpu().numpy(), w)
    sub = np.arange(40, 300, 3)
    _same_csr(P.build_graph(eps=mid, distance=op, idxs=sub), *csr_of(D[np.ix_(sub, sub)], operator.le, mid, diagonal=False))
    P.build_graph(k=4, distance=op, store="Overlap", output="csr")
    assert np.array_equal(P.degree("Overlap"), knn_of(D, 4, 1)[1].sum(1).astype(np.float32))


def test_searches_equal_a_stable_descending_sort_of_the_recurrence(tmp_path):
    tok, S, D = varlen()
    P = _prograph(tmp_path, tok, "varlen24")
    op = semiglobal_alignment(S, 3, 2)
    rng = np.random.default_rng(5)
    Q = np.zeros((9, 33), dtype=np.int64)                         # wider than the dataset
    Q[:, :24] = tok[[0, 17, 40, 99, 150, 151, 222, 298, 299]]
    Q[3, 24:31] = rng.integers(1, 21, 7)
    Q[5, 9:] = 0
    Q[6] = 0
    Q[6, :12] = tok[222, 6:18]                                    # a fragment of a dataset row
    DQ = definition(S, 3, 2, tok, Q)
    for k in (5, 70):
        G = P.search(Q, k=k, distance=op, output="csr")
        wi, wd = knn_of(DQ, k, 0)
        assert G.first == 0 and np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    assert knn_of(DQ, 1, 0)[0][0, 0] == 0
    mid = int(np.median(DQ[DQ > 0]))
    for comp, eps in ((operator.le, mid), (operator.gt, mid + 0.5), (operator.eq, mid)):
        _same_csr(P.search(Q, eps=eps, distance=op, comp=comp), *csr_of(DQ, comp, eps))
    hit, best = P.nearest_neighbour(synth.tokens_to_strings(tok[40:41])[0], distance=op)
    assert list(hit.index) == [int(knn_of(DQ, 1, 0)[0][2, 0])] and best == DQ[2].max()


def test_the_torch_side_beyond_the_fp16_bound(tmp_path):
    """128 positions at 17 a symbol: 2176 > 2048, so the selection runs in torch over the operator's int64 blocks."""
    rng = np.random.default_rng(13)
    S = score_table(rng, 21, -5, 2, diag=[3, 4, 17])
    tok = rows_of(rng, 21, list(rng.integers(90, 129, 38)) + [128, 128], 128)
    tok[39] = tok[38]
    tok[5, :40] = tok[38, 88:]
    P = _prograph(tmp_path, tok, "wide")
    op = semiglobal_alignment(S, 2, 1)
    assert 128 * op.max_score == 2176 and not P._local_native(128, op) and P._local_native(128, semiglobal_alignment(np.minimum(S, 16), 2, 1))
    D = definition(S, 2, 1, tok, tok)
    G = P.build_graph(k=3, distance=op, output="csr")
    wi, wd = knn_of(D, 3, 1)
    assert G.dist.dtype == torch.int64 and np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    _same_csr(P.build_graph(eps=40, distance=op), *csr_of(D, operator.le, 40, diagonal=False))
    gi, gw = _arrays(P.search(tok[[38, 5]], k=2, distance=op))
    assert np.array_equal(gi, knn_of(D[[38, 5]], 2, 0)[0]) and np.array_equal(gw, knn_of(D[[38, 5]], 2, 0)[1])
    _same_csr(P.search(tok[[38, 5]], eps=40, distance=op), *csr_of(D[[38, 5]], operator.le, 40))
