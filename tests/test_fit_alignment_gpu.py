"""
Fit alignment scores on the GPU: `pg_alignment_fit_dense` (prograph_amd/csrc/pg_aln_fit.hip), the operator, the graph /
search routes with their shifted blocks, and the tracebacks, every entry against `definition` / `canonical` of
tests/fit_testdata.py (the recurrence as a numpy double loop, held against a brute force over the worded definition in
tests/test_fit_alignment_cpu.py).  Every comparison is exact.
"""
import functools
import operator

import numpy as np
import pandas as pd
import pytest
import torch

from fit_testdata import canonical, definition, fragments, lengths, rows_of, score_table, seq
from local_testdata import csr_of, knn_of
from prograph_amd import _native, synth
from prograph_amd.distance import fit_alignment

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

LENS = (0, 1, 15, 16, 17, 33, 127, 128)         # sequence lengths: around the 16-score read and the chunk counts
GAPS = ((1, 0), (3, 11), (2, 1), (255, 255))


def dense(S, gap, gap_open, X, Y, out_bytes=8, rows=None, bias=0):
    a = len(S)
    xo = _native.aln_operand(torch.from_numpy(np.ascontiguousarray(X.astype(np.uint8))), a)
    yo = _native.aln_operand(torch.from_numpy(np.ascontiguousarray(Y.astype(np.uint8))), a)
    assert _native.aln_fit_fits(xo.l, yo.l, int(np.max(S)), gap, gap_open)
    out = _native.alignment_fit_dense(xo, yo, _native.aln_local_score(S), gap, gap_open, out_bytes=out_bytes, rows=rows, bias=bias)
    assert xo.valid() and yo.valid()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def shapes(a):
    """The operands of the dense cases for an alphabet of `a` symbols, built once: (name, X, Y)."""
    rng = np.random.default_rng(a)
    every = rows_of(rng, a, list(LENS) * 9 + [128, 64, 3], 128)                # 75 columns: every length, several times
    ylens = rows_of(rng, a, list(LENS) + [40], 128)                          # 9 rows: two workgroups of Y rows
    every[8:16] = ylens[:8]                                                   # equal pairs of every length
    every[20, :100] = np.concatenate([rng.integers(1, a, 30), ylens[5, :33], rng.integers(1, a, 37)])    # holds a whole y row
    every[21, :60] = np.concatenate([rng.integers(1, a, 20), ylens[8, :40]])  # ... at its end
    every[22, :33] = ylens[6, 60:93]                                          # a fragment of a y row: len y > len x
    lanes = rows_of(rng, a, list(rng.permutation(129)) + [77], 128)           # 130 columns: every lane its own length
    lanes[::5, 3] = 0                                                         # interior zeros (and shorter rows where l <= 4)
    lane_y = rows_of(rng, a, [128, 100, 17], 128)
    lanes[7, :] = 0
    lanes[7, :117] = np.concatenate([rng.integers(1, a, 9), lane_y[1, :100], rng.integers(1, a, 8)])
    many_x = rows_of(rng, a, rng.integers(0, 41, 600), 40)                    # 600 columns: three column tiles, the last partial
    many_y = rows_of(rng, a, rng.integers(0, 34, 70), 33)                     # 70 rows: nine workgroups, the last partial
    many_x[::7, 5], many_y[::3, 2] = 0, 0
    many_x[100:170, 4:37] = many_y                                            # something to find
    return (("every length", every, ylens), ("a lane a length", lanes, lane_y),
            ("70 x 600", many_x, many_y), ("1 x 1", rows_of(rng, a, [12], 12), rows_of(rng, a, [9], 9)))


@functools.lru_cache(maxsize=None)
def table_of(a):
    rng = np.random.default_rng(100 + a)
    S = score_table(rng, a, -11, 4, diag=np.arange(2, 10))
    S[0, :] = S[:, 0] = -2
    S[0, 0] = 3
    S[1, 1] = 9
    return S


@pytest.mark.parametrize("a", [5, 32])
@pytest.mark.parametrize("gap,gap_open", GAPS)
def test_kernel_equals_the_recurrence_on_every_entry(a, gap, gap_open):
    S = table_of(a)
    assert S.max() == 9 and 255 + 128 * (255 + 2 * 9) + 255 == 35454 <= _native.ALN_LONG_CELL_MAX
    for name, X, Y in shapes(a):
        want = definition(S, gap, gap_open, X, Y)
        got = dense(S, gap, gap_open, X, Y)
        assert got.shape == want.shape and got.dtype == np.int64
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
        if name != "1 x 1":
            assert want.max() > 0 and want.min() < 0                          # contained rows, and rows longer than their column
    assert lengths(shapes(a)[0][1]).max() == 128 and len(set(lengths(shapes(a)[1][1]))) >= 120


@functools.lru_cache(maxsize=None)
def every_y_length():
    """Y rows of every length 0..128 against 130 X rows of mixed lengths, some of which hold a Y row; the recurrence once."""
    rng = np.random.default_rng(77)
    S = score_table(rng, 21, -7, 3, diag=np.arange(2, 9))
    Y = rows_of(rng, 21, list(range(129)), 128)
    X = rows_of(rng, 21, list(rng.integers(0, 129, 120)) + [128, 127, 1, 0, 16, 17, 112, 113, 64, 128], 128)
    for c in range(0, 120, 3):                                    # x holds y row r after a head / is a piece of it / is it
        r = 9 + c
        l = int(lengths(Y)[r])
        X[c] = 0
        if c % 9 == 0:
            head = min(20, 128 - l)
            X[c, :head + l] = np.concatenate([rng.integers(1, 21, head), Y[r, :l]])
        elif c % 9 == 3:
            X[c, :l // 2] = Y[r, l // 4:l // 4 + l // 2]
        else:
            X[c, :l] = Y[r, :l]
    return S, X, Y, definition(S, 2, 3, X, Y)


def test_the_last_column_at_every_position_of_every_chunk_count():
    """len y = 0..128: the pick of column len y inside the last chunk sits at each of its 16 positions for each of the
    eight chunk counts, and row 0 ends at each of them; int64, and fp16 with the selection's shift."""
    S, X, Y, want = every_y_length()
    assert (want > 40).sum() > 15 and (want < 0).sum() > 1000 and np.array_equal(lengths(Y), np.arange(129))
    got = dense(S, 2, 3, X, Y)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    K = 3 + 2 * 128
    assert want.min() == -K and K + 128 * int(S.max()) <= 2048
    half = dense(S, 2, 3, X, Y, out_bytes=2, bias=K)
    assert half.dtype == np.float16 and np.array_equal(half.astype(np.int64), want + K)
    part = dense(S, 2, 3, X, Y, out_bytes=2, rows=(3, 100), bias=K)
    assert part.shape == (97, 130) and np.array_equal(part, half[3:100])
    assert np.array_equal(dense(S, 2, 3, X, Y, rows=(128, 129), bias=7), want[128:129] + 7)


@pytest.mark.parametrize("width", [32, 128])
def test_padding_never_scores(width):
    """S[0][0] = 127 and S[a][0] > 0: a kernel that lets a padded cell - past len y in the last chunk, or an outer step past
    a lane's len x - reach the result reports more than the recurrence."""
    rng = np.random.default_rng(width)
    S = score_table(rng, 6, -9, -1, diag=[1, 2])
    S[0, :] = S[:, 0] = 9
    S[0, 0] = 127
    X = rows_of(rng, 6, [15, 17, 15, 17, 1, 0, width] * 10, width)
    Y = rows_of(rng, 6, [15, 17, 17, 15, 2, 0, 1, 16, width], width)
    X[0, 3] = 0                                                   # a real symbol 0 does score: 9 against any symbol
    for gap, gap_open in ((1, 0), (2, 3)):
        want = definition(S, gap, gap_open, X, Y)
        assert want.max() < 127                                   # no two real zeros to meet
        assert np.array_equal(dense(S, gap, gap_open, X, Y), want)
        assert np.array_equal(dense(S, gap, gap_open, Y, X), definition(S, gap, gap_open, Y, X))


def test_the_floor_at_work():
    """min(S) = -128, max(S) = 1, 128 positions, unrelated rows: cells of the recurrence pass -16 000 while the kernel's
    stop at -Z; the scores, all of y unaligned among them, are the same."""
    rng = np.random.default_rng(6)
    S = np.full((8, 8), -128)
    S[np.arange(8), np.arange(8)] = 1
    X, Y = rows_of(rng, 8, [128] * 60 + [100, 64, 3, 0], 128), rows_of(rng, 8, [128, 128, 127, 90, 128, 17, 128, 128, 40], 128)
    X[:4] = np.arange(128) % 3 + 1                                # nothing in common with
    Y[:2] = np.arange(128) % 3 + 4                                # these: every aligned pair costs 128
    X[5, 50:90] = Y[8, :40]                                       # holds row 8
    for gap, gap_open in ((255, 0), (1, 0), (100, 7)):
        want = definition(S, gap, gap_open, X, Y)
        assert want[0, 0] == max(-(gap_open + 128 * gap), -128 * 128) and want[8, 5] == 40 and want.max() < 128
        assert np.array_equal(dense(S, gap, gap_open, X, Y), want)


def test_outside_the_cells_the_operator_falls_back_and_stays_exact(monkeypatch):
    """128 positions at 255 / 255 / 127: 255 + 128 * (255 + 254) + 255 = 65 662 > 65 535.  One position fewer fits."""
    S = np.full((4, 4), -128)
    S[np.arange(4), np.arange(4)] = 127
    rng = np.random.default_rng(3)
    X, Y = rows_of(rng, 4, [128, 128, 60, 0, 128], 128), rows_of(rng, 4, [128, 30, 0], 128)
    X[1], X[2, :60] = Y[0], np.concatenate([rng.integers(1, 4, 15), Y[1, :30], rng.integers(1, 4, 15)])
    assert not _native.aln_fit_fits(128, 128, 127, 255, 255) and _native.aln_fit_fits(127, 127, 127, 255, 255)
    op = fit_alignment(S, 255, 255)
    want = definition(S, 255, 255, X, Y)
    assert want[0, 1] == 128 * 127 and want[1, 2] == 30 * 127 and want[0, 3] == -(255 + 128 * 255)
    calls = []
    real = _native.alignment_fit_dense
    monkeypatch.setattr(_native, "alignment_fit_dense", lambda *a, **k: calls.append(1) or real(*a, **k))
    got = op(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
    assert got.is_cuda and not calls and np.array_equal(got.cpu().numpy(), want)
    got = op(torch.from_numpy(X[:, :127]).cuda(), torch.from_numpy(Y[:, :127]).cuda())          # just inside: the kernel
    assert calls and np.array_equal(got.cpu().numpy(), definition(S, 255, 255, X[:, :127], Y[:, :127]))


def test_operator_on_the_device_equals_the_host():
    rng = np.random.default_rng(2)
    S = score_table(rng, 21, -6, 3, diag=np.arange(3, 9))
    X, Y = rows_of(rng, 21, rng.integers(0, 61, 90), 60), rows_of(rng, 21, rng.integers(0, 45, 13), 44)
    X[::6, 4] = 0
    r, l = int(np.argmax(lengths(Y))), int(lengths(Y).max())
    X[7, :] = 0
    X[7, 5:5 + l] = Y[r, :l]                                      # holds the longest row
    for gap, gap_open in ((2, 0), (1, 7)):
        op = fit_alignment(S, gap, gap_open)
        host = op(torch.from_numpy(X), torch.from_numpy(Y))
        dev = op(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
        assert dev.is_cuda and dev.dtype == torch.int64 and torch.equal(dev.cpu(), host)
        assert np.array_equal(host.numpy(), definition(S, gap, gap_open, X, Y)) and host.min() < 0 < host.max()
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
def family():
    """288 rows of lengths 1..128 (a dataset has no empty sequence; the queries below have one) - parents and fragments
    cut from them -, a table, gaps, and the recurrence over all pairs: computed once."""
    rng = np.random.default_rng(9)
    tok = fragments(rng, 21, 288, 128, least=1)
    tok[0, :] = rng.integers(1, 21, 128)                          # the width is 128
    tok[2], tok[2, 0] = 0, 5                                      # one symbol
    S = score_table(rng, 21, -4, 1, diag=np.arange(2, 6))
    return tok, S, definition(S, 1, 2, tok, tok)


def test_graphs_equal_a_stable_descending_sort_of_the_recurrence(tmp_path):
    tok, S, D = family()
    assert set(lengths(tok)) >= {1, 128} and D.min() <= -(2 + 128) + 5 and (D < 0).mean() > 0.3 and not np.array_equal(D, D.T)
    P = _prograph(tmp_path, tok, "family")
    op = fit_alignment(S, 1, 2)
    assert P._local_native(128, op, 128) and op._select_bias(128) == 130
    for k in (5, 70):
        G = P.build_graph(k=k, distance=op, output="csr")
        wi, wd = knn_of(D, k, 1)
        assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.similarity is False
        assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    assert (knn_of(D, 70, 1)[1] < 0).any()                                        # negative ranks, ranked
    gi, gw = _arrays(P.build_graph(k=5, distance=op, similarity=True))          # not consulted
    assert gw.dtype == np.int64 and np.array_equal(gi, knn_of(D, 5, 1)[0]) and np.array_equal(gw, knn_of(D, 5, 1)[1])
    mid = int(np.median(D[D > 0]))
    for comp, eps in ((operator.le, mid), (operator.lt, mid + 2.5), (operator.eq, mid), (operator.ge, 4), (operator.gt, 3.5),
                      (operator.le, -3), (operator.ge, -3)):
        G = P.build_graph(eps=eps, distance=op, comp=comp, output="csr")
        ip, ix, w = csr_of(D, comp, eps, diagonal=False)
        assert G.weights.dtype == torch.int16 and (ip[-1] > 0 or comp is operator.ge) and np.array_equal(G.indptr.cpu().numpy(), ip)
        assert np.array_equal(G.indices.cpu().numpy(), ix) and np.array_equal(G.weights.cpu().numpy(), w)
    sub = np.arange(40, 288, 3)
    _same_csr(P.build_graph(eps=mid, distance=op, idxs=sub), *csr_of(D[np.ix_(sub, sub)], operator.le, mid, diagonal=False))
    P.build_graph(k=4, distance=op, store="Fit", output="csr")
    assert np.array_equal(P.degree("Fit"), knn_of(D, 4, 1)[1].sum(1).astype(np.float32))


def test_searches_equal_a_stable_descending_sort_of_the_recurrence(tmp_path):
    tok, S, D = family()
    P = _prograph(tmp_path, tok, "family")
    op = fit_alignment(S, 1, 2)
    rng = np.random.default_rng(5)
    Q = np.zeros((9, 60), dtype=np.int64)                         # narrower than the dataset: K follows the queries' width
    Q[:, :40] = tok[[0, 17, 40, 99, 150, 151, 222, 286, 287], 20:60]
    Q[3, 40:47] = rng.integers(1, 21, 7)
    Q[5, 9:] = 0
    Q[6] = 0
    DQ = definition(S, 1, 2, tok, Q)
    assert DQ.min() < 0 < DQ.max() and op._select_bias(60) == 62
    for k in (5, 70, 288):
        G = P.search(Q, k=k, distance=op, output="csr")
        wi, wd = knn_of(DQ, k, 0)
        assert G.first == 0 and G.dist.dtype == torch.int16
        assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    mid = int(np.median(DQ[DQ > 0]))
    for comp, eps in ((operator.le, mid), (operator.gt, mid + 0.5), (operator.eq, mid), (operator.ge, -50), (operator.lt, 7)):
        _same_csr(P.search(Q, eps=eps, distance=op, comp=comp), *csr_of(DQ, comp, eps))
    hit, best = P.nearest_neighbour(synth.tokens_to_strings(tok[0:1, 20:60])[0], distance=op)
    q = definition(S, 1, 2, tok, tok[0:1, 20:60])
    assert list(hit.index) == [int(knn_of(q, 1, 0)[0][0, 0])] and best == q.max()


def test_every_rank_of_forty_rows_negative_ones_among_them(tmp_path):
    """k = N - 1 at N = 40: every other row is ranked, most of them below 0, in the order of the unshifted scores."""
    rng = np.random.default_rng(40)
    tok = fragments(rng, 21, 40, 64, least=1)
    tok[0, :] = rng.integers(1, 21, 64)
    S = score_table(rng, 21, -6, 2, diag=[3, 4, 5])
    D = definition(S, 3, 11, tok, tok)
    P = _prograph(tmp_path, tok, "forty")
    op = fit_alignment(S, 3, 11)
    G = P.build_graph(k=39, distance=op, output="csr")
    wi, wd = knn_of(D, 39, 1)
    assert (wd < 0).mean() > 0.3 and (wd > 0).any()
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)


def test_tracebacks_equal_the_canonical_alignment(tmp_path):
    """`op.align` (row p of Y whole within row p of X) and `Prograph.align` over a graph's edges and a search's hits: every
    field and every code of `canonical`, and the score is the edge's weight."""
    tok, S, D = family()
    op = fit_alignment(S, 1, 2)
    rng = np.random.default_rng(8)
    xi, yi = rng.integers(0, 288, 150), rng.integers(0, 288, 150)
    xi[:3], yi[:3] = (0, 2, 5), (2, 0, 5)                          # one symbol in 128, 128 in one symbol, a row against itself
    A = op.align(torch.from_numpy(tok[xi]).cuda(), torch.from_numpy(tok[yi]).cuda()).host()

    def same(A, p, x, y, weight=None):
        want = canonical(S, 1, 2, seq(x), seq(y))
        got = tuple(int(getattr(A, f)[p]) for f in ("score", "x_begin", "x_end", "y_begin", "y_end", "n_ops", "identities"))
        assert got == want[:7] and A.ops[p, :want[5]].tolist() == want[7] and not A.ops[p, want[5]:].any(), (p, got, want)
        assert weight is None or want[0] == weight

    for p in range(150):
        same(A, p, tok[xi[p]], tok[yi[p]])
        assert int(A.score[p]) == D[yi[p], xi[p]] and int(A.y_begin[p]) == 0 and int(A.y_end[p]) == lengths(tok)[yi[p]]
    P = _prograph(tmp_path, tok, "family")
    G = P.build_graph(k=3, distance=op, output="csr")
    A = P.align(G, distance=op).host()
    idx, w = G.idx.cpu().numpy(), G.dist.cpu().numpy()
    assert len(A) == 288 * 3
    for p in range(0, 288 * 3, 5):
        r, c = p // 3, int(idx[p // 3, p % 3])
        same(A, p, tok[c], tok[r], int(w[p // 3, p % 3]))           # x: the containing column, y: the row
    Q = tok[[17, 40, 99], 20:60]
    H = P.search(Q, k=4, distance=op, output="csr")
    A = P.align(H, queries=Q, distance=op).host()
    hi, hw = H.idx.cpu().numpy(), H.dist.cpu().numpy()
    for p in range(12):
        same(A, p, tok[int(hi[p // 4, p % 4])], Q[p // 4], int(hw[p // 4, p % 4]))
