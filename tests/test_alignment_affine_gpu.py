"""
Affine gap penalties of the alignment distance on the GPU: `pg_alignment_affine_dense` on every entry against the
three-table recurrence of tests/test_alignment_affine_cpu.py (`definition`, which that file holds against a brute force
over alignment paths), the operator, and `build_graph` / `search` with `distance=alignment(C, gap, gap_open=o)` against a
stable sort / nonzero of the same definition.  Every comparison is an every-entry equality.
"""
import operator

import numpy as np
import pandas as pd
import pytest
import torch

from prograph_amd import synth
from prograph_amd.distance import alignment
from test_alignment_affine_cpu import csr_of, definition, knn_of, lengths, rows_of, table

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

OPS = {"le": operator.le, "lt": operator.lt, "eq": operator.eq, "ge": operator.ge, "gt": operator.gt}
LENS = (0, 1, 15, 16, 17, 33, 127, 128)       # sequence lengths: around the 16-cost read and every chunk count's edge


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def operands(nat, a, X, Y):
    xo = nat.aln_operand(torch.from_numpy(np.ascontiguousarray(X).astype(np.uint8)), a)
    yo = nat.aln_operand(torch.from_numpy(np.ascontiguousarray(Y).astype(np.uint8)), a)
    assert xo.valid() and yo.valid()
    return xo, yo


def dense(nat, C, gap, gap_open, X, Y, **kw):
    xo, yo = operands(nat, len(C), X, Y)
    return nat.alignment_affine_dense(xo, yo, nat.sub_cost(C), gap, gap_open, **kw)


# ---------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("gap,gap_open", [(1, 0), (1, 11), (7, 3), (255, 255), (1, 255)])
@pytest.mark.parametrize("a", [21, 32])
def test_kernel_against_the_definition(nat, a, gap, gap_open):
    """Row r of either operand has length LENS[r % 8], so any window of 8 rows holds every length and every pair of
    lengths meets: the empty row and instances 1, 2, 3 and 8 of the row routine (NC = ceil(len y / 16)), positions 1, 15
    and 16 of a chunk.  Instances 4 to 7 and the other positions of the result select are run by
    tests/test_alignment_lengths_gpu.py, on a row of every length 0..128.  The definition is evaluated once on 77 x 607
    pairs and every (rows, columns) shape - partial row groups, partial column tiles, more than one tile - is a window
    of it, from every offset 0..7."""
    rng = np.random.default_rng(1000 * a + 10 * gap + gap_open)
    C = table(rng, a, np.arange(256))
    C[1, a - 1] = C[a - 1, 1] = 255
    Xall = rows_of(rng, a, [LENS[r % 8] for r in range(607)], 128)
    Yall = rows_of(rng, a, [LENS[(r + 3) % 8] for r in range(77)], 128)
    want = definition(C, gap, gap_open, Xall, Yall)
    width = lambda T: max(1, int(lengths(T).max()))              # the operands go in at their own widths
    for M in (1, 15, 17, 70):
        for N in (1, 63, 65, 257, 600):
            for o in range(8):
                for p in (range(8) if N == 1 else [(5 * o + 1) % 8]):
                    X, Y = Xall[p:p + N], Yall[o:o + M]
                    got = dense(nat, C, gap, gap_open, X[:, :width(X)], Y[:, :width(Y)])
                    assert got.dtype == torch.int64 and got.shape == (M, N)
                    assert np.array_equal(got.cpu().numpy(), want[o:o + M, p:p + N]), (a, gap, gap_open, M, N, o, p)
    got = dense(nat, C, gap, gap_open, Xall, Yall)                            # and both at the full width, zero padded
    assert np.array_equal(got.cpu().numpy(), want)


def test_kernel_every_lane_its_own_length_and_interior_zeros(nat):
    rng = np.random.default_rng(77)
    C = table(rng, 21, np.arange(256))
    X = rows_of(rng, 21, list(rng.permutation(np.arange(1, 129)))[:64] + list(range(64, 0, -1)), 128)   # two waves
    Y = rows_of(rng, 21, [128, 90, 64, 17, 5, 0, 33, 100, 77], 128)
    assert len(set(lengths(X[:64]))) == 64
    assert np.array_equal(dense(nat, C, 9, 20, X, Y).cpu().numpy(), definition(C, 9, 20, X, Y))
    # interior zeros are symbol 0 of the table; only trailing ones are padding
    X[::3, 2], X[1::5, 0], Y[::2, 4], Y[3, :16] = 0, 0, 0, 0
    X[7, 100:] = 0
    X[7, 110] = 3                                                 # zeros inside, a symbol after them
    want = definition(C, 9, 20, X, Y)
    assert np.array_equal(dense(nat, C, 9, 20, X, Y).cpu().numpy(), want)
    assert lengths(X)[7] == 111 and lengths(Y)[3] == 17


def test_kernel_sixteen_bit_edge(nat):
    """H and E share a dword as unsigned 16-bit halves.  At gap = gap_open = 255 and substitution cost 255 the distances
    pass 32 767, where a signed or saturating packed operation would show: 128 symbols against one is a pair and one run
    of 127, 255 + 255 + 127 * 255 = 32 895, reached through E (the long operand in X) and through F (the long one in Y)
    with every value of the run's tail above 32 767."""
    C = np.zeros((21, 21), dtype=np.int64)
    C[3, 7] = C[7, 3] = 255
    X, Y = np.full((70, 128), 3), np.full((9, 128), 7)
    Y[1, 1:] = 0                                                  # a single 7: the run is in X, carried by E
    X[5, 1:] = 0                                                  # a single 3: the run is in Y, carried by F
    X[6, :] = 0                                                   # empty
    want = definition(C, 255, 255, X, Y)
    assert want[0, 0] == 128 * 255 and want[1, 0] == 32895 and want[0, 5] == 32895 and want[1, 5] == 255
    assert want[0, 6] == 32895 and want.max() == 32895 and (want > 32767).sum() >= 70 + 8
    got = dense(nat, C, 255, 255, X, Y)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    # a cheap pair at the far end: the optimal path is one run whose E (F) values pass 32 767 before the last cell
    C2 = C.copy()
    C2[3, 9] = C2[9, 3] = 1
    X2, Y2 = X.copy(), Y.copy()
    Y2[2, :] = 0
    Y2[2, 0] = 9
    Y2[3, -1] = 9
    want = definition(C2, 255, 255, X2, Y2)
    assert want[2, 0] == 1 + 255 + 127 * 255
    assert np.array_equal(dense(nat, C2, 255, 255, X2, Y2).cpu().numpy(), want)
    assert np.array_equal(dense(nat, C2, 255, 255, Y2, X2).cpu().numpy(), want.T)


def test_kernel_output_types_and_row_range(nat):
    # fp16 equals int64 up to d = 2048 exactly: 64 positions at cost 31 with gap 31 and gap_open 64
    rng = np.random.default_rng(9)
    C = table(rng, 32, np.arange(32))
    C[1, 2] = C[2, 1] = 31
    X, Y = rows_of(rng, 32, rng.integers(1, 65, 300), 64), rows_of(rng, 32, rng.integers(1, 65, 33), 64)
    X[17], Y[4] = 1, 0
    Y[4, 0] = 2                                                   # one pair at 31 and one run of 63: 31 + 64 + 63 * 31
    want = definition(C, 31, 64, X, Y)
    assert want.max() == 2048 and want[4, 17] == 2048
    xo, yo = operands(nat, 32, X, Y)
    cost = nat.sub_cost(C)
    one = nat.alignment_affine_dense(xo, yo, cost, 31, 64)
    assert one.dtype == torch.int64 and np.array_equal(one.cpu().numpy(), want)
    h = nat.alignment_affine_dense(xo, yo, cost, 31, 64, out_bytes=2)
    assert h.dtype == torch.float16 and np.array_equal(h.cpu().numpy().astype(np.int64), want)
    for ob in (8, 2):
        rows = nat.alignment_affine_dense(xo, yo, cost, 31, 64, out_bytes=ob, rows=(3, 19))        # a Y operand from row 3 on
        assert rows.shape == (16, 300) and np.array_equal(rows.cpu().numpy().astype(np.int64), want[3:19])


def test_gap_open_zero_is_the_linear_kernel(nat):
    rng = np.random.default_rng(31)
    C = table(rng, 21, np.arange(256))
    X = rows_of(rng, 21, [LENS[r % 8] for r in range(300)], 128)
    Y = rows_of(rng, 21, [LENS[(r + 5) % 8] for r in range(41)], 128)
    X[::7, 3] = 0
    xo, yo = operands(nat, 21, X, Y)
    cost = nat.sub_cost(C)
    for gap in (1, 13, 255):
        for ob in (8, 2) if gap == 1 else (8,):
            lin = nat.alignment_dense(xo, yo, cost, gap, out_bytes=ob)
            aff = nat.alignment_affine_dense(xo, yo, cost, gap, 0, out_bytes=ob)
            assert aff.dtype == lin.dtype and torch.equal(aff, lin), (gap, ob)


def test_operator_on_device_and_host_agree():
    rng = np.random.default_rng(4)
    C = table(rng, 21, np.arange(256))
    dist = alignment(C, 17, gap_open=40)
    X, Y = rows_of(rng, 21, rng.integers(0, 51, 300), 50), rows_of(rng, 21, rng.integers(0, 38, 21), 37)     # unequal widths
    X[::4, 3] = 0
    want = definition(C, 17, 40, X, Y)
    on_gpu = dist(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
    on_cpu = dist(torch.from_numpy(X), torch.from_numpy(Y))
    assert on_gpu.is_cuda and on_gpu.dtype == torch.int64 and not on_cpu.is_cuda
    assert np.array_equal(on_gpu.cpu().numpy(), want) and np.array_equal(on_cpu.numpy(), want)
    half = dist(torch.from_numpy(X).cuda().half(), torch.from_numpy(Y).cuda().half(), similarity=True)
    assert half.dtype == torch.float32 and torch.equal(half, 1 / (1 + on_gpu))
    Xw, Yw = rows_of(rng, 21, rng.integers(100, 131, 40), 130), rows_of(rng, 21, [130, 5, 64], 130)
    Xw[0, :] = rng.integers(1, 21, 130)                           # 130 positions: the torch expression, on the device
    wide = dist(torch.from_numpy(Xw).cuda(), torch.from_numpy(Yw).cuda())
    assert wide.is_cuda and np.array_equal(wide.cpu().numpy(), definition(C, 17, 40, Xw, Yw))
    with pytest.raises(ValueError):
        dist(torch.tensor([[1, 21]]).cuda(), torch.tensor([[1, 2]]).cuda())


# ---------------------------------------------------------------- 2. graphs and search against the definition
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


@pytest.fixture(scope="module")
def weighted(tmp_path_factory):
    """300 clustered rows of 16..24 positions with duplicates; a random symmetric table of even costs up to 12, gap 5 and
    gap_open 7, so that many alignments share a cost and distances tie; 24 * 12 + 7 <= 2048, and queries of up to 128
    positions stay native."""
    tok, _ = synth.clustered_varlen_tokens(300, Lmax=24, Lmin=16, seed=11, members=30)
    tok = tok.copy()
    tok[40], tok[299] = tok[41], tok[41]
    rng = np.random.default_rng(21)
    C = table(rng, 21, 2 * np.arange(1, 7))
    P = _prograph(tmp_path_factory.mktemp("aln_affine"), tok, "weighted")
    D = definition(C, 5, 7, tok, tok)
    assert (D != definition(C, 5, 0, tok, tok)).any()             # the open penalty matters on this data
    return P, tok, C, alignment(C, 5, gap_open=7), D


@pytest.mark.parametrize("k", [1, 16, 70])
def test_knn_graph(weighted, k):
    P, tok, C, dist, D = weighted
    wi, wd = knn_of(D, k, 1)
    G = P.build_graph(k=k, distance=dist, output="csr")
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.first == 1
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    assert k == 1 or (np.diff(wd, axis=1) == 0).any(), "ties must be present"
    gi, gw = _arrays(P.build_graph(k=k, distance=dist))
    assert gi.dtype == np.int64 and gw.dtype == np.int64 and np.array_equal(gi, wi) and np.array_equal(gw, wd)


@pytest.mark.parametrize("comp,eps", [("le", 30), ("lt", 30), ("eq", 17), ("le", 22.5), ("ge", 100)])
def test_eps_graph(weighted, comp, eps):
    P, tok, C, dist, D = weighted
    ip, ix, w = csr_of(D, OPS[comp], eps)
    assert 0 < ip[-1] < D.size
    G = P.build_graph(eps=eps, distance=dist, comp=OPS[comp], output="csr")
    assert G.indptr.dtype == torch.int64 and G.indices.dtype == torch.int32 and G.weights.dtype == torch.int16
    assert np.array_equal(G.indptr.cpu().numpy(), ip) and np.array_equal(G.indices.cpu().numpy(), ix)
    assert np.array_equal(G.weights.cpu().numpy(), w)
    for i in (40, 41, 299):
        assert not {40, 41, 299} & set(ix[ip[i]:ip[i + 1]])       # d > 0: a row and its duplicates are no neighbours


def test_search(weighted):
    P, tok, C, dist, D = weighted
    lut = np.array([""] + list(synth.AMINO))
    rows = tok[[3, 50, 99, 200, 41]].copy()
    strings = ["".join(lut[r[r > 0]]) for r in rows]
    strings[0] = strings[0][:9]                                   # narrower than the dataset
    strings[1] = strings[1] + "ACDEFGHIKL" * 4                    # wider than it
    strings[2] = "XB" + strings[2][2:]                            # unknown letters: token 0
    strings[3] = strings[3][:5] + strings[3][8:]                  # a block of three deleted: one run
    Q = P.tokenize(strings)
    assert Q.shape[1] > tok.shape[1] and (Q[2, :2] == 0).all() and Q.shape[1] * dist.max_cost + dist.gap_open <= 2048
    DQ = definition(C, 5, 7, tok, Q)
    assert DQ[3, 200] == 7 + 3 * 5 and DQ[4].min() == 0           # one open, three symbols; a dataset row
    for q in (strings, Q, torch.from_numpy(Q)):
        for k in (1, 5, 70, len(tok) + 5):                        # k >= N: every row, in order
            wi, wd = knn_of(DQ, min(k, len(tok)), 0)
            gi, gw = _arrays(P.search(q, k=k, distance=dist))
            assert gi.dtype == np.int64 and np.array_equal(gi, wi) and np.array_equal(gw, wd)
        for comp, eps in (("le", 0), ("le", 30), ("ge", 100), ("eq", 22), ("lt", 22.5)):
            ip, ix, w = csr_of(DQ, OPS[comp], eps, keep_zero=True)
            got = P.search(q, eps=eps, distance=dist, comp=OPS[comp])
            for i, (gi, gw) in enumerate(got):
                assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]]), (comp, eps, i)
    exact = P.search(strings[4], eps=0, distance=dist)[0]
    assert list(exact[0]) == [40, 41, 299] and (exact[1] == 0).all()         # eps = 0 keeps the exact matches
    first = P.search(strings[4], k=2, distance=dist)[0]
    assert first[1][0] == 0 and first[0][0] == 40                 # rank 0 kept
    G = P.search(Q, k=3, distance=dist, output="csr")
    assert G.first == 0 and G.nrows == len(Q) and G.ncols == len(tok) and G.dist.dtype == torch.int16
    wi, wd = knn_of(DQ, 1, 0)
    hit, dmin = P.nearest_neighbour(strings[3], distance=dist)
    assert list(hit.index) == [int(wi[3, 0])] and dmin == wd[3, 0]
    seq = P("Sequence")[41]
    want = np.nonzero(D[41] <= 30)[0]
    assert np.array_equal(np.sort(np.asarray(P.calc_neighbours(seq, eps=30, distance=dist, comp=operator.le))), want)
    assert list(P.neighbourhood(seq, 30, distance=dist).index) == list(want)


def test_block_insertions_against_scattered_substitutions(tmp_path):
    """The feature reaches the graph: a base sequence, copies with one block of six residues inserted (one event) and
    copies with two substitutions far apart, every substitution at cost 6.  Linear, gap 1: a substitution is undone by two
    gaps at 2, so a substitution copy is at 4 and an insertion copy at 6, and the base's neighbours are the substitution
    copies - the shredded alignments of a cheap linear gap.  With gap_open 3 two gaps cost 8, a substitution copy is at
    12, an insertion copy at 3 + 6 = 9, and the insertion copies come first.  The affine graph equals the definition's
    and differs from the linear graph."""
    rng = np.random.default_rng(17)
    a = 21
    C = np.full((a, a), 6, dtype=np.int64)
    np.fill_diagonal(C, 0)
    base = rng.integers(1, a, 40)
    rows = [base]
    for t in range(8):                                            # block insertions
        at = 3 + 4 * t
        rows.append(np.concatenate([base[:at], rng.integers(1, a, 6), base[at:]]))
    for t in range(8):                                            # two substitutions, far apart
        r = base.copy()
        for at in (4 + 2 * t, 22 + t):
            r[at] = (r[at] % (a - 1)) + 1                         # another symbol
        rows.append(r)
    for _ in range(60):                                           # unrelated rows: more than one wave of columns
        rows.append(rng.integers(1, a, rng.integers(30, 47)))
    tok = np.zeros((len(rows), 46), dtype=np.int64)
    for r, row in enumerate(rows):
        tok[r, :len(row)] = row
    P = _prograph(tmp_path, tok, "indels")
    affine, linear = alignment(C, 1, gap_open=3), alignment(C, 1)
    D = definition(C, 1, 3, tok, tok)
    DL = definition(C, 1, 0, tok, tok)
    assert (D[0, 1:9] == 9).all() and (D[0, 9:17] == 12).all() and (DL[0, 1:9] == 6).all() and (DL[0, 9:17] == 4).all()
    GA = P.build_graph(k=8, distance=affine, output="csr")
    GL = P.build_graph(k=8, distance=linear, output="csr")
    wi, wd = knn_of(D, 8, 1)
    assert np.array_equal(GA.idx.cpu().numpy(), wi) and np.array_equal(GA.dist.cpu().numpy(), wd)
    assert set(GA.idx[0].tolist()) == set(range(1, 9)) and set(GL.idx[0].tolist()) == set(range(9, 17))
    assert not torch.equal(GA.idx, GL.idx)                        # the affine graph is not the linear one


def test_beyond_the_fp16_bound_the_generic_loop_gives_the_definition(tmp_path, monkeypatch):
    from prograph_amd import _native
    rng = np.random.default_rng(13)
    tok = rows_of(rng, 21, [9] * 60, 9)
    tok[1::3] = tok[0]                                            # near rows: one position apart
    tok[1::3, 5] = rng.integers(1, 21, 20)
    C = table(rng, 21, [1, 2, 3])
    dist = alignment(C, 227, gap_open=6)                          # 9 * 227 + 6 = 2049; + 5 = 2048 would still be native
    assert 9 * dist.max_cost + dist.gap_open == 2049
    P = _prograph(tmp_path, tok, "narrow")
    D = definition(C, 227, 6, tok, tok)
    native = P.build_graph(k=4, distance=alignment(C, 227, gap_open=5), output="csr")       # at the bound: the kernel
    wi, wd = knn_of(definition(C, 227, 5, tok, tok), 4, 1)
    assert native.dist.dtype == torch.int16 and np.array_equal(native.idx.cpu().numpy(), wi)
    assert np.array_equal(native.dist.cpu().numpy(), wd)
    monkeypatch.setattr(_native, "f16_knn", None)                 # beyond it the selection layer must not run
    monkeypatch.setattr(_native, "f16_eps", None)
    gi, gw = _arrays(P.build_graph(k=4, distance=dist))
    wi, wd = knn_of(D, 4, 1)
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd)
    ip, ix, w = csr_of(D, operator.le, 3)
    assert ip[-1] > 0
    for i, (gi, gw) in enumerate(P.build_graph(eps=3, distance=dist)):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    gi, gw = _arrays(P.search(tok[:2], k=3, distance=dist))
    wi, wd = knn_of(D[:2], 3, 0)
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd)
