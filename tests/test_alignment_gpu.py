"""
Gapped alignment distance on the GPU: `pg_alignment_dense` (every entry against the definition in numpy below),
`build_graph` / `search` with `distance=alignment(C, gap)` against a stable sort / nonzero of that definition, and the two
identities that pin the definition to tested code: (1 - I, 1) is `levenshtein`, and on equal-length rows with
2 * gap > L * max(C) it is `substitution(C)`.  Every comparison is an every-entry equality.
"""
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import lev_testdata as LT
from conftest import load_golden
from prograph_amd import synth
from prograph_amd.distance import alignment, levenshtein, substitution

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

OPS = {"le": operator.le, "lt": operator.lt, "eq": operator.eq, "ge": operator.ge, "gt": operator.gt}
LENS = (0, 1, 15, 16, 17, 33, 127, 128)       # sequence lengths: around the 16-cost read and the chunk counts


# ---------------------------------------------------------------- the yardstick: the definition
def lengths(T):
    """Index of the last non-zero + 1 per row."""
    T = np.asarray(T)
    return np.where(T != 0, np.arange(1, T.shape[1] + 1), 0).max(axis=1, initial=0)


def definition(C, gap, X, Y):
    """(M, N) int64: H[len y][len x] of the recurrence, the plain double loop over positions, all pairs at once (the
    rows of Y taken length by length, so that the outer loop stops at the last row of their tables)."""
    C, X, Y = np.asarray(C, dtype=np.int64), np.atleast_2d(np.asarray(X, dtype=np.intp)), np.atleast_2d(np.asarray(Y, dtype=np.intp))
    lx, ly = lengths(X), lengths(Y)
    X = X[:, :lx.max(initial=0)]
    N, LX = len(X), X.shape[1]
    out = np.empty((len(Y), N), dtype=np.int64)
    for l in np.unique(ly):
        rows = np.nonzero(ly == l)[0]
        H = np.empty((LX + 1, len(rows), N), dtype=np.int64)      # one table row for every pair: H[j] = H[i][j]
        H[:] = (np.arange(LX + 1) * gap)[:, None, None]
        for i in range(1, l + 1):
            cy = C[Y[rows, i - 1]]                                # (rows, A): the costs of y_i against every symbol
            diag = H[0].copy()
            H[0] = i * gap
            for j in range(1, LX + 1):
                up = H[j].copy()
                H[j] = np.minimum(diag + cy[:, X[:, j - 1]], np.minimum(up, H[j - 1]) + gap)
                diag = up
        out[rows] = np.take_along_axis(H, np.broadcast_to(lx[None, None, :], (1, len(rows), N)), 0)[0]
    return out


def knn_of(D, k, first):
    order = np.argsort(D, axis=1, kind="stable")[:, first:first + k]
    return order, np.take_along_axis(D, order, 1)


def csr_of(D, comp, eps, keep_zero=False):
    keep = comp(D, eps) & ((D >= 0) if keep_zero else (D > 0))
    r, c = np.nonzero(keep)
    return np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64), c, D[r, c]


def table(rng, a, values):
    """A random symmetric (a, a) table with a zero diagonal, entries drawn from `values`."""
    C = rng.choice(np.asarray(values), size=(a, a))
    C = np.triu(C, 1)
    return C + C.T


def rows_of(rng, a, lens, width):
    """Rows of tokens 1..a-1 with the given lengths, zero right-padded to `width`."""
    T = np.zeros((len(lens), width), dtype=np.int64)
    for r, l in enumerate(lens):
        T[r, :l] = rng.integers(1, a, l)
    return T


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def dense(nat, C, gap, X, Y, **kw):
    a = len(C)
    xo = nat.aln_operand(torch.from_numpy(np.ascontiguousarray(X).astype(np.uint8)), a)
    yo = nat.aln_operand(torch.from_numpy(np.ascontiguousarray(Y).astype(np.uint8)), a)
    assert xo.valid() and yo.valid()
    return nat.alignment_dense(xo, yo, nat.sub_cost(C), gap, **kw)


# ---------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("a,gap", [(21, 1), (21, 7), (21, 255), (32, 1), (32, 7), (32, 255)])
def test_kernel_against_the_definition(nat, a, gap):
    """One lane per column, 64 columns per wave, 256 per workgroup, 8 rows per workgroup, 16 cells per LDS read, the
    kernel switches on ceil(len y / 16).  Row r of either operand has length LENS[r % 8], so any window of 8 rows
    holds every length: the definition is evaluated once on 77 x 607 pairs and every (rows, columns) shape is taken as
    a window of it, from every offset 0..7 - every length against every number of rows and columns, and every pair of
    lengths."""
    rng = np.random.default_rng(1000 * a + gap)
    C = table(rng, a, np.arange(256))
    C[1, a - 1] = C[a - 1, 1] = 255
    Xall = rows_of(rng, a, [LENS[r % 8] for r in range(607)], 128)
    Yall = rows_of(rng, a, [LENS[(r + 3) % 8] for r in range(77)], 128)
    want = definition(C, gap, Xall, Yall)
    width = lambda T: max(1, int(lengths(T).max()))              # the operands go in at their own widths
    for M in (1, 15, 17, 70):
        for N in (1, 63, 65, 257, 600):
            for o in range(8):
                for p in (range(8) if N == 1 else [(5 * o + 1) % 8]):
                    X, Y = Xall[p:p + N], Yall[o:o + M]
                    got = dense(nat, C, gap, X[:, :width(X)], Y[:, :width(Y)])
                    assert got.dtype == torch.int64 and got.shape == (M, N)
                    assert np.array_equal(got.cpu().numpy(), want[o:o + M, p:p + N]), (a, gap, M, N, o, p)
    got = dense(nat, C, gap, Xall, Yall)                                      # and both at the full width, zero padded
    assert np.array_equal(got.cpu().numpy(), want)


def test_kernel_every_lane_its_own_length_and_interior_zeros(nat):
    rng = np.random.default_rng(77)
    C = table(rng, 21, np.arange(256))
    X = rows_of(rng, 21, list(rng.permutation(np.arange(1, 129)))[:64] + list(range(64, 0, -1)), 128)   # two waves
    Y = rows_of(rng, 21, [128, 90, 64, 17, 5, 0, 33, 100, 77], 128)
    assert len(set(lengths(X[:64]))) == 64
    assert np.array_equal(dense(nat, C, 9, X, Y).cpu().numpy(), definition(C, 9, X, Y))
    # interior zeros are symbol 0 of the table; only trailing ones are padding
    X[::3, 2], X[1::5, 0], Y[::2, 4], Y[3, :16] = 0, 0, 0, 0
    X[7, 100:] = 0
    X[7, 110] = 3                                                 # zeros inside, a symbol after them
    want = definition(C, 9, X, Y)
    assert np.array_equal(dense(nat, C, 9, X, Y).cpu().numpy(), want)
    assert lengths(X)[7] == 111 and lengths(Y)[3] == 17


def test_kernel_cell_range_and_output_types(nat):
    C = np.zeros((21, 21), dtype=np.int64)
    C[3, 7] = C[7, 3] = 255
    X, Y = np.full((70, 128), 3), np.full((9, 128), 7)
    Y[1, 1:] = 0                                                  # a single token 7: one pair, 127 gaps
    want = definition(C, 255, X, Y)
    assert (want == 32640).all()                                  # 128 * 255: a cell narrower than 16 bits fails
    got = dense(nat, C, 255, X, Y)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    # fp16 equals int64 up to d = 2048 exactly: 64 positions at cost 32 with gap 32
    rng = np.random.default_rng(9)
    C = table(rng, 32, np.arange(33))
    C[1, 2] = C[2, 1] = 32
    X, Y = rows_of(rng, 32, rng.integers(1, 65, 300), 64), rows_of(rng, 32, rng.integers(1, 65, 33), 64)
    X[17], Y[4] = 1, 2
    want = definition(C, 32, X, Y)
    assert want.max() == 2048 and want[4, 17] == 2048
    assert np.array_equal(dense(nat, C, 32, X, Y).cpu().numpy(), want)
    h = dense(nat, C, 32, X, Y, out_bytes=2)
    assert h.dtype == torch.float16 and np.array_equal(h.cpu().numpy().astype(np.int64), want)


def test_kernel_row_range(nat):
    rng = np.random.default_rng(2)
    C = table(rng, 21, np.arange(256))
    X, Y = rows_of(rng, 21, rng.integers(0, 51, 130), 50), rows_of(rng, 21, rng.integers(0, 41, 19), 40)
    xo, yo = (nat.aln_operand(torch.from_numpy(T.astype(np.uint8)), 21) for T in (X, Y))
    cost = nat.sub_cost(C)
    one = nat.alignment_dense(xo, yo, cost, 11)
    assert np.array_equal(one.cpu().numpy(), definition(C, 11, X, Y))
    for ob in (8, 2):
        rows = nat.alignment_dense(xo, yo, cost, 11, out_bytes=ob, rows=(3, 19))          # a Y operand from row 3 on
        assert rows.shape == (16, 130) and np.array_equal(rows.cpu().numpy().astype(np.int64), one.cpu().numpy()[3:])


# ---------------------------------------------------------------- datasets
def _prograph(tmp, tok, name):
    from prograph_amd import Prograph
    f = tmp / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P


def _same_tuples(got, want):
    assert len(got) == len(want)
    for (gi, gw), (wi, ww) in zip(got, want):
        assert gi.dtype == wi.dtype and gw.dtype == ww.dtype
        assert np.array_equal(gi, wi) and np.array_equal(gw, ww)


# ---------------------------------------------------------------- 2. the two identities
def test_one_minus_identity_with_gap_one_is_levenshtein_operator():
    dist = alignment(1 - np.eye(32, dtype=np.int64), 1)
    A = LT.set_a()
    X, Y = torch.from_numpy(A[:700]).cuda(), torch.from_numpy(A[700:820]).cuda()
    assert torch.equal(dist(X, Y), levenshtein(X, Y))
    V = torch.from_numpy(load_golden("synth_n300_varlen24")["tokens"]).cuda()
    assert torch.equal(dist(V, V), levenshtein(V, V))
    assert torch.equal(dist(X, V[:40]), levenshtein(X, V[:40]))                          # unequal widths


def test_one_minus_identity_with_gap_one_is_levenshtein_graphs(tmp_path):
    g = load_golden("synth_n300_varlen24")
    P = _prograph(tmp_path, g["tokens"], "varlen24")
    dist = alignment(1 - np.eye(21, dtype=np.int64), 1)
    for k in (1, 8, 70):
        G = P.build_graph(k=k, distance=dist, output="csr")
        L = P.build_graph(k=k, distance=levenshtein, output="csr")
        assert G.dist.dtype == torch.int16 and L.dist.dtype == torch.uint8                # the device weight types differ
        assert torch.equal(G.idx, L.idx) and torch.equal(G.dist.long(), L.dist.long())
        _same_tuples(P.build_graph(k=k, distance=dist), P.build_graph(k=k, distance=levenshtein))
    for comp, eps in (("le", 2), ("le", 6), ("eq", 3), ("ge", 20), ("lt", 9.5)):
        G = P.build_graph(eps=eps, distance=dist, comp=OPS[comp], output="csr")
        assert G.weights.dtype == torch.int16 and G.indices.numel() > 0
        _same_tuples(G.to_tuples(), P.build_graph(eps=eps, distance=levenshtein, comp=OPS[comp]))
    strings = synth.tokens_to_strings(g["tokens"][[3, 77, 200]])
    strings += [strings[0][:-4], strings[1] + "ACDAC", "WWWW"]
    for q in (strings, g["tokens"][10:14].astype(np.int64)):
        _same_tuples(P.search(q, k=7, distance=dist), P.search(q, k=7, distance=levenshtein))
        _same_tuples(P.search(q, eps=3, distance=dist), P.search(q, eps=3, distance=levenshtein))
        _same_tuples(P.search(q, eps=0, distance=dist), P.search(q, eps=0, distance=levenshtein))


def test_one_minus_identity_with_gap_one_is_levenshtein_graphs_set_a(tmp_path, monkeypatch):
    """The same on set A of the Levenshtein tests: 1060 rows of width 128, lengths 40..128, so eight chunks per row, and -
    with the block budget cut to 200 rows - six row blocks of the 128-position kernel through `_select_blocks`; queries
    longer than the golden's 24 positions and still native."""
    from prograph_amd import Prograph
    A = LT.set_a()
    P = _prograph(tmp_path, A, "set_a")
    n = len(A)
    assert A.shape == (1060, 128) and lengths(A).min() >= 40 and lengths(A).max() == 128
    monkeypatch.setattr(Prograph, "_BLOCK_ELEMS", n * 200)
    assert P._block_rows(n, n, 64) == 200
    dist = alignment(1 - np.eye(21, dtype=np.int64), 1)
    for k in (1, 16, 70):
        G = P.build_graph(k=k, distance=dist, output="csr")
        L = P.build_graph(k=k, distance=levenshtein, output="csr")
        assert G.dist.dtype == torch.int16 and L.dist.dtype == torch.uint8                # the device weight types differ
        assert torch.equal(G.idx, L.idx) and torch.equal(G.dist.long(), L.dist.long())
        _same_tuples(P.build_graph(k=k, distance=dist), P.build_graph(k=k, distance=levenshtein))
    for comp, eps in (("le", 4), ("le", 12), ("eq", 3), ("ge", 90), ("lt", 9.5), ("gt", 80.5)):
        G = P.build_graph(eps=eps, distance=dist, comp=OPS[comp], output="csr")
        assert G.weights.dtype == torch.int16 and 0 < G.indices.numel() < n * n
        _same_tuples(G.to_tuples(), P.build_graph(eps=eps, distance=levenshtein, comp=OPS[comp]))
    rows = A[[5, 300, 640, 1000]]
    short = int(np.argmin(lengths(A)))
    strings = synth.tokens_to_strings(np.concatenate([rows, A[[short]]]))
    assert max(map(len, strings)) > 24 and len(strings[4]) + 30 <= 128
    strings[1] = strings[1][:50]                                   # shorter than its row
    unknown = [strings[2][:30] + "XB" + strings[2][32:]]          # unknown letters: token 0, an interior zero
    strings[2] = strings[2][:9]
    strings[3] = strings[3][:17] + strings[3][18:]                # one deletion
    strings[4] = strings[4] + "ACDEFGHIKL" * 3                    # longer than its row
    strings.append("WWWW")
    for q in (strings, unknown, A[10:14].astype(np.int64), torch.from_numpy(A[500:503].astype(np.int64))):
        for k in (1, 7, 70):
            _same_tuples(P.search(q, k=k, distance=dist), P.search(q, k=k, distance=levenshtein))
        for comp, eps in (("le", 0), ("le", 3), ("le", 12), ("ge", 90)):
            _same_tuples(P.search(q, eps=eps, distance=dist, comp=OPS[comp]),
                         P.search(q, eps=eps, distance=levenshtein, comp=OPS[comp]))
    G = P.search(strings, k=7, distance=dist, output="csr")
    L = P.search(strings, k=7, distance=levenshtein, output="csr")
    assert G.nrows == len(strings) == 6 and G.first == 0
    assert G.dist.dtype == torch.int16 and L.dist.dtype == torch.uint8 and torch.equal(G.idx, L.idx)
    assert torch.equal(G.dist.long(), L.dist.long())


def test_with_a_prohibitive_gap_it_is_substitution():
    rng = np.random.default_rng(6)
    for L, top, gap in ((8, 48, 193), (40, 6, 121)):
        C = table(rng, 21, np.arange(1, top + 1))
        assert 2 * gap > L * C.max()
        X, Y = rng.integers(1, 21, (400, L)), rng.integers(1, 21, (37, L))                # one length, no zeros
        Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
        got = alignment(C, gap)(Xd, Yd)
        assert torch.equal(got, substitution(C)(Xd, Yd))
        assert torch.equal(got, alignment(substitution(C), gap)(Xd, Yd))                  # a substitution lends its table


# ---------------------------------------------------------------- 3. the operator
def test_operator_on_device_and_host_agree():
    rng = np.random.default_rng(4)
    C = table(rng, 21, np.arange(256))
    dist = alignment(C, 17)
    X, Y = rows_of(rng, 21, rng.integers(0, 51, 300), 50), rows_of(rng, 21, rng.integers(0, 38, 21), 37)     # unequal widths
    X[::4, 3] = 0
    want = definition(C, 17, X, Y)
    on_gpu = dist(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
    on_cpu = dist(torch.from_numpy(X), torch.from_numpy(Y))
    assert on_gpu.is_cuda and on_gpu.dtype == torch.int64 and not on_cpu.is_cuda
    assert np.array_equal(on_gpu.cpu().numpy(), want) and np.array_equal(on_cpu.numpy(), want)
    half = dist(torch.from_numpy(X).cuda().half(), torch.from_numpy(Y).cuda().half(), similarity=True)
    assert half.dtype == torch.float32 and torch.equal(half, 1 / (1 + on_gpu))
    Xw, Yw = rows_of(rng, 21, rng.integers(100, 131, 40), 130), rows_of(rng, 21, [130, 5, 64], 130)
    Xw[0, :] = rng.integers(1, 21, 130)                           # 130 positions: the torch expression, on the device
    wide = dist(torch.from_numpy(Xw).cuda(), torch.from_numpy(Yw).cuda())
    assert wide.is_cuda and np.array_equal(wide.cpu().numpy(), definition(C, 17, Xw, Yw))
    with pytest.raises(ValueError):
        dist(torch.tensor([[1, 21]]).cuda(), torch.tensor([[1, 2]]).cuda())


# ---------------------------------------------------------------- 4. weighted graphs against the definition
@pytest.fixture(scope="module")
def weighted(tmp_path_factory):
    """300 clustered rows of 16..24 positions with duplicates; a table of even costs up to 12 and gap 5, so that many
    alignments share a cost and distances tie; 24 * 12 = 288 <= 2048, and queries of up to 128 positions stay native."""
    tok, _ = synth.clustered_varlen_tokens(300, Lmax=24, Lmin=16, seed=11, members=30)
    tok = tok.copy()
    tok[40], tok[299] = tok[41], tok[41]
    rng = np.random.default_rng(21)
    C = table(rng, 21, 2 * np.arange(1, 7))
    assert C.max() == 12
    P = _prograph(tmp_path_factory.mktemp("aln"), tok, "weighted")
    D = definition(C, 5, tok, tok)
    assert D.max() == 126
    padded = C[tok.astype(np.intp)[:, None, :], tok.astype(np.intp)[None, :, :]].sum(-1)
    assert (D != padded).sum() == 89418                           # gaps matter on this data
    return P, tok, C, alignment(C, 5), D


@pytest.mark.parametrize("k", [1, 16, 70])
def test_weighted_knn_graph(weighted, k):
    P, tok, C, dist, D = weighted
    wi, wd = knn_of(D, k, 1)
    G = P.build_graph(k=k, distance=dist, output="csr")
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.first == 1
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    assert k == 1 or (np.diff(wd, axis=1) == 0).any(), "ties must be present"
    got = P.build_graph(k=k, distance=dist)
    assert all(gi.dtype == np.int64 and gw.dtype == np.int64 for gi, gw in got)
    assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)
    sim = P.build_graph(k=k, distance=dist, similarity=True)
    ws = (1 / (1 + torch.from_numpy(wd))).numpy()
    assert all(gw.dtype == np.float32 for _, gw in sim)
    assert np.array_equal(np.array([i for i, _ in sim]), wi) and np.array_equal(np.array([w for _, w in sim]), ws)


@pytest.mark.parametrize("comp,eps,kept", [("le", 20, 5268), ("lt", 20, 4256), ("eq", 10, 756), ("le", 12.5, 1438),
                                           ("ge", 100, 23038), ("gt", 99.5, 23038)])
def test_weighted_eps_graph(weighted, comp, eps, kept):
    P, tok, C, dist, D = weighted
    ip, ix, w = csr_of(D, OPS[comp], eps)
    assert ip[-1] == kept and 0 < ip[-1] < D.size
    G = P.build_graph(eps=eps, distance=dist, comp=OPS[comp], output="csr")
    assert G.indptr.dtype == torch.int64 and G.indices.dtype == torch.int32 and G.weights.dtype == torch.int16
    assert np.array_equal(G.indptr.cpu().numpy(), ip) and np.array_equal(G.indices.cpu().numpy(), ix)
    assert np.array_equal(G.weights.cpu().numpy(), w)
    for i in (40, 41, 299):
        assert not {40, 41, 299} & set(ix[ip[i]:ip[i + 1]])       # d > 0: a row and its duplicates are no neighbours
    got = P.build_graph(eps=eps, distance=dist, comp=OPS[comp], similarity=True)
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]])
        assert not len(gi) or (gw.dtype == np.float32 and np.array_equal(gw, (1 / (1 + torch.from_numpy(w[ip[i]:ip[i + 1]]))).numpy()))


def test_weighted_surface(weighted):
    P, tok, C, dist, D = weighted
    sub = np.arange(100, 250)
    ip, ix, w = csr_of(D[np.ix_(sub, sub)], operator.le, 25)
    got = P.build_graph(eps=25, distance=dist, idxs=sub)
    assert len(got) == len(sub) and ip[-1] > 0
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])      # subset-relative
        assert not len(gi) or (gi.dtype == np.int64 and gw.dtype == np.int64)
    wi, wd = knn_of(D[np.ix_(sub, sub)], 5, 1)
    got = P.build_graph(k=5, distance=dist, idxs=sub)
    assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)
    G = P.build_graph(eps=30, distance=dist, store="S", output="csr")
    assert "S" in P.csr_graphs and P._device_graph("S") is not None
    deg, dirichlet, lv = P.degree("S"), P.dirichlet("S"), P.local_variance("S")
    P.graph["S_host"] = list(P.graph["S"])                       # same rows, no device graph behind them: the tuple route
    assert P._device_graph("S_host") is None
    assert np.array_equal(deg, P.degree("S_host")) and np.isclose(dirichlet, P.dirichlet("S_host"), rtol=1e-9)
    assert np.allclose(lv, P.local_variance("S_host"), equal_nan=True)
    assert (P.adjacency("S") != P.adjacency("S_host")).nnz == 0
    ip, ix, w = csr_of(D, operator.le, 30)
    assert np.array_equal(G.indptr.cpu().numpy(), ip) and np.array_equal(G.weights.cpu().numpy(), w)
    twin = alignment(C.copy(), 5)                                # an equal table and gap: the same route, the same graph
    T = P.build_graph(eps=30, distance=twin, output="csr")
    assert T.weights.dtype == torch.int16 and torch.equal(T.indices, G.indices) and torch.equal(T.weights, G.weights)


# ---------------------------------------------------------------- 5. search
def test_search(weighted):
    P, tok, C, dist, D = weighted
    lut = np.array([""] + list(synth.AMINO))
    rows = tok[[3, 50, 99, 200, 41, 17, 250, 120, 8]].copy()
    strings = ["".join(lut[r[r > 0]]) for r in rows]
    strings[0] = strings[0][:9]                                   # shorter than the dataset
    strings[1] = strings[1] + "ACDEFGHIKL" * 4                    # longer than it
    strings[2] = "XB" + strings[2][2:]                            # unknown letters: token 0
    strings[3] = strings[3][:5] + strings[3][6:]                  # one deletion
    Q = P.tokenize(strings)
    assert Q.shape[1] > tok.shape[1] and (Q[2, :2] == 0).all() and Q.shape[1] * dist.max_cost <= 2048
    DQ = definition(C, 5, tok, Q)
    assert DQ[3].min() == 5 and DQ[4].min() == 0                  # one gap; a dataset row
    for q in (strings, Q, torch.from_numpy(Q)):
        for k in (1, 5, 70, len(tok) + 5):                        # k >= N: every row, in order
            wi, wd = knn_of(DQ, min(k, len(tok)), 0)
            got = P.search(q, k=k, distance=dist)
            assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)
            assert got[0][0].dtype == np.int64 and got[0][1].dtype == np.int64
        for comp, eps in (("le", 0), ("le", 20), ("ge", 100), ("eq", 10), ("lt", 12.5)):
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
    S = P.search(Q, eps=20, distance=dist, output="csr", similarity=True)
    assert S.weights.dtype == torch.int16 and S.nrows == len(Q)
    wi, wd = knn_of(DQ, 1, 0)
    hit, dmin = P.nearest_neighbour(strings[3], distance=dist)
    assert list(hit.index) == [int(wi[3, 0])] and dmin == wd[3, 0]
    # neighbourhood / calc_neighbours take the instance as they take levenshtein: a dataset row and a new string
    seq = P("Sequence")[41]
    want = np.nonzero(D[41] <= 20)[0]
    assert np.array_equal(np.sort(np.asarray(P.calc_neighbours(seq, eps=20, distance=dist, comp=operator.le))), want)
    assert list(P.neighbourhood(seq, 20, distance=dist).index) == list(want)
    assert list(P.neighbourhood(strings[3], 20, distance=dist).index) == list(np.nonzero(DQ[3] <= 20)[0])


# ---------------------------------------------------------------- 6. the non-native side
def test_beyond_the_fp16_bound_the_generic_loop_gives_the_definition(tmp_path, monkeypatch):
    from prograph_amd import _native
    rng = np.random.default_rng(13)
    tok = rows_of(rng, 21, [9] * 60, 9)
    tok[1::3] = tok[0]                                            # near rows: one position apart
    tok[1::3, 5] = rng.integers(1, 21, 20)
    C = table(rng, 21, [1, 2, 3])
    dist = alignment(C, 251)                                      # max(max C, gap) = 251: 9 * 251 = 2259, and
    short = alignment(C, 227)                                     # 9 * 227 = 2043 would still be native
    assert 9 * dist.max_cost > 2048 >= 9 * short.max_cost
    wide = np.zeros((60, 683), dtype=np.int64)                    # the bound itself: width * max(max C, gap) = 2049
    wide[:, :9] = tok
    assert 683 * alignment(C, 3).max_cost == 2049
    P = _prograph(tmp_path, tok, "narrow")
    D = definition(C, 251, tok, tok)
    monkeypatch.setattr(_native, "f16_knn", None)                 # the selection layer must not run
    monkeypatch.setattr(_native, "f16_eps", None)
    got = P.build_graph(k=4, distance=dist)
    wi, wd = knn_of(D, 4, 1)
    assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)
    ip, ix, w = csr_of(D, operator.le, 3)
    assert ip[-1] > 0
    got = P.build_graph(eps=3, distance=dist)
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    got = P.search(tok[:2], k=3, distance=dist)
    wi, wd = knn_of(D[:2], 3, 0)
    assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)
    P.graph["W683"] = list(wide)                                  # 683 positions at cost 3: 2049, the torch expression
    got = P.build_graph(k=2, distance=alignment(C, 3), representation="W683", idxs=np.arange(12))
    wi, wd = knn_of(definition(C, 3, wide[:12], wide[:12]), 2, 1)
    assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)
