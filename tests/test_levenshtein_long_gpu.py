"""
The Levenshtein kernel beyond 128 positions on the device (pg_lev_long.hip): the dense kernel as windows of the one
reference matrix of tests/lev_long_testdata.py at every instantiated block count, closed forms at full length, the
operator, the independent alignment kernel with 1 - I, and the surface (graphs, search, single-sequence queries).
"""
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import lev_long_testdata as LL
import lev_testdata as LT
from prograph_amd.distance import alignment, levenshtein

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    return _native


@pytest.fixture(scope="module")
def D():
    return LL.long_matrix()


def _x(nat, width, ncols):
    """Column c = the (c mod count)-th row of long_x() that fits `width`, packed at that width; its rows of long_x()."""
    sel = np.array([r for r, l in enumerate(LL.X_LENS) if l <= width])
    cols = sel[np.arange(ncols) % len(sel)]
    return nat.lev_long_operand(torch.from_numpy(np.ascontiguousarray(LL.long_x()[cols][:, :width]))), cols


def _y(nat, width, m):
    sel = np.array([i for i, l in enumerate(LL.Y_LENS) if l <= width])
    rows = sel[np.arange(m) % len(sel)]
    return nat.lev_long_operand(torch.from_numpy(np.ascontiguousarray(LL.long_y()[rows][:, :width]))), rows


def _check(nat, D, xo, cols, yo, rows, out_bytes, r=None):
    got = nat.levenshtein_long_dense(xo, yo, out_bytes=out_bytes, rows=r)
    r0, r1 = (0, len(rows)) if r is None else r
    assert got.shape == (r1 - r0, len(cols)) and got.dtype == (torch.float16 if out_bytes == 2 else torch.int64) and got.is_cuda
    assert np.array_equal(got.cpu().numpy().astype(np.int64), D[np.ix_(rows[r0:r1], cols)])


# ---------------------------------------------------------------- 1. the dense kernel
@pytest.mark.parametrize("M", [1, 16, 17])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_dense_kernel_as_windows_of_one_matrix(nat, D, M, N):
    """One lane per column, 64 columns per wave, 256 per workgroup, 16 rows per workgroup: one row, a full group, a group
    and one row; one lane, a wave less one, a wave, a wave and one lane, a workgroup and one lane.  Both output types."""
    xo, cols = _x(nat, 2048, N)
    yo, rows = _y(nat, 2048, M)
    assert xo.valid() and yo.valid()
    for out_bytes in (8, 2):
        _check(nat, D, xo, cols, yo, rows, out_bytes)


@pytest.mark.parametrize("xw, yw", [(129, 2048), (256, 257), (257, 129), (513, 1025), (1024, 2048), (1025, 1025), (2048, 256),
                                    (1, 2048), (2048, 1), (128, 300), (300, 128)])
def test_dense_kernel_at_every_block_count(nat, D, xw, yw):
    """The operands at their own widths: 2 blocks (129, 256), 3 (257: the instance for 4), 5 and 8 (the instance for 8),
    9 and 16 (the instance for 16), 1 (a narrow pattern under a wide text); the text in 1..16 chunks."""
    xo, cols = _x(nat, xw, 65)
    yo, rows = _y(nat, yw, 17)
    assert (xo.l, yo.l) == (xw, yw)
    _check(nat, D, xo, cols, yo, rows, 8 if (xw + yw) % 2 else 2)


def test_dense_kernel_row_ranges_and_the_transposed_call(nat, D):
    xo, cols = _x(nat, 2048, 70)
    yo, rows = _y(nat, 2048, 40)
    _check(nat, D, xo, cols, yo, rows, 2, r=(5, 38))                       # starts inside a group of 16, ends inside one
    _check(nat, D, xo, cols, yo, rows, 8, r=(17, 18))
    got = nat.levenshtein_long_dense(yo, xo, out_bytes=8)                  # the X rows as texts, the Y rows as patterns
    assert np.array_equal(got.cpu().numpy(), D[np.ix_(rows, cols)].T)
    xs, cs = _x(nat, 300, 70)
    got = nat.levenshtein_long_dense(yo, xs, out_bytes=2, rows=(3, 69))    # 16 pattern blocks under 3 chunks of text
    assert np.array_equal(got.cpu().numpy().astype(np.int64), D[np.ix_(rows, cs[3:69])].T)


# ---------------------------------------------------------------- 2. closed forms at full length
def test_closed_forms_at_full_length(nat):
    lens = np.array([0, 1, 127, 128, 129, 1024, 1025, 2047, 2048])
    H = np.zeros((len(lens), 2048), dtype=np.uint8)
    for r, l in zip(H, lens):
        r[:l] = 31
    ho = nat.lev_long_operand(torch.from_numpy(H))
    got = nat.levenshtein_long_dense(ho, ho, out_bytes=8).cpu().numpy()
    assert np.array_equal(got, np.abs(lens[:, None] - lens[None, :]))       # two homopolymers: |la - lb|
    R = np.random.default_rng(1).integers(1, 32, (5, 2048)).astype(np.uint8)
    R[4] = 0                                                                # the empty row
    ro = nat.lev_long_operand(torch.from_numpy(R))
    got = nat.levenshtein_long_dense(ro, ro, out_bytes=2).cpu().numpy()
    assert (np.diag(got) == 0).all()                                        # x against x
    assert (got[4, :4] == 2048).all() and (got[:4, 4] == 2048).all()        # the empty row against 2048 tokens


# ---------------------------------------------------------------- 3. the operator
def test_operator_on_the_long_set(D, monkeypatch):
    import sys
    monkeypatch.setattr(sys.modules["prograph_amd.distance.levenshtein"], "_torch_levenshtein", None)   # the kernel or nothing
    X, Y = torch.from_numpy(LL.long_x()).cuda(), torch.from_numpy(LL.long_y()).cuda()
    d = levenshtein(X, Y)
    assert d.is_cuda and d.dtype == torch.int64 and np.array_equal(d.cpu().numpy(), D)
    for dt in (torch.int64, torch.float16):
        assert torch.equal(levenshtein(X.to(dt), Y.to(dt)), d)
    s = levenshtein(X, Y, similarity=True)
    assert s.is_cuda and s.dtype == torch.float32 and torch.equal(s, 1 / (1 + d))
    narrow = levenshtein(X[:30, :129], Y[:5, :129])                          # 129 positions: the first width of the route
    assert np.array_equal(narrow.cpu().numpy(), LL.wagner_fischer_rows(LL.long_x()[:30, :129], LL.long_y()[:5, :129]))


# ---------------------------------------------------------------- 4. two independent kernels
def test_alignment_of_one_minus_identity_is_levenshtein(D):
    dist = alignment(1 - np.eye(32, dtype=np.int64), 1)
    X, Y = torch.from_numpy(LL.long_x()).cuda(), torch.from_numpy(LL.long_y()).cuda()
    got = dist(X, Y)
    assert torch.equal(got, levenshtein(X, Y)) and np.array_equal(got.cpu().numpy(), D)


# ---------------------------------------------------------------- 5. the surface
SURFACE_ROWS = [r for r, l in enumerate(LL.X_LENS) if l <= 600] + [LL.X_LENS.index(l) for l in (1025, 1535, 2048)]


@pytest.fixture(scope="module")
def surface(tmp_path_factory):
    """A Prograph of 47 strings, lengths 0..600 and three beyond 1024; a pickled frame, because a csv cannot hold the
    empty sequence.  With it the (47, 47) reference."""
    from prograph_amd import Prograph
    tok = np.ascontiguousarray(LL.long_x()[SURFACE_ROWS])
    f = tmp_path_factory.mktemp("levlong") / "long.pkl"
    seqs = LL.strings(tok)
    assert len(seqs) == 47 and seqs.count("") == 1 and sum(len(s) > 1024 for s in seqs) == 3
    pd.DataFrame({"Sequence": seqs, "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_pickle(str(f))
    P = Prograph(file=str(f), seed_seq=seqs[20], amino_acids=LL.ALPHABET)
    assert np.array_equal(P.tokenized, tok)
    return P, tok, LL.wagner_fischer_rows(tok, tok)


def _same_tuples(got, want_idx, want_w):
    assert len(got) == len(want_idx)
    for (gi, gw), wi, ww in zip(got, want_idx, want_w):
        assert len(gi) == len(wi)
        if len(wi):
            assert gi.dtype == np.int64 and gw.dtype == np.int64
        assert np.array_equal(gi, wi) and np.array_equal(gw, ww)


@pytest.mark.parametrize("k", [1, 16, 70])
def test_surface_knn_graph(surface, k):
    P, tok, DS = surface
    kk = min(k, len(tok) - 1)
    wi, wd = LL.knn_from_matrix(DS, kk, 1)
    G = P.build_graph(k=k, distance=levenshtein, output="csr")
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.first == 1 and G.idx.is_cuda
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    _same_tuples(P.build_graph(k=k, distance=levenshtein), wi, wd)


@pytest.mark.parametrize("comp", ["le", "lt", "eq", "ge"])
@pytest.mark.parametrize("eps", [0.5, 8, 9, 1500])
def test_surface_eps_graph(surface, comp, eps):
    P, tok, DS = surface
    want = LL.csr_from_matrix(DS, LT.OPS[comp], eps)
    G = P.build_graph(eps=eps, distance=levenshtein, comp=LT.OPS[comp], output="csr")
    ip, ix, w = (t.cpu().numpy() for t in (G.indptr, G.indices, G.weights))
    assert ip.dtype == np.int64 and ix.dtype == np.int32 and w.dtype == np.int16
    assert np.array_equal(ip, want[0]) and np.array_equal(ix, want[1]) and np.array_equal(w, want[2])
    if (comp, eps) in (("le", 8), ("lt", 9), ("ge", 1500), ("ge", 9)):
        assert want[0][-1] > 0


def test_surface_containers(surface):
    P, tok, DS = surface
    sub = np.arange(5, 40)
    wi, wd = LL.knn_from_matrix(DS[np.ix_(sub, sub)], 3, 1)
    _same_tuples(P.build_graph(k=3, distance=levenshtein, idxs=sub), wi, wd)
    sim = P.build_graph(k=3, distance=levenshtein, similarity=True, output="csr")
    want_s = (1 / (1 + torch.from_numpy(LL.knn_from_matrix(DS, 3, 1, np.int64)[1]))).numpy()
    assert all(np.array_equal(gw, ws) and gw.dtype == np.float32 for (_, gw), ws in zip(sim.to_tuples(), want_s))
    P.build_graph(eps=40, distance=levenshtein, store="L40")
    ip, ix, w = LL.csr_from_matrix(DS, operator.le, 40)
    assert ip[-1] > 0 and P._device_graph("L40") is not None                 # the analytics run from the device CSR
    assert np.array_equal(np.asarray(P.degree("L40", boolean_weights=True)).reshape(-1), np.diff(ip))
    assert np.array_equal(np.asarray(P.degree("L40")).reshape(-1), np.add.reduceat(np.append(w, 0), ip[:-1]) * (np.diff(ip) > 0))
    got = P.graph["L40"]
    assert all(np.array_equal(got[i][0], ix[ip[i]:ip[i + 1]]) and np.array_equal(got[i][1], w[ip[i]:ip[i + 1]]) for i in range(len(tok)))


def test_surface_search_and_single_sequence_queries(surface):
    P, tok, DS = surface
    p = LL.parent()
    Q = np.zeros((4, 2048), dtype=np.uint8)
    Q[0, :1] = p[:1]                                                        # one token
    Q[1, :129] = p[:129]
    Q[1, 128] = 1 + p[128] % 31                                             # 129 tokens, the last one changed
    Q[2] = tok[-1]                                                          # a dataset row of 2048 tokens: d = 0 is kept
    Q[3, :400] = p[100:500]
    DQ = LL.wagner_fischer_rows(tok, Q)
    qs = LL.strings(Q)
    assert [len(s) for s in qs] == [1, 129, 2048, 400]
    wi, wd = LL.knn_from_matrix(DQ, 5, 0)
    G = P.search(qs, k=5, distance=levenshtein, output="csr")
    assert G.first == 0 and G.nrows == 4 and G.ncols == len(tok) and G.dist.dtype == torch.int16
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd) and wd[2, 0] == 0
    _same_tuples(P.search(Q, k=5, distance=levenshtein), wi, wd)
    for one in (0, 1, 2):                                                   # queries of 1, 129 and 2048 tokens on their own
        _same_tuples(P.search(qs[one], k=3, distance=levenshtein), wi[one:one + 1, :3], wd[one:one + 1, :3])
    for comp, eps in (("le", 130), ("lt", 130), ("eq", 0), ("ge", 1900)):
        ip, ix, w = LL.csr_from_matrix(DQ, LT.OPS[comp], eps, keep_zero=True)
        assert ip[-1] > 0
        G = P.search(qs, eps=eps, distance=levenshtein, comp=LT.OPS[comp], output="csr")
        assert G.weights.dtype == torch.int16 and np.array_equal(G.indptr.cpu().numpy(), ip)
        assert np.array_equal(G.indices.cpu().numpy(), ix) and np.array_equal(G.weights.cpu().numpy(), w)
    rows, dmin = P.nearest_neighbour(qs[1], distance=levenshtein)
    assert list(rows.index) == [int(wi[1, 0])] and dmin == wd[1, 0]
    ip, ix, w = LL.csr_from_matrix(DQ, operator.le, 10, keep_zero=True)
    assert ip[2] > ip[1]
    assert list(P.neighbourhood(qs[1], 10, distance=levenshtein).index) == list(ix[ip[1]:ip[2]])
    assert np.array_equal(P.calc_neighbours(qs[3], eps=350, distance=levenshtein, comp=operator.lt), np.nonzero(DQ[3] < 350)[0])


def test_wide_query_against_a_narrow_dataset(tmp_path):
    from prograph_amd import Prograph
    rows = [r for r, l in enumerate(LL.X_LENS) if 1 <= l <= 128]
    tok = np.ascontiguousarray(LL.long_x()[rows][:, :128])
    seqs = LL.strings(tok)
    f = tmp_path / "narrow.pkl"
    pd.DataFrame({"Sequence": seqs, "Fitness": np.linspace(0, 1, len(tok))}).to_pickle(str(f))
    P = Prograph(file=str(f), seed_seq=seqs[-1], amino_acids=LL.ALPHABET)
    Q = np.ascontiguousarray(LL.long_y()[[4, 9]])                           # 129 and 1024 tokens
    DQ = LL.wagner_fischer_rows(tok, Q)
    wi, wd = LL.knn_from_matrix(DQ, 4, 0)
    G = P.search(LL.strings(Q), k=4, distance=levenshtein, output="csr")
    assert G.dist.dtype == torch.int16 and np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    short = P.search(seqs[:3], k=2, distance=levenshtein, output="csr")     # and a narrow one: the one-word kernel, uint8
    assert short.dist.dtype == torch.uint8 and (short.dist[:, 0] == 0).all()


# ---------------------------------------------------------------- 6. the short route was not re-routed
def test_short_datasets_keep_their_route_and_weights(tmp_path):
    from prograph_amd import Prograph, synth
    tok = LT.set_a()[:200]
    f = tmp_path / "short.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": np.linspace(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    G = P.build_graph(k=16, distance=levenshtein, output="csr")
    wi, wd = LT.knn_from_matrix(LT.pair_matrix(tok, tok), 16, 1)
    assert G.dist.dtype == torch.uint8 and np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
