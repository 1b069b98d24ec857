"""
The Levenshtein kernels at every length and word boundary, on set B of tests/lev_testdata.py: 441 rows whose lengths
walk through 0, 1, 2, 7..9, 30..34, 62..66, 95..97, 127, 128 - homopolymers (the carry chain through all four dwords of
the 128-bit pattern), periodic strings and their shifts, pieces and mutants of one parent, duplicates, unrelated rows,
tokens up to 31.  `pg_levenshtein_dense` as windows of one reference matrix, the banded kNN at every band against the
oracle's lists, the exact epsilon graph at every threshold, and the Prograph surface on top of them.  Every comparison
is an every-entry equality; tests/test_levenshtein_lengths_cpu.py pins the reference (C oracle == numpy Wagner-Fischer)
and asserts that set B holds the cases these tests are about.
"""
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import lev_testdata as LT
from oracle import c_oracle as C
from prograph_amd.distance import alignment, levenshtein

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

ALPHABET = "ACDEFGHIKLMNPQRSTVWYBJOUXZabcde"      # 31 letters: token t is letter t - 1
Y0, YM, XN = 200, 77, 420                         # the dense tests' matrix: rows Y0..Y0+YM of set B against its first XN rows


@pytest.fixture(scope="module")
def B():
    return np.array(LT.set_b())                   # a writable copy for torch.from_numpy


@pytest.fixture(scope="module")
def D():
    return LT.set_b_matrix()


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def operand(nat, T):
    op = nat.lev_operand(torch.from_numpy(np.ascontiguousarray(T)))
    assert op.valid()
    return op


def own_width(T):
    """The rows cut to the longest of them (at least one position): operands go in at their own widths."""
    return T[:, :max(1, int(LT.lengths(T).max(initial=0)))]


def strings(T):
    lut = np.array([""] + list(ALPHABET))
    return ["".join(lut[r[r > 0]]) for r in np.asarray(T)]


def _same_csr(got, want):
    """`got`: a CSRGraph or the (indptr, indices, weights) tensors of `_native.levenshtein_eps`."""
    ip, ix, w = (t.cpu().numpy() for t in (got if isinstance(got, tuple) else (got.indptr, got.indices, got.weights)))
    assert ip.dtype == np.int64 and ix.dtype == np.int32 and w.dtype == np.uint8
    assert np.array_equal(ip, want[0]) and np.array_equal(ix, want[1]) and np.array_equal(w, want[2])


def _same_tuples(got, want_idx, want_w):
    assert len(got) == len(want_idx)
    for (gi, gw), wi, ww in zip(got, want_idx, want_w):
        assert not len(wi) or (gi.dtype == np.int64 and gw.dtype == np.int64)
        assert np.array_equal(gi, wi) and np.array_equal(gw, ww)


# ---------------------------------------------------------------- 1. pg_levenshtein_dense
def test_dense_kernel_as_windows_of_one_matrix(nat, B, D):
    """One lane per column, 64 columns per wave, 256 per workgroup, PG_LEVD_ROWS = 16 rows per workgroup.  Row r of set B
    has length LENS[r % 21], so every (M, N) shape is a window of the one reference matrix, taken from offsets that bring
    every length to every lane and every row slot (asserted below); the operands go in at their own widths, the output
    types alternate."""
    want = D[Y0:Y0 + YM, :XN]
    lanes, slots, widths, types = set(), set(), set(), set()
    c = 0
    for M in (1, 15, 16, 17, 33):
        for N in (1, 63, 64, 65, 255, 257):
            for t in range(3):
                o, p = (4 * c) % 21 + 21 * (t % 2), c % 21 + 21 * (c % 5)
                assert o + M <= YM and p + N <= XN
                X, Y = own_width(B[p:p + N]), own_width(B[Y0 + o:Y0 + o + M])
                ob = (8, 2)[c % 2]
                got = nat.levenshtein_dense(operand(nat, X), operand(nat, Y), out_bytes=ob)
                assert got.dtype == (torch.int64 if ob == 8 else torch.float16) and got.shape == (M, N)
                assert np.array_equal(got.cpu().numpy().astype(np.int64), want[o:o + M, p:p + N]), (M, N, o, p, ob)
                lanes |= {(col % 64, (p + col) % 21) for col in range(N)}
                slots |= {(r % 16, (Y0 + o + r) % 21) for r in range(M)}
                widths |= {X.shape[1], Y.shape[1]}
                types.add((M, N, ob))
                c += 1
    assert len(lanes) == 64 * 21 and len(slots) == 16 * 21 and {1, 2, 128} <= widths and len(types) == 60
    xo, yo = operand(nat, B[:XN]), operand(nat, B[Y0:Y0 + YM])              # both at the full width, zero padded
    for ob in (8, 2):
        got = nat.levenshtein_dense(xo, yo, out_bytes=ob)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
        for r0, r1 in ((5, YM), (17, 50), (31, 32)):                      # a Y operand that starts inside a group of 16 rows
            rows = nat.levenshtein_dense(xo, yo, out_bytes=ob, rows=(r0, r1))
            assert rows.shape == (r1 - r0, XN) and np.array_equal(rows.cpu().numpy().astype(np.int64), want[r0:r1])
    narrow = operand(nat, B[0:1, :1])                                      # width 1 against width 128: l = max of the two
    assert narrow.l == 1 and np.array_equal(nat.levenshtein_dense(xo, narrow).cpu().numpy(), D[0:1, :XN])
    assert np.array_equal(nat.levenshtein_dense(narrow, yo).cpu().numpy(), D[Y0:Y0 + YM, 0:1])
    one = operand(nat, B[1:2, :1])                                         # a single token
    assert np.array_equal(nat.levenshtein_dense(one, yo, out_bytes=2).cpu().numpy().astype(np.int64), D[Y0:Y0 + YM, 1:2])


def test_dense_kernel_one_wave_of_64_lengths(nat, B):
    """64 lanes with 64 different lengths - the `rows` mask of every lane differs, the text loop is wave uniform -
    against texts of length 0, 32, 64, 96 and 128: homopolymers, periodic strings and pieces of the parent in turn."""
    rng = np.random.default_rng(64)
    lay = [LT.set_b_layout(r) for r in range(len(B))]
    parent = B[next(r for r, (l, f, v) in enumerate(lay) if (l, f, v) == (128, "parent_piece", 0))]
    must = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128]
    lens = must + [int(l) for l in rng.permutation(np.setdiff1d(np.arange(129), must))[:64 - len(must)]]
    lens = [lens[i] for i in rng.permutation(64)]

    def row(l, kind):
        out = np.zeros(128, dtype=np.uint8)
        out[:l] = (np.full(l, 31), np.array([16, 31])[np.arange(l) % 2], parent[128 - l:])[kind]
        return out
    X = np.array([row(l, c % 3) for c, l in enumerate(lens)])
    Y = np.array([row(l, kind) for l in (0, 32, 64, 96, 128) for kind in range(3)])
    assert len(set(LT.lengths(X))) == 64 and len(X) == 64
    want = LT.oracle_pairs(X, Y)
    assert np.array_equal(want, LT.wagner_fischer(X, Y))
    for ob in (8, 2):
        got = nat.levenshtein_dense(operand(nat, X), operand(nat, Y), out_bytes=ob)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want)
    got = nat.levenshtein_dense(operand(nat, Y), operand(nat, X))           # and the other way round
    assert np.array_equal(got.cpu().numpy(), want.T)


def test_operator_on_set_b(B, D, monkeypatch):
    import sys
    monkeypatch.setattr(sys.modules["prograph_amd.distance.levenshtein"], "_torch_levenshtein", None)   # the kernel or nothing
    want = D[Y0:Y0 + YM, :XN]
    X, Y = torch.from_numpy(B[:XN]).cuda(), torch.from_numpy(B[Y0:Y0 + YM]).cuda()
    d = levenshtein(X, Y)
    assert d.is_cuda and d.dtype == torch.int64 and np.array_equal(d.cpu().numpy(), want)
    for dt in (torch.int64, torch.float16):
        assert torch.equal(levenshtein(X.to(dt), Y.to(dt)), d)
    s = levenshtein(X, Y, similarity=True)
    assert s.dtype == torch.float32 and torch.equal(s, 1 / (1 + d))
    Xs, Ys = torch.from_numpy(own_width(B[:11])).cuda(), torch.from_numpy(own_width(B[21:24])).cuda()     # widths 34 and 2
    assert Xs.shape[1] == 34 and Ys.shape[1] == 2
    assert np.array_equal(levenshtein(Xs, Ys).cpu().numpy(), D[21:24, :11])
    assert np.array_equal(levenshtein(Ys, Xs).cpu().numpy(), D[:11, 21:24])


# ---------------------------------------------------------------- 2. the banded kNN
@pytest.mark.parametrize("band", range(1, 9))
def test_banded_knn_against_the_oracle(nat, B, band, monkeypatch):
    """`_native.levenshtein_knn` = bag filter + pg_lev_select_kernel, with rectangular candidate slots (PG_EPS_SYM=0:
    one kernel, every candidate of a row evaluated by that row) and symmetric ones (1: every pair once, then selection)."""
    T = torch.from_numpy(B)
    want_idx, want_d = C.lev_knn(B, 63, band=band)
    for sym in ("0", "1"):
        monkeypatch.setenv("PG_EPS_SYM", sym)
        for k in (1, 8, 63):
            idx, d, st = nat.levenshtein_knn(T, k, band=band, return_stats=True)
            assert st["symmetric"] == (sym == "1") and st["filter_passes"] == 1
            assert idx.dtype == torch.int32 and d.dtype == torch.uint8
            assert np.array_equal(idx.cpu().numpy(), want_idx[:, :k]), (band, sym, k)
            assert np.array_equal(d.cpu().numpy(), want_d[:, :k]), (band, sym, k)
        idx, d, st = nat.levenshtein_knn(T, 8, band=band, cap=16, return_stats=True)     # rows outgrow 16 slots: the filter reruns
        assert st["filter_passes"] == 2 and st["cap"] > 16 and st["symmetric"] == (sym == "1")
        assert np.array_equal(idx.cpu().numpy(), want_idx[:, :8]) and np.array_equal(d.cpu().numpy(), want_d[:, :8])
        few_idx, few_d = nat.levenshtein_knn(T[:40], 63, band=band)         # N < k + 1: ranks that do not exist are (-1, 255)
        wi, wd = C.lev_knn(B[:40], 63, band=band)
        assert (wi[:, 39:] == -1).all() and (wd[:, 39:] == 255).all()
        assert np.array_equal(few_idx.cpu().numpy(), wi) and np.array_equal(few_d.cpu().numpy(), wd)
    for row0, nrows, k in ((37, 150, 8), (1, 439, 63), (430, 11, 1)):       # a window of rows: rectangular slots
        idx, d, st = nat.levenshtein_knn(T, k, band=band, row0=row0, nrows=nrows, return_stats=True)
        assert not st["symmetric"] and idx.shape == (nrows, k)
        assert np.array_equal(idx.cpu().numpy(), want_idx[row0:row0 + nrows, :k])
        assert np.array_equal(d.cpu().numpy(), want_d[row0:row0 + nrows, :k])


# ---------------------------------------------------------------- 3. the exact epsilon graph
@pytest.mark.parametrize("thr", range(9))
def test_exact_eps_graph_against_the_matrix(nat, B, D, thr, monkeypatch):
    """`_native.levenshtein_eps`: bag filter with band = thr over every unordered pair, the banded distance of every
    candidate pair once, count / scan / fill.  A row is no pair with itself, so the diagonal of the reference matrix is
    taken out; with keep_zero the exact duplicates (d = 0) are neighbours."""
    Dm = D.copy()
    np.fill_diagonal(Dm, -1)
    op = operand(nat, B)
    nnz = set()
    for name, code in (("le", nat.CMP_LE), ("lt", nat.CMP_LT), ("eq", nat.CMP_EQ)):
        for keep_zero in (False, True):
            want = LT.csr_from_matrix(Dm, LT.OPS[name], thr, keep_zero=keep_zero)
            _same_csr(nat.levenshtein_eps(op, code, thr, keep_zero=keep_zero), want)
            nnz.add(int(want[0][-1]))
    assert max(nnz) > 0 and (thr < 2 or min(nnz) > 0)
    calls = []
    real = nat.lib().pg_lev_candidates_sym
    monkeypatch.setattr(nat.lib(), "pg_lev_candidates_sym", lambda *a: (calls.append(a[4]), real(*a))[1])
    got = nat.levenshtein_eps(op, nat.CMP_LE, thr, cap=16, keep_zero=True)   # rows outgrow 16 slots: the filter reruns
    assert len(calls) == 2 and calls[0] == 16 and calls[1] > 16
    _same_csr(got, LT.csr_from_matrix(Dm, operator.le, thr, keep_zero=True))


# ---------------------------------------------------------------- 4. the surface
@pytest.fixture(scope="module")
def pg(B, tmp_path_factory):
    """A Prograph of set B's strings over a 31-letter alphabet; a pickled frame, because a csv cannot hold the empty
    sequence."""
    from prograph_amd import Prograph
    f = tmp_path_factory.mktemp("levb") / "set_b.pkl"
    seqs = strings(B)
    assert sorted(set(map(len, seqs))) == sorted(LT.LENS) and seqs.count("") >= 2
    pd.DataFrame({"Sequence": seqs, "Fitness": np.random.default_rng(0).uniform(0, 1, len(B))}).to_pickle(str(f))
    P = Prograph(file=str(f), seed_seq=seqs[20], amino_acids=ALPHABET)
    assert np.array_equal(P.tokenized, B)
    return P


@pytest.mark.parametrize("k", [1, 16, 70])
def test_surface_knn_graph(pg, D, k):
    """k <= 63: the banded kNN and the dense kernel for the rows whose k-th neighbour is beyond the band; 70: dense only."""
    wi, wd = LT.knn_from_matrix(D, k, 1)
    assert k > 63 or ((wd[:, k - 1] > 8).any() and (wd[:, k - 1] <= 8).any())          # both kinds of rows
    G = pg.build_graph(k=k, distance=levenshtein, output="csr")
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.uint8 and G.first == 1
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    _same_tuples(pg.build_graph(k=k, distance=levenshtein), wi, wd)


@pytest.mark.parametrize("comp,eps", [("le", 0), ("le", 0.5), ("le", 2), ("le", 8), ("le", 9), ("le", 40), ("eq", 2), ("lt", 9),
                                      ("ge", 120)])
def test_surface_eps_graph(pg, D, comp, eps):
    """Thresholds up to 8: the fused graph; beyond, and `ge`: the dense kernel plus the fp16 selection.  `build_graph`
    takes eps = 0 for "no eps", as the reference does; below 1 nothing but duplicates is within reach, and d > 0."""
    if eps == 0:
        with pytest.raises(ValueError):
            pg.build_graph(eps=eps, distance=levenshtein, comp=LT.OPS[comp], output="csr")
        return
    want = LT.csr_from_matrix(D, LT.OPS[comp], eps)
    assert (want[0][-1] > 0) == (eps >= 1) and want[0][-1] < D.size - len(D)
    G = pg.build_graph(eps=eps, distance=levenshtein, comp=LT.OPS[comp], output="csr")
    assert G.nrows == len(D)
    _same_csr(G, want)


def test_surface_search(pg, B, D):
    lay = [LT.set_b_layout(r) for r in range(len(B))]
    parent = B[next(r for r, (l, f, v) in enumerate(lay) if (l, f, v) == (128, "parent_piece", 0))]
    Q = np.zeros((6, 128), dtype=np.uint8)
    Q[0, :1] = 31                                                          # one token
    Q[1, :31] = parent[:31]
    Q[1, 30] = 1 + parent[30] % 31                                         # a prefix with its last token changed
    Q[2, :32] = 31                                                         # a homopolymer that fills one dword
    Q[3, :33] = np.array([31, 16])[np.arange(33) % 2]                      # period 2, one bit into the second dword
    Q[4] = np.concatenate([np.delete(parent, 64), [5]])                    # 128 tokens: the parent, one deletion, one more
    Q[5, :9] = parent[:9]                                                  # a row of the dataset
    assert list(LT.lengths(Q)) == [1, 31, 32, 33, 128, 9]
    qs = strings(Q)
    DQ = LT.oracle_pairs(B, Q)
    assert np.array_equal(DQ, LT.wagner_fischer(B, Q)) and DQ[5].min() == 0 and DQ[4].min() == 2 and DQ[1].min() == 1
    for q in (qs, Q.astype(np.int64)):
        for k in (1, 7, 70):
            wi, wd = LT.knn_from_matrix(DQ, k, 0)                          # rank 0 is kept
            _same_tuples(pg.search(q, k=k, distance=levenshtein), wi, wd)
        for comp, eps in (("le", 0), ("le", 3), ("le", 8), ("le", 40), ("eq", 1)):
            want = LT.csr_from_matrix(DQ, LT.OPS[comp], eps, keep_zero=True)
            assert want[0][-1] > 0
            G = pg.search(q, eps=eps, distance=levenshtein, comp=LT.OPS[comp], output="csr")
            _same_csr(G, want)
    K = pg.search(qs, k=7, distance=levenshtein, output="csr")
    wi, wd = LT.knn_from_matrix(DQ, 7, 0)
    assert K.first == 0 and np.array_equal(K.idx.cpu().numpy(), wi) and np.array_equal(K.dist.cpu().numpy(), wd)


def test_surface_alignment_of_one_minus_identity_is_levenshtein(pg, B, D):
    dist = alignment(1 - np.eye(32, dtype=np.int64), 1)
    T = torch.from_numpy(B).cuda()
    got = dist(T, T)
    assert torch.equal(got, levenshtein(T, T)) and np.array_equal(got.cpu().numpy(), D)
    G = pg.build_graph(k=16, distance=dist, output="csr")
    L = pg.build_graph(k=16, distance=levenshtein, output="csr")
    assert G.dist.dtype == torch.int16 and L.dist.dtype == torch.uint8                    # the device weight types differ
    assert torch.equal(G.idx, L.idx) and torch.equal(G.dist.long(), L.dist.long())
    wi, wd = LT.knn_from_matrix(D, 16, 1)
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
