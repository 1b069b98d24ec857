"""
Local alignment scores (`distance.local_alignment`) without a GPU.

Two statements of the definition live in tests/local_testdata.py and are held against each other here: `definition`, the
recurrence as a numpy double loop, and `brute_force`, every pair of substrings and every alignment path of them.
Everything else - the operator's torch expression on CPU tensors, the stand-in of tests/fake_local_native.py behind the
graph / search routes, and on the GPU the kernel (tests/test_local_alignment_gpu.py) - is compared with `definition`.
"""
import ctypes
import operator
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import fake_aln_native
import fake_local_native
from local_testdata import brute_force, csr_of, definition, knn_of, lengths, rows_of, score_table
from prograph_amd import synth
from prograph_amd.distance import alignment, local_alignment


# ---------------------------------------------------------------- (a) the recurrence against (b) every path
@pytest.mark.parametrize("gap,gap_open", [(1, 0), (2, 3), (1, 4)])
def test_the_recurrence_is_the_best_local_alignment_path(gap, gap_open):
    """Sequences of 0..4 symbols out of three (symbol 0 only inside a sequence: a trailing zero is padding), two of every
    length and both orders of every pair; a table with negative entries; gaps that pay (1, 0), that rarely pay, and an
    open above every score."""
    rng = np.random.default_rng(10 * gap + gap_open)
    S = np.array([[2, -1, -3], [-1, 3, -2], [-3, -2, 4]])
    seqs = np.zeros((10, 4), dtype=np.int64)
    for r in range(10):
        l = r // 2
        seqs[r, :l] = rng.integers(0, 3, l)
        if l:
            seqs[r, l - 1] = rng.integers(1, 3)                   # the last symbol is not the padding value
    lens = lengths(seqs)
    assert sorted(lens) == sorted(list(range(5)) * 2) and (seqs[:, :3] == 0).any()
    D = definition(S, gap, gap_open, seqs, seqs)
    for r in range(10):
        for c in range(10):
            assert D[r, c] == brute_force(S, gap, gap_open, list(seqs[c, :lens[c]]), list(seqs[r, :lens[r]])), (r, c)
    assert np.array_equal(D, D.T) and (D >= 0).all() and (D[:2] == 0).all()
    assert (D <= np.minimum(lens[:, None], lens[None, :]) * S.max()).all()
    assert np.array_equal(fake_local_native.recurrence(S, gap, gap_open, seqs, seqs), D)


def test_a_gap_that_pays_and_one_that_does_not():
    S = np.array([[0, -5, -5], [-5, 4, -5], [-5, -5, 4]])
    x, y = np.array([[1, 2, 1, 2, 1, 2]]), np.array([[1, 2, 1, 1, 2, 1, 2]])       # y = x with one symbol inserted
    for f in (definition, lambda *a: brute_force(a[0], a[1], a[2], list(a[3][0]), list(a[4][0]))):
        assert int(np.asarray(f(S, 1, 2, x, y)).reshape(-1)[0]) == 6 * 4 - 3       # one run of one: open 2 + 1
        assert int(np.asarray(f(S, 1, 20, x, y)).reshape(-1)[0]) == 4 * 4          # too dear: the longer flank alone
    assert int(local_alignment(S, 1, 2)(torch.from_numpy(x), torch.from_numpy(y))) == 21


# ---------------------------------------------------------------- the constructor
def test_constructor_rules():
    rng = np.random.default_rng(0)
    good = score_table(rng, 5, -128, 127)
    good[0, 0] = -7                                               # no rule for the diagonal
    good[1, 2] = good[2, 1] = 127
    op = local_alignment(good, 7, gap_open=11)
    assert op.gap == 7 and op.gap_open == 11 and op.symbols == 5 and op.max_score == 127
    assert op.table.dtype == np.int8 and np.array_equal(op.table, good) and not op.table.flags.writeable
    keep = good.copy()
    good[1, 1] = 99                                               # copied: later edits do not reach the operator
    assert np.array_equal(op.table, keep)
    good = keep
    assert local_alignment(torch.from_numpy(good), 1).gap_open == 0 and local_alignment(good.astype(np.float64), 3.0, 2.0).gap == 3
    assert repr(local_alignment(good, 7)) == repr(local_alignment(good, 7, gap_open=0)) \
        == f"local_alignment(<5 x 5 table, scores {good.min()}..127>, gap=7)"
    assert repr(op) == f"local_alignment(<5 x 5 table, scores {good.min()}..127>, gap=7, gap_open=11)"
    for name in ("table", "gap", "gap_open", "symbols", "max_score"):
        with pytest.raises(AttributeError):
            setattr(op, name, 3)
    bad_tables = [good[:, :4], good[:1, :1], np.zeros((33, 33), dtype=np.int64) + 1, good + 0.5, good.astype(bool),
                  np.where(np.eye(5, dtype=bool), 128, good), np.where(np.eye(5, dtype=bool), -129, good),
                  good + np.triu(np.ones((5, 5), dtype=np.int64), 1), np.minimum(good, 0), -np.abs(good) - 1, good.reshape(-1)]
    for T in bad_tables:
        with pytest.raises(ValueError):
            local_alignment(T, 5)
    local_alignment(np.array([[0, 1], [1, 0]]), 1)                # two symbols, the only positive entry off the diagonal
    local_alignment(np.ones((32, 32), dtype=np.int64), 1)
    for g in (0, 256, -1, 2.5, True, None, "3", float("nan")):
        with pytest.raises(ValueError):
            local_alignment(good, g)
    for o in (-1, 256, 2.5, True, None, "3", float("inf")):
        with pytest.raises(ValueError):
            local_alignment(good, 5, gap_open=o)
    assert local_alignment(good, 255, gap_open=255).gap_open == 255


def test_a_score_is_a_similarity():
    op = local_alignment(np.array([[1, -1], [-1, 2]]), 1)
    X = torch.tensor([[1, 1, 0]])
    assert torch.equal(op(X, X), op(X, X, similarity=True)) and int(op(X, X)) == 4
    with pytest.raises(ValueError, match="similarity"):
        op(X, X, similarity=False)
    with pytest.raises(ValueError):
        op(X[:0], X)                                              # an empty operand
    with pytest.raises(ValueError):
        op(X, X[:0])
    with pytest.raises(ValueError):
        op(torch.tensor([[1, 2]]), X)                             # a token outside the table
    with pytest.raises(ValueError):
        op(X, torch.tensor([[0.5, 1]]))


# ---------------------------------------------------------------- the operator on the host
@pytest.mark.parametrize("a,gap,gap_open", [(21, 1, 0), (21, 3, 11), (32, 255, 255), (32, 1, 255), (5, 2, 1)])
def test_operator_against_the_definition_on_cpu_tensors(a, gap, gap_open):
    rng = np.random.default_rng(100 * a + gap + gap_open)
    S = score_table(rng, a, -9, 6, diag=np.arange(2, 12))
    S[0, :] = S[:, 0] = rng.integers(1, 9)                        # padding would score if it were let in
    op = local_alignment(S, gap, gap_open=gap_open)
    X = rows_of(rng, a, [0, 1, 15, 16, 17, 33] + list(rng.integers(0, 41, 34)), 40)         # tokens up to a - 1
    Y = rows_of(rng, a, [0, 1, 15, 16, 17, 33, 5], 33)            # unequal widths
    X[9] = 0                                                      # empty rows on both sides
    X[::4, 2], Y[3, 7], Y[4, 0] = 0, 0, 0                         # interior zeros: symbol 0 of the table
    X[5, :] = 0
    X[5, 9] = a - 1                                               # leading zeros count: length 10
    X[6, :33] = Y[5]                                              # something to find
    assert X.max() == a - 1 and lengths(X)[0] == 0 and lengths(X)[5] == 10
    want = definition(S, gap, gap_open, X, Y)
    s = op(torch.from_numpy(X), torch.from_numpy(Y))
    assert s.shape == (7, 40) and s.dtype == torch.int64 and s.device.type == "cpu"
    assert np.array_equal(s.numpy(), want)
    assert (want[0] == 0).all() and (want[:, 0] == 0).all() and (want[:, 9] == 0).all() and want.max() > 60
    lx, ly = lengths(X), lengths(Y)
    assert (want <= np.minimum(lx[None, :], ly[:, None]) * S.max()).all() and (want >= 0).all()
    assert np.array_equal(op(torch.from_numpy(Y), torch.from_numpy(X)).numpy(), want.T)      # symmetric
    one = op(torch.from_numpy(X), torch.from_numpy(Y[2]))         # a 1-D operand
    assert one.shape == (1, 40) and np.array_equal(one.numpy(), want[2:3])
    padded = op(torch.from_numpy(np.pad(X, ((0, 0), (0, 9)))), torch.from_numpy(Y))         # padding changes nothing
    assert np.array_equal(padded.numpy(), want)
    for dt in (torch.uint8, torch.int32, torch.float64):
        assert np.array_equal(op(torch.from_numpy(X).to(dt), torch.from_numpy(Y).to(dt)).numpy(), want)
    mod = sys.modules["prograph_amd.distance.local_alignment"]    # (the package attribute of that name is the class)
    old = mod._DP_ELEMS
    try:
        mod._DP_ELEMS = 41 * 9 * 2                                # blocks of the table do not change the result
        assert np.array_equal(op(torch.from_numpy(X), torch.from_numpy(Y)).numpy(), want)
    finally:
        mod._DP_ELEMS = old
    assert np.array_equal(fake_local_native.recurrence(S, gap, gap_open, X, Y), want)       # the stand-in's own loop


def test_width_130_on_the_host():
    rng = np.random.default_rng(7)
    S = score_table(rng, 21, -6, 3, diag=np.arange(3, 9))
    X, Y = rows_of(rng, 21, [130, 129, 64, 0, 7], 130), rows_of(rng, 21, [130, 100, 1], 130)
    X[2, 10:50] = Y[0, 80:120]
    want = definition(S, 2, 5, X, Y)
    assert np.array_equal(local_alignment(S, 2, 5)(torch.from_numpy(X), torch.from_numpy(Y)).numpy(), want)
    assert want[0, 2] >= 40 * 3


def test_self_score_and_fragment_against_parent():
    rng = np.random.default_rng(3)
    diag = np.array([-5, 1, 2, 3, 4, 5, 6, 7, -3, 10])
    S = np.full((10, 10), -50)
    S[np.arange(10), np.arange(10)] = diag
    op = local_alignment(S, 200)                                  # no gap pays: 15 symbols score at most 150
    X = rows_of(rng, 10, rng.integers(1, 16, 40), 15, low=0)
    s = op(torch.from_numpy(X), torch.from_numpy(X)).numpy()
    for r, l in enumerate(lengths(X)):
        d = diag[X[r, :l]]
        runs = max([d[i:j].sum() for i in range(l) for j in range(i + 1, l + 1)] + [0])
        assert s[r, r] == runs, r                                 # the best run of the diagonal
    assert np.array_equal(s, definition(S, 200, 0, X, X))
    # a fragment against the sequence it was cut from scores what it scores against itself
    S = score_table(rng, 21, -8, -1, diag=np.arange(4, 12))      # every symbol likes itself best
    parent = rows_of(rng, 21, [120] * 6, 120)
    frag = np.zeros((6, 40), dtype=np.int64)
    for r in range(6):
        frag[r, :40 - 3 * r] = parent[r, 11 * r:11 * r + 40 - 3 * r]
    for gap, gap_open in ((1, 0), (4, 9)):
        op = local_alignment(S, gap, gap_open)
        both = op(torch.from_numpy(parent), torch.from_numpy(frag)).numpy()
        own = op(torch.from_numpy(frag), torch.from_numpy(frag)).numpy()
        assert np.array_equal(np.diag(both), np.diag(own)) and (np.diag(own) == [S[f[f > 0], f[f > 0]].sum() for f in frag]).all()
        cost = np.where(np.eye(21, dtype=bool), 0, 3)
        assert (np.diag(alignment(cost, gap, gap_open)(torch.from_numpy(parent), torch.from_numpy(frag)).numpy()) >= 80 * gap).all()


# ---------------------------------------------------------------- host logic through the stand-in
N, L = 120, 24


@pytest.fixture()
def pg(tmp_path, monkeypatch):
    fake_local_native.install(monkeypatch)
    from prograph_amd import Prograph
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=16, seed=5, members=12)
    tok = tok.copy()
    tok[7] = tok[8]
    assert lengths(tok).max() == L
    f = tmp_path / "local.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    del fake_aln_native.calls[:]
    return P, tok


def _arrays(got):
    return np.array([i for i, _ in got]), np.array([w for _, w in got])


def _same_csr(got, ip, ix, w):
    assert len(got) == len(ip) - 1
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]]), i


def test_graph_and_search_routes(pg):
    from prograph_amd import _native
    P, tok = pg
    calls = fake_aln_native.calls
    rng = np.random.default_rng(3)
    S = score_table(rng, 21, -4, 1, diag=np.arange(2, 6))
    op = local_alignment(S, 3, gap_open=2)
    D = definition(S, 3, 2, tok, tok)
    G = P.build_graph(k=5, distance=op, output="csr")
    assert calls == [("operand", N, L, 21), ("score", 21), ("local_dense", N, 2, 3, 2), ("f16_knn", 5, 1, True)]
    wi, wd = knn_of(D, 5, 1)
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.first == 1 and G.similarity is False
    assert np.array_equal(G.idx.numpy(), wi) and np.array_equal(G.dist.numpy(), wd)
    for sim in (False, True):                                     # `similarity` is not consulted: the weights are the scores
        gi, gw = _arrays(P.build_graph(k=5, distance=op, similarity=sim))
        assert gw.dtype == np.int64 and np.array_equal(gi, wi) and np.array_equal(gw, wd)
    # eps: comp(eps, s) & s > 0 without the diagonal; the kernels test (value, threshold), so the comparator is mirrored
    mid = int(np.median(D[D > 0]))
    for name, comp, eps, thr in (("ge", operator.le, mid, float(mid)), ("gt", operator.lt, mid - 0.5, float(mid - 1)),
                                 ("eq", operator.eq, mid, float(mid)), ("le", operator.ge, 3.5, 3.0), ("lt", operator.gt, 4, 4.0),
                                 ("eq", operator.eq, 10.5, -1.0)):
        del calls[:]
        G = P.build_graph(eps=eps, distance=op, comp=comp, output="csr")
        assert calls[:2] == [("operand", N, L, 21), ("local_dense", N, 2, 3, 2)]
        assert calls[-1] == ("f16_eps", getattr(_native, "CMP_" + name.upper()), thr, False, False), calls
        ip, ix, w = csr_of(D, comp, eps, diagonal=False)
        assert G.weights.dtype == torch.int16 and G.similarity is False and np.array_equal(G.indptr.numpy(), ip)
        assert np.array_equal(G.indices.numpy(), ix) and np.array_equal(G.weights.numpy(), w)
        assert not (G.indices.numpy() == np.repeat(np.arange(N), np.diff(ip))).any()
    assert (np.diag(D) >= mid).all() and csr_of(D, operator.le, mid)[0][-1] == csr_of(D, operator.le, mid, diagonal=False)[0][-1] + N
    _same_csr(P.build_graph(eps=mid, distance=op), *csr_of(D, operator.le, mid, diagonal=False))      # the default comp: s >= eps
    # a subset: the diagonal is the position within the subset
    sub = np.arange(50, 120)
    del calls[:]
    got = P.build_graph(eps=mid, distance=op, idxs=sub)
    assert calls[:2] == [("operand", 70, L, 21), ("local_dense", 70, 2, 3, 2)]
    ip, ix, w = csr_of(D[np.ix_(sub, sub)], operator.le, mid, diagonal=False)
    assert ip[-1] > 0
    _same_csr(got, ip, ix, w)
    gi, gw = _arrays(P.build_graph(k=70, distance=op, idxs=sub))  # n - 1 = 69 ranks exist
    wi, wd = knn_of(D[np.ix_(sub, sub)], 69, 1)
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd)
    # search: rank 0 kept, queries wider than the dataset
    Q = np.zeros((5, L + 9), dtype=np.int64)
    Q[:, :L] = tok[[3, 50, 99, 100, 8]]
    Q[3, L:L + 6] = rng.integers(1, 21, 6)                        # longer than the dataset's rows
    Q[2, 11:] = 0                                                 # shorter
    DQ = definition(S, 3, 2, tok, Q)
    del calls[:]
    gi, gw = _arrays(P.search(Q, k=6, distance=op))
    assert calls == [("operand", N, L, 21), ("operand", 5, L + 9, 21), ("local_dense", 5, 2, 3, 2), ("f16_knn", 6, 0, True)]
    wi, wd = knn_of(DQ, 6, 0)
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd) and list(wi[4, :2]) == [7, 8] and wd[4, 0] == D[8, 8]
    assert np.array_equal(_arrays(P.search(Q, k=6, distance=op, similarity=True))[1], wd)
    del calls[:]
    got = P.search(Q, eps=mid, distance=op)
    assert calls[-1] == ("f16_eps", _native.CMP_GE, float(mid), False, False)
    _same_csr(got, *csr_of(DQ, operator.le, mid))                 # nothing is excluded but s = 0
    G = P.search(Q, eps=10_000, distance=op, comp=operator.ge, output="csr")                   # s <= eps: every s > 0
    _same_csr(G.to_tuples(), *csr_of(DQ, operator.ge, 10_000))
    assert G.nnz == (DQ > 0).sum() and G.weights.dtype == torch.int16
    hit, best = P.nearest_neighbour(synth.tokens_to_strings(tok[50:51])[0], distance=op)
    assert list(hit.index) == [int(wi[1, 0])] and best == wd[1, 0]
    with pytest.raises(ValueError):
        P.search(np.array([[1, 21]]), k=1, distance=op)           # a token outside the table: no generic loop
    st = P.build_graph(k=4, distance=op, store="Local", output="csr")
    assert "Local" in P.csr_graphs and np.array_equal(P.degree("Local"), knn_of(D, 4, 1)[1].sum(1).astype(np.float32))


def test_routes_at_and_beyond_the_bounds(pg):
    P, tok = pg
    calls = fake_aln_native.calls
    rng = np.random.default_rng(4)
    rows = np.arange(N - 12, N)
    narrow, wide = rows_of(rng, 21, rng.integers(1, 17, 12), 16), rows_of(rng, 21, rng.integers(100, 129, 12), 128)
    over = rows_of(rng, 21, rng.integers(100, 130, 12), 129)
    narrow[5, :8] = narrow[2, 4:12]
    P.graph["W16"] = list(narrow[:1]) * (N - 12) + list(narrow)
    P.graph["W128"] = list(wide[:1]) * (N - 12) + list(wide)
    P.graph["W129"] = list(over[:1]) * (N - 12) + list(over)

    def table(top):
        S = score_table(rng, 21, -5, 2, diag=[3, 4])
        S[3, 3] = top
        return S
    # width * max_score: 16 * 127 = 2032 and 128 * 16 = 2048 are native, 128 * 17 = 2176 and 129 positions are not.  An int8
    # table cannot meet 2049 within 128 positions (2049 = 3 * 683), so the condition itself is held at 2048 / 2049 below
    for rep, mat, top, native in (("W16", narrow, 127, True), ("W128", wide, 16, True), ("W128", wide, 17, False),
                                  ("W129", over, 4, False)):
        S = table(top)
        op = local_alignment(S, 2, 1)
        assert P._local_native(mat.shape[1], op) is native
        del calls[:]
        gi, gw = _arrays(P.build_graph(k=3, distance=op, representation=rep, idxs=rows))
        assert [c[0] for c in calls if "dense" in c[0]] == (["local_dense"] if native else []), (rep, top)
        assert bool(calls) is native                              # outside: the operator's torch blocks, no native call
        D = definition(S, 2, 1, mat, mat)
        wi, wd = knn_of(D, 3, 1)
        assert np.array_equal(gi, wi) and np.array_equal(gw, wd), (rep, top)
        ip, ix, w = csr_of(D, operator.le, 6, diagonal=False)
        _same_csr(P.build_graph(eps=6, distance=op, representation=rep, idxs=rows), ip, ix, w)
    op = local_alignment(table(4), 2)

    class W:                                                      # the condition itself at 2048 and 2049
        max_score = 683
    assert P._local_native(3, W) is False and 3 * 683 == 2049
    W.max_score = 16
    assert P._local_native(128, W) is True and P._local_native(129, W) is False
    W.max_score = 1024
    assert P._local_native(2, W) is True and 2 * 1024 == 2048
    # search: the wider of dataset and queries counts
    S = table(17)
    del calls[:]
    gi, gw = _arrays(P.search(wide[:3], k=2, distance=local_alignment(S, 2, 1)))
    wi, wd = knn_of(definition(S, 2, 1, tok, wide[:3]), 2, 0)
    assert not calls and np.array_equal(gi, wi) and np.array_equal(gw, wd)
    S = table(16)
    gi, gw = _arrays(P.search(wide[:3], k=2, distance=local_alignment(S, 2, 1)))
    assert ("local_dense", 3, 2, 2, 1) in calls
    wi, wd = knn_of(definition(S, 2, 1, tok, wide[:3]), 2, 0)
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd)
    # a comp outside the five orderings: the torch selection, the same edge set
    del calls[:]
    got = P.build_graph(eps=5, distance=op, comp=lambda t, s: t <= s, idxs=np.arange(30))
    assert not calls
    _same_csr(got, *csr_of(definition(op.table, 2, 0, tok[:30], tok[:30]), operator.le, 5, diagonal=False))


def test_block_rows(pg, monkeypatch):
    P, tok = pg
    calls = fake_aln_native.calls
    op = local_alignment(score_table(np.random.default_rng(6), 21, -4, 1, diag=[2, 3]), 2, gap_open=3)
    D = definition(op.table, 2, 3, tok, tok)
    monkeypatch.setattr(type(P), "_BLOCK_ELEMS", N * 3)
    gi, gw = _arrays(P.build_graph(k=4, distance=op))
    assert [c[1] for c in calls if c[0] == "local_dense"] == [64, 56]                  # never below 64 rows
    assert np.array_equal(gi, knn_of(D, 4, 1)[0])
    del calls[:]
    P.search(tok[:7], k=4, distance=op)
    assert [c[1] for c in calls if c[0] == "local_dense"] == [3, 3, 1]                 # queries: down to one row
    monkeypatch.setattr(type(P), "_BLOCK_ELEMS", N * 100)
    del calls[:]
    got = P.build_graph(eps=12, distance=op)
    assert [c[1] for c in calls if c[0] == "local_dense"] == [100, 20]
    _same_csr(got, *csr_of(D, operator.le, 12, diagonal=False))   # the diagonal of the second block is at columns 100..119
    del calls[:]
    P.search(tok[:7], eps=12, distance=op)
    assert [c[1] for c in calls if c[0] == "local_dense"] == [7]
    assert not [c for c in calls if c[0] in ("dense", "affine_dense")]


# ---------------------------------------------------------------- the C entry's argument checks
def test_argument_checks_of_the_c_entry_without_a_gpu():
    """`pg_alignment_local_dense` returns the PG_E_* of `pg_alignment_affine_dense` before any launch."""
    from prograph_amd import _native
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                      # never dereferenced on the host
    ok = dict(x=p, n=4, xnpad=256, xl=16, y=p, m=3, ynpad=256, yl=16, score=p, gap=2, gap_open=5, out=p, ldo=4, ob=8, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.pg_alignment_local_dense(a["x"], a["n"], a["xnpad"], a["xl"], a["y"], a["m"], a["ynpad"], a["yl"], a["score"],
                                            a["gap"], a["gap_open"], a["out"], a["ldo"], a["ob"], a["stream"])

    BADARG, TOOLONG = -1, -2
    for kw in (dict(x=None), dict(y=None), dict(score=None), dict(out=None), dict(n=0), dict(m=0), dict(xl=0), dict(yl=0),
               dict(ldo=3), dict(gap=0), dict(gap=256), dict(gap_open=-1), dict(gap_open=256), dict(xnpad=255), dict(xnpad=3),
               dict(ynpad=2), dict(ob=4)):
        assert call(**kw) == BADARG, kw
        assert b"pg_alignment_local_dense" in lib.pg_last_error()
    for kw in (dict(xl=129), dict(yl=129)):
        assert call(**kw) == TOOLONG, kw
        assert b"at most 128 positions" in lib.pg_last_error()
    assert lib.pg_version() == 3 and "pg_alignment_local_dense" in _native.SYMBOLS
    with pytest.raises(ValueError):
        _native.alignment_local_dense(None, None, None, 1, 1, out_bytes=4)
    with pytest.raises(ValueError):
        _native.aln_local_score(np.full((3, 3), 128))
