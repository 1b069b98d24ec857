"""
Semi-global alignment scores (`distance.semiglobal_alignment`) without a GPU.

Two statements of the definition live in tests/semiglobal_testdata.py and are held against each other here: `definition`,
the recurrence as a numpy double loop, and `brute_force`, every free prefix / suffix choice and every alignment path of
the rest.  Everything else - the operator's torch expression on CPU tensors, the stand-in of
tests/fake_semiglobal_native.py behind the graph / search routes, and on the GPU the kernels
(tests/test_semiglobal_alignment_gpu.py, tests/test_semiglobal_alignment_long_gpu.py) - is compared with `definition`.
"""
import ctypes
import operator
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import fake_aln_native
import fake_semiglobal_native
from semiglobal_testdata import brute_force, csr_of, definition, knn_of, lengths, rows_of, score_table
from prograph_amd import synth
from prograph_amd.distance import local_alignment, semiglobal_alignment


# ---------------------------------------------------------------- (a) the recurrence against (b) the worded definition
@pytest.mark.parametrize("gap,gap_open", [(1, 0), (2, 3), (1, 4)])
def test_the_recurrence_is_the_best_end_gap_free_alignment(gap, gap_open):
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
    assert np.array_equal(semiglobal_alignment(S, gap, gap_open)(torch.from_numpy(seqs), torch.from_numpy(seqs)).numpy(), D)


# ---------------------------------------------------------------- the constructor
def test_constructor_rules():
    rng = np.random.default_rng(0)
    good = score_table(rng, 5, -128, 127)
    good[0, 0] = -7                                               # no rule for the diagonal
    good[1, 2] = good[2, 1] = 127
    op = semiglobal_alignment(good, 7, gap_open=11)
    assert op.gap == 7 and op.gap_open == 11 and op.symbols == 5 and op.max_score == 127
    assert op.table.dtype == np.int8 and np.array_equal(op.table, good) and not op.table.flags.writeable
    keep = good.copy()
    good[1, 1] = 99                                               # copied: later edits do not reach the operator
    assert np.array_equal(op.table, keep)
    good = keep
    assert semiglobal_alignment(torch.from_numpy(good), 1).gap_open == 0
    assert semiglobal_alignment(good.astype(np.float64), 3.0, 2.0).gap == 3
    assert repr(semiglobal_alignment(good, 7)) == repr(semiglobal_alignment(good, 7, gap_open=0)) \
        == f"semiglobal_alignment(<5 x 5 table, scores {good.min()}..127>, gap=7)"
    assert repr(op) == f"semiglobal_alignment(<5 x 5 table, scores {good.min()}..127>, gap=7, gap_open=11)"
    assert repr(local_alignment(good, 7)) == f"local_alignment(<5 x 5 table, scores {good.min()}..127>, gap=7)"
    assert not isinstance(op, local_alignment) and not isinstance(local_alignment(good, 7), semiglobal_alignment)
    for name in ("table", "gap", "gap_open", "symbols", "max_score"):
        with pytest.raises(AttributeError):
            setattr(op, name, 3)
    bad_tables = [good[:, :4], good[:1, :1], np.zeros((33, 33), dtype=np.int64) + 1, good + 0.5, good.astype(bool),
                  np.where(np.eye(5, dtype=bool), 128, good), np.where(np.eye(5, dtype=bool), -129, good),
                  good + np.triu(np.ones((5, 5), dtype=np.int64), 1), np.minimum(good, 0), -np.abs(good) - 1, good.reshape(-1)]
    for T in bad_tables:
        with pytest.raises(ValueError):
            semiglobal_alignment(T, 5)
    semiglobal_alignment(np.array([[0, 1], [1, 0]]), 1)           # two symbols, the only positive entry off the diagonal
    semiglobal_alignment(np.ones((32, 32), dtype=np.int64), 1)
    for g in (0, 256, -1, 2.5, True, None, "3", float("nan")):
        with pytest.raises(ValueError):
            semiglobal_alignment(good, g)
    for o in (-1, 256, 2.5, True, None, "3", float("inf")):
        with pytest.raises(ValueError):
            semiglobal_alignment(good, 5, gap_open=o)
    assert semiglobal_alignment(good, 255, gap_open=255).gap_open == 255


def test_a_score_is_a_similarity():
    op = semiglobal_alignment(np.array([[1, -1], [-1, 2]]), 1)
    X = torch.tensor([[1, 1, 0]])
    assert torch.equal(op(X, X), op(X, X, similarity=True)) and int(op(X, X)) == 4
    with pytest.raises(ValueError, match="semiglobal_alignment.*similarity"):
        op(X, X, similarity=False)
    with pytest.raises(ValueError):
        op(X[:0], X)                                              # an empty operand
    with pytest.raises(ValueError):
        op(X, X[:0])
    with pytest.raises(ValueError, match="semiglobal_alignment"):
        op(torch.tensor([[1, 2]]), X)                             # a token outside the table
    with pytest.raises(ValueError):
        op(X, torch.tensor([[0.5, 1]]))


# ---------------------------------------------------------------- the operator on the host
@pytest.mark.parametrize("a,gap,gap_open", [(21, 1, 0), (21, 3, 11), (32, 255, 255), (32, 1, 255), (5, 2, 1)])
def test_operator_against_the_definition_on_cpu_tensors(a, gap, gap_open):
    rng = np.random.default_rng(100 * a + gap + gap_open)
    S = score_table(rng, a, -9, 6, diag=np.arange(2, 12))
    S[0, :] = S[:, 0] = rng.integers(1, 9)                        # padding would score if it were let in
    op = semiglobal_alignment(S, gap, gap_open=gap_open)
    X = rows_of(rng, a, [0, 1, 15, 16, 17, 33] + list(rng.integers(0, 41, 34)), 40)         # tokens up to a - 1
    Y = rows_of(rng, a, [0, 1, 15, 16, 17, 33, 5], 33)            # unequal widths
    X[9] = 0                                                      # empty rows on both sides
    X[::4, 2], Y[3, 7], Y[4, 0] = 0, 0, 0                         # interior zeros: symbol 0 of the table
    X[5, :] = 0
    X[5, 9] = a - 1                                               # leading zeros count: length 10
    X[6, :33] = Y[5]                                              # the same row
    X[7, :] = 0
    X[7, :20] = Y[5, 13:]                                         # a suffix of a row
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
    mod = sys.modules["prograph_amd.distance.local_alignment"]    # the blocking both score operators share
    old = mod._DP_ELEMS
    try:
        mod._DP_ELEMS = 41 * 9 * 2                                # blocks of the table do not change the result
        assert np.array_equal(op(torch.from_numpy(X), torch.from_numpy(Y)).numpy(), want)
    finally:
        mod._DP_ELEMS = old


def test_width_130_on_the_host():
    rng = np.random.default_rng(7)
    S = score_table(rng, 21, -6, 3, diag=np.arange(3, 9))
    X, Y = rows_of(rng, 21, [130, 129, 64, 0, 7], 130), rows_of(rng, 21, [130, 100, 1], 130)
    X[2, 24:64] = Y[0, :40]                                       # x ends as y begins
    want = definition(S, 2, 5, X, Y)
    assert np.array_equal(semiglobal_alignment(S, 2, 5)(torch.from_numpy(X), torch.from_numpy(Y)).numpy(), want)
    assert want[0, 2] >= 40 * 3


def test_fragment_against_parent_and_one_internal_mismatch():
    """A fragment against the sequence it was cut from scores what it scores against itself - here and under
    `local_alignment`.  With the fragment's second symbol replaced (a mismatch costs 20, any gap more, a symbol is worth at
    most 11) the whole fragment must still align: this operator pays the mismatch and scores less than the intact
    fragment; `local_alignment` drops the first two symbols instead and scores more - not less than this operator in any
    case, being its relaxation.  The two differ."""
    rng = np.random.default_rng(3)
    S = np.full((21, 21), -20)
    S[np.arange(21), np.arange(21)] = rng.integers(4, 12, 21)    # every symbol likes itself best
    parent = rows_of(rng, 21, [120] * 6, 120)
    frag = np.zeros((6, 40), dtype=np.int64)
    for r in range(6):
        frag[r, :40 - 3 * r] = parent[r, 11 * r + 5:11 * r + 45 - 3 * r]
    mut = frag.copy()
    mut[:, 1] = mut[:, 1] % 20 + 1                                # another symbol in second place
    for gap, gap_open in ((30, 0), (4, 40)):
        semi, loc = semiglobal_alignment(S, gap, gap_open), local_alignment(S, gap, gap_open)
        P, Fr, Mu = torch.from_numpy(parent), torch.from_numpy(frag), torch.from_numpy(mut)
        own = np.array([S[f[f > 0], f[f > 0]].sum() for f in frag])
        assert np.array_equal(np.diag(semi(P, Fr).numpy()), own) and np.array_equal(np.diag(semi(Fr, Fr).numpy()), own)
        assert np.array_equal(np.diag(loc(P, Fr).numpy()), own)
        s_mut, l_mut = np.diag(semi(P, Mu).numpy()), np.diag(loc(P, Mu).numpy())
        assert (s_mut < own).all() and (l_mut > s_mut).all()
        assert np.array_equal(l_mut, own - S[frag[:, 0], frag[:, 0]] - S[frag[:, 1], frag[:, 1]])
        assert np.array_equal(s_mut, own - 20 - S[frag[:, 1], frag[:, 1]])
        assert np.array_equal(s_mut, np.diag(definition(S, gap, gap_open, parent, mut)))


def test_a_suffix_prefix_overlap_scores_the_overlap():
    """x ends with the ten symbols y begins with; everything else of the two comes from disjoint alphabets, and no two
    different symbols score above 0, so nothing but the overlap can be aligned at a profit."""
    rng = np.random.default_rng(5)
    S = score_table(rng, 21, -6, -1, diag=np.arange(2, 9))
    ov = rng.integers(15, 21, (4, 10))
    X, Y = np.zeros((4, 60), dtype=np.int64), np.zeros((4, 70), dtype=np.int64)
    for r in range(4):
        lx, ly = 30 + 7 * r, 25 + 11 * r
        X[r, :lx - 10], X[r, lx - 10:lx] = rng.integers(1, 8, lx - 10), ov[r]
        Y[r, :10], Y[r, 10:ly] = ov[r], rng.integers(8, 15, ly - 10)
    for gap, gap_open in ((1, 0), (3, 4)):
        op = semiglobal_alignment(S, gap, gap_open)
        s = op(torch.from_numpy(X), torch.from_numpy(Y)).numpy()
        assert np.array_equal(np.diag(s), [S[o, o].sum() for o in ov])
        assert np.array_equal(s, definition(S, gap, gap_open, X, Y)) and np.array_equal(s.T, op(torch.from_numpy(Y), torch.from_numpy(X)).numpy())
        assert (np.diag(local_alignment(S, gap, gap_open)(torch.from_numpy(X), torch.from_numpy(Y)).numpy()) >= np.diag(s)).all()


# ---------------------------------------------------------------- host logic through the stand-in
N, L = 120, 24


@pytest.fixture()
def pg(tmp_path, monkeypatch):
    fake_semiglobal_native.install(monkeypatch)
    from prograph_amd import Prograph
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=16, seed=5, members=12)
    tok = tok.copy()
    tok[7] = tok[8]
    assert lengths(tok).max() == L
    f = tmp_path / "semiglobal.csv"
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
    op = semiglobal_alignment(S, 3, gap_open=2)
    D = definition(S, 3, 2, tok, tok)
    assert not np.array_equal(D, fake_semiglobal_native.fake_long_native.fake_local_native.recurrence(S, 3, 2, tok, tok))
    G = P.build_graph(k=5, distance=op, output="csr")
    assert calls == [("operand", N, L, 21), ("score", 21), ("semiglobal_dense", N, 2, 3, 2), ("f16_knn", 5, 1, True)]
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
        assert calls[:2] == [("operand", N, L, 21), ("semiglobal_dense", N, 2, 3, 2)]
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
    assert calls[:2] == [("operand", 70, L, 21), ("semiglobal_dense", 70, 2, 3, 2)]
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
    assert calls == [("operand", N, L, 21), ("operand", 5, L + 9, 21), ("semiglobal_dense", 5, 2, 3, 2), ("f16_knn", 6, 0, True)]
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
    with pytest.raises(ValueError, match="semiglobal_alignment"):
        P.search(np.array([[1, 21]]), k=1, distance=op)           # a token outside the table: no generic loop
    P.build_graph(k=4, distance=op, store="Overlap", output="csr")
    assert "Overlap" in P.csr_graphs and np.array_equal(P.degree("Overlap"), knn_of(D, 4, 1)[1].sum(1).astype(np.float32))
    assert not [c for c in calls if "local" in c[0]]              # never the local kernels


def test_routes_at_and_beyond_the_bounds(pg, monkeypatch):
    from prograph_amd import _native
    P, tok = pg
    calls = fake_aln_native.calls
    rng = np.random.default_rng(4)
    rows = np.arange(N - 12, N)
    wide = rows_of(rng, 21, rng.integers(100, 129, 12), 128)
    over = rows_of(rng, 21, rng.integers(100, 130, 12), 129)
    over[0, 128] = 5                                              # 129 positions in use
    P.graph["W128"] = list(wide[:1]) * (N - 12) + list(wide)
    P.graph["W129"] = list(over[:1]) * (N - 12) + list(over)

    def table(top):
        S = score_table(rng, 21, -5, 2, diag=[3, 4])
        S[3, 3] = top
        return S
    # 128 * 16 = 2048: the fp16 route; 128 * 17: the torch selection; 129 positions: the long kernel and the int32 selection
    for rep, mat, top, route in (("W128", wide, 16, "semiglobal_dense"), ("W128", wide, 17, None),
                                 ("W129", over, 4, "semiglobal_long_dense")):
        S = table(top)
        op = semiglobal_alignment(S, 2, 1)
        del calls[:]
        gi, gw = _arrays(P.build_graph(k=3, distance=op, representation=rep, idxs=rows))
        assert [c[0] for c in calls if "dense" in c[0]] == ([route] if route else []), (rep, top, calls)
        if route == "semiglobal_dense":
            assert calls[-1] == ("f16_knn", 3, 1, True) and calls[-2][2] == 2
        elif route:
            assert calls[-1] == ("i32_knn", 3, 1, True) and calls[-2][2] == 4 and calls[0][0] == "long_operand"
        else:
            assert not calls                                      # the operator's torch blocks, no native call
        D = definition(S, 2, 1, mat, mat)
        wi, wd = knn_of(D, 3, 1)
        assert np.array_equal(gi, wi) and np.array_equal(gw, wd), (rep, top)
        del calls[:]
        _same_csr(P.build_graph(eps=6, distance=op, representation=rep, idxs=rows), *csr_of(D, operator.le, 6, diagonal=False))
        if route == "semiglobal_long_dense":
            assert calls[-1] == ("i32_eps", _native.CMP_GE, 6, False)
    # the long route switched off, and a table outside the 16-bit bound: the torch selection, the same answers
    S = table(4)
    op = semiglobal_alignment(S, 2, 1)
    D = definition(S, 2, 1, over, over)
    monkeypatch.setattr(_native, "aln_long_ready", lambda: False)
    del calls[:]
    gi, gw = _arrays(P.build_graph(k=3, distance=op, representation="W129", idxs=rows))
    assert not calls and np.array_equal(gi, knn_of(D, 3, 1)[0]) and np.array_equal(gw, knn_of(D, 3, 1)[1])
    monkeypatch.setattr(_native, "aln_long_ready", lambda: True)
    monkeypatch.setattr(_native, "aln_semiglobal_long_fits", lambda *a: False)
    gi, gw = _arrays(P.build_graph(k=3, distance=op, representation="W129", idxs=rows))
    assert not calls and np.array_equal(gi, knn_of(D, 3, 1)[0]) and np.array_equal(gw, knn_of(D, 3, 1)[1])
    # a comp outside the five orderings: the torch selection, the same edge set
    got = P.build_graph(eps=5, distance=op, comp=lambda t, s: t <= s, idxs=np.arange(30))
    assert not calls
    _same_csr(got, *csr_of(definition(op.table, 2, 1, tok[:30], tok[:30]), operator.le, 5, diagonal=False))


def test_the_bound_of_the_long_route():
    """2 * min(widths) * max(S) + 255 <= 65 535, i.e. min(widths) * max(S) <= 32 640; at most 2048 positions a side."""
    from prograph_amd import _native
    fits = _native.aln_semiglobal_long_fits
    assert fits(2048, 2048, 11)                                   # BLOSUM62's largest entry at full width
    assert fits(2040, 2040, 16) and 2 * 2040 * 16 + 255 == 65535 and not fits(2041, 2041, 16)
    assert fits(2048, 2048, 15) and not fits(2048, 2048, 16)
    assert fits(2048, 257, 127) and 2 * 257 * 127 + 255 == 65533 and not fits(2048, 258, 127) and not fits(258, 2048, 127)
    assert fits(257, 2048, 127) and not fits(2049, 1, 1) and not fits(1, 2049, 1)
    op = semiglobal_alignment(np.where(np.eye(4, dtype=bool), 11, -4), 1)
    assert op._long_fits(2048, 2048) and not semiglobal_alignment(np.where(np.eye(4, dtype=bool), 16, -4), 1)._long_fits(2048, 2048)


# ---------------------------------------------------------------- the C entries' argument checks
def test_argument_checks_of_the_c_entries_without_a_gpu():
    """Both entries return the PG_E_* of their local counterparts before any launch."""
    from prograph_amd import _native
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                      # never dereferenced on the host
    ok = dict(x=p, n=4, xnpad=256, xl=16, y=p, m=3, ynpad=256, yl=16, score=p, gap=2, gap_open=5, out=p, ldo=4, ob=8, stream=None,
              ws=p, wsb=1 << 30)

    def short(**kw):
        a = dict(ok, **kw)
        return lib.pg_alignment_semiglobal_dense(a["x"], a["n"], a["xnpad"], a["xl"], a["y"], a["m"], a["ynpad"], a["yl"], a["score"],
                                                 a["gap"], a["gap_open"], a["out"], a["ldo"], a["ob"], a["stream"])

    def long(**kw):
        a = dict(ok, **kw)
        return lib.pg_alignment_semiglobal_long_dense(a["x"], a["n"], a["xnpad"], a["xl"], a["y"], a["m"], a["ynpad"], a["yl"],
                                                      a["score"], a["gap"], a["gap_open"], a["out"], a["ldo"], a["ob"], a["ws"],
                                                      a["wsb"], a["stream"])

    BADARG, TOOLONG = -1, -2
    common = (dict(x=None), dict(y=None), dict(score=None), dict(out=None), dict(n=0), dict(m=0), dict(xl=0), dict(yl=0),
              dict(ldo=3), dict(gap=0), dict(gap=256), dict(gap_open=-1), dict(gap_open=256), dict(xnpad=255), dict(xnpad=3),
              dict(ynpad=2))
    for kw in common + (dict(ob=4),):
        assert short(**kw) == BADARG, kw
        assert b"pg_alignment_semiglobal_dense" in lib.pg_last_error()
    for kw in (dict(xl=129), dict(yl=129)):
        assert short(**kw) == TOOLONG, kw
        assert b"at most 128 positions" in lib.pg_last_error()
    for kw in common + (dict(ob=2), dict(ws=None), dict(wsb=256 * 16 * 4 - 1), dict(xl=300, wsb=256 * 300 * 4 - 1)):
        assert long(**kw) == BADARG, kw
        assert b"pg_alignment_semiglobal_long_dense" in lib.pg_last_error()
    for kw in (dict(xl=2049), dict(yl=2049)):
        assert long(**kw) == TOOLONG, kw
        assert b"at most 2048 positions" in lib.pg_last_error()
    assert lib.pg_version() == 3
    assert "pg_alignment_semiglobal_dense" in _native.SYMBOLS and "pg_alignment_semiglobal_long_dense" in _native.SYMBOLS
    with pytest.raises(ValueError):
        _native.alignment_semiglobal_dense(None, None, None, 1, 1, out_bytes=4)
    with pytest.raises(ValueError):
        _native.alignment_semiglobal_long_dense(None, None, None, 1, 1, out_bytes=2)
