"""
Affine gap penalties of the alignment distance without a GPU.

Two statements of the definition live here and are held against each other: `definition`, Gotoh's three tables H, E, F as
plain numpy loops over positions, and `brute_force`, which walks every alignment path of two short sequences and charges
`gap_open` whenever a gap column does not follow a gap column of the same kind.  Everything else - the operator's torch
expression on CPU tensors, the stand-in of tests/fake_affine_native.py behind the graph / search routes, and on the GPU
the kernel (tests/test_alignment_affine_gpu.py) - is compared with `definition`.
"""
import ctypes
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import fake_affine_native
import fake_aln_native
from prograph_amd import synth
from prograph_amd.distance import alignment, substitution

INF = 1 << 40


def lengths(T):
    T = np.asarray(T)
    return np.where(T != 0, np.arange(1, T.shape[1] + 1), 0).max(axis=1, initial=0)


# ---------------------------------------------------------------- (a) the three-table recurrence
def definition(C, gap, gap_open, X, Y):
    """(M, N) int64: H[len x][len y] of the affine recurrence, i over the positions of x and j over those of y, the three
    tables H, E, F held for rows i - 1 and i, all pairs of one y length at once."""
    C, X, Y = np.asarray(C, dtype=np.int64), np.atleast_2d(np.asarray(X, dtype=np.intp)), np.atleast_2d(np.asarray(Y, dtype=np.intp))
    lx, ly = lengths(X), lengths(Y)
    LX, N, e, o = int(lx.max(initial=0)), len(X), int(gap), int(gap_open)
    out = np.empty((len(Y), N), dtype=np.int64)
    for l in np.unique(ly):
        rows = np.nonzero(ly == l)[0]
        shape = (l + 1, len(rows), N)
        H, E = np.zeros(shape, dtype=np.int64), np.full(shape, INF, dtype=np.int64)       # row 0: E[0][j] = inf
        for j in range(1, l + 1):
            H[j] = o + j * e
        res = np.where(lx == 0, H[l], 0)                          # H[len x][l], taken at row i = len x
        Hp, Ep, F = np.empty_like(H), np.full(shape, INF, dtype=np.int64), np.full(shape, INF, dtype=np.int64)
        for i in range(1, LX + 1):
            H, E, Hp, Ep = Hp, Ep, H, E                           # rows i - 1 become the old ones, their buffers are reused
            H[0] = o + i * e                                      # E[i][0] = F[i][0] = inf stay as set above
            cx = C[X[:, i - 1]]                                   # (N, A): the costs of x_i against every symbol
            for j in range(1, l + 1):
                E[j] = np.minimum(Ep[j] + e, Hp[j] + o + e)
                F[j] = np.minimum(F[j - 1] + e, H[j - 1] + o + e)
                H[j] = np.minimum(Hp[j - 1] + cx[:, Y[rows, j - 1]].T, np.minimum(E[j], F[j]))
            res = np.where(lx == i, H[l], res)
        out[rows] = res
    return out


# ---------------------------------------------------------------- (b) every alignment path
def brute_force(C, gap, gap_open, x, y):
    """The cheapest of all alignments of the token lists x and y, each path walked to its end: a column pairs x_i with y_j,
    or leaves x_i unaligned (kind 1), or leaves y_j unaligned (kind 2); an unaligned column costs `gap`, plus `gap_open`
    unless the column before it is of the same kind."""
    def walk(i, j, last):
        if i == len(x) and j == len(y):
            return 0
        best = INF
        if i < len(x) and j < len(y):
            best = min(best, int(C[x[i]][y[j]]) + walk(i + 1, j + 1, 0))
        if i < len(x):
            best = min(best, gap + (0 if last == 1 else gap_open) + walk(i + 1, j, 1))
        if j < len(y):
            best = min(best, gap + (0 if last == 2 else gap_open) + walk(i, j + 1, 2))
        return best
    return walk(0, 0, 0)


def knn_of(D, k, first):
    order = np.argsort(D, axis=1, kind="stable")[:, first:first + k]
    return order, np.take_along_axis(D, order, 1)


def csr_of(D, comp, eps, keep_zero=False):
    keep = comp(D, eps) & ((D >= 0) if keep_zero else (D > 0))
    r, c = np.nonzero(keep)
    return np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64), c, D[r, c]


def table(rng, a, values):
    C = np.triu(rng.choice(np.asarray(values), size=(a, a)), 1)
    return C + C.T


def rows_of(rng, a, lens, width):
    T = np.zeros((len(lens), width), dtype=np.int64)
    for r, l in enumerate(lens):
        T[r, :l] = rng.integers(1, a, l)
    return T


@pytest.mark.parametrize("values,gap,gap_open", [((1, 2, 3), 1, 0), ((1, 2, 3), 2, 5), ((2, 5, 9), 1, 11), ((1, 4), 3, 1),
                                                ((3, 7, 20), 4, 9), ((1, 2), 255, 255)])
def test_the_recurrence_is_the_cheapest_alignment_path(values, gap, gap_open):
    """(a) against (b) on sequences of 0..5 symbols out of four (symbol 0 only inside a sequence: a trailing zero is
    padding): four sequences of every length, all 24 x 24 pairs, at most 1683 paths each.  `gap_open` above every
    substitution cost, below it, and 0."""
    rng = np.random.default_rng(gap * 1000 + gap_open)
    C = table(rng, 4, values)
    seqs = np.zeros((24, 5), dtype=np.int64)
    for r in range(24):
        l = r // 4
        seqs[r, :l] = rng.integers(0, 4, l)
        if l:
            seqs[r, l - 1] = rng.integers(1, 4)                   # the last symbol is not the padding value
    assert sorted(lengths(seqs)) == sorted(list(range(6)) * 4)
    D = definition(C, gap, gap_open, seqs, seqs)
    lens = lengths(seqs)
    for r in range(24):
        for c in range(24):
            assert D[r, c] == brute_force(C, gap, gap_open, list(seqs[c, :lens[c]]), list(seqs[r, :lens[r]])), (r, c)
    assert np.array_equal(D, D.T) and (np.diag(D) == 0).all()


def test_an_x_run_followed_by_a_y_run_is_two_runs():
    """One symbol against one symbol whose substitution costs more than two opened gaps: the cheapest alignment leaves
    both unaligned, and that is two runs, 2 (gap_open + gap) - not gap_open + 2 gap."""
    C = np.array([[0, 9, 9], [9, 0, 200], [9, 200, 0]])
    for f in (definition, lambda *a: brute_force(a[0], a[1], a[2], list(a[3][0]), list(a[4][0]))):
        assert int(np.asarray(f(C, 3, 10, np.array([[1]]), np.array([[2]]))).reshape(-1)[0]) == 26
    assert int(alignment(C, 3, 10)(torch.tensor([[1]]), torch.tensor([[2]]))) == 26
    assert int(fake_affine_native.recurrence(C, 3, 10, np.array([[1]]), np.array([[2]]))[0, 0]) == 26


# ---------------------------------------------------------------- the constructor
def test_constructor_rules_for_gap_open():
    good = table(np.random.default_rng(0), 5, np.arange(1, 200))
    dist = alignment(good, 7, gap_open=11)
    assert dist.gap == 7 and dist.gap_open == 11 and dist.max_cost == max(good.max(), 7)
    assert alignment(good, 7, 11).gap_open == 11 and alignment(good, 7, gap_open=3.0).gap_open == 3
    assert alignment(good, 7, gap_open=np.int64(255)).gap_open == 255 and alignment(good, 7, gap_open=np.uint8(0)).gap_open == 0
    assert alignment(substitution(good), 2, gap_open=9).gap_open == 9
    for o in (-1, 256, 2.5, True, False, np.bool_(True), float("nan"), float("inf"), None, "3"):
        with pytest.raises(ValueError):
            alignment(good, 5, gap_open=o)
            pytest.fail(repr(o))
    with pytest.raises(AttributeError):
        dist.gap_open = 3                                         # read-only
    plain = alignment(good, 7)
    assert plain.gap_open == 0 and alignment(good, 7, gap_open=0).gap_open == 0
    assert repr(plain) == repr(alignment(good, 7, gap_open=0)) == f"alignment(<5 x 5 table, costs up to {good.max()}>, gap=7)"
    assert "gap_open" not in repr(plain)
    assert repr(dist) == f"alignment(<5 x 5 table, costs up to {good.max()}>, gap=7, gap_open=11)"
    assert plain.max_cost == dist.max_cost == alignment(good, 7, gap_open=255).max_cost     # max_cost does not count the open


# ---------------------------------------------------------------- the operator on the host
@pytest.mark.parametrize("a,gap,gap_open", [(21, 1, 11), (21, 7, 3), (32, 255, 255), (32, 1, 255), (32, 40, 0)])
def test_operator_against_the_definition_on_cpu_tensors(a, gap, gap_open):
    rng = np.random.default_rng(100 * a + gap + gap_open)
    C = table(rng, a, np.arange(256))
    dist = alignment(C, gap, gap_open=gap_open)
    X = rows_of(rng, a, [0, 1, 15, 16, 17, 33] + list(rng.integers(0, 41, 34)), 40)       # tokens up to a - 1 = 31
    Y = rows_of(rng, a, [0, 1, 15, 16, 17, 33, 5], 33)            # unequal widths
    X[9] = 0                                                      # empty rows on both sides
    X[::4, 2], Y[3, 7], Y[4, 0] = 0, 0, 0                         # interior zeros: symbol 0 of the table
    X[5, :] = 0
    X[5, 9] = a - 1                                               # leading zeros count: length 10
    assert X.max() == a - 1 and lengths(X)[0] == 0 and lengths(X)[5] == 10
    want = definition(C, gap, gap_open, X, Y)
    d = dist(torch.from_numpy(X), torch.from_numpy(Y))
    assert d.shape == (7, 40) and d.dtype == torch.int64 and d.device.type == "cpu"
    assert np.array_equal(d.numpy(), want)
    lx = lengths(X)
    assert (want[0] == np.where(lx > 0, gap_open + lx * gap, 0)).all() and want[0, 5] == gap_open + 10 * gap and want[0, 9] == 0
    assert np.array_equal(dist(torch.from_numpy(Y), torch.from_numpy(X)).numpy(), want.T)      # symmetric
    one = dist(torch.from_numpy(X), torch.from_numpy(Y[2]))       # a 1-D operand
    assert one.shape == (1, 40) and np.array_equal(one.numpy(), want[2:3])
    padded = dist(torch.from_numpy(np.pad(X, ((0, 0), (0, 9)))), torch.from_numpy(Y))       # padding changes nothing
    assert np.array_equal(padded.numpy(), want)
    for dt in (torch.uint8, torch.int32, torch.float64):
        assert np.array_equal(dist(torch.from_numpy(X).to(dt), torch.from_numpy(Y).to(dt)).numpy(), want)
    s = dist(torch.from_numpy(X), torch.from_numpy(Y), similarity=True)
    assert s.dtype == torch.float32 and torch.equal(s, 1 / (1 + d))
    import sys
    mod = sys.modules["prograph_amd.distance.alignment"]         # (the package attribute of that name is the class)
    old = mod._DP_ELEMS
    try:
        mod._DP_ELEMS = 41 * 9 * 2                                 # blocks of the table do not change the result
        assert np.array_equal(dist(torch.from_numpy(X), torch.from_numpy(Y)).numpy(), want)
    finally:
        mod._DP_ELEMS = old
    assert np.array_equal(fake_affine_native.recurrence(C, gap, gap_open, X, Y), want)      # the stand-in's own loop
    with pytest.raises(ValueError):
        dist(torch.tensor([[1, a]]), torch.tensor([[1, 2]]))      # a token outside the table


def test_gap_open_zero_is_the_linear_distance():
    rng = np.random.default_rng(5)
    C = table(rng, 21, np.arange(256))
    X, Y = rows_of(rng, 21, rng.integers(0, 34, 50), 33), rows_of(rng, 21, rng.integers(0, 20, 11), 19)
    X[::3, 1] = 0
    for gap in (1, 9, 255):
        lin = alignment(C, gap)(torch.from_numpy(X), torch.from_numpy(Y))
        assert torch.equal(alignment(C, gap, gap_open=0)(torch.from_numpy(X), torch.from_numpy(Y)), lin)
        assert np.array_equal(definition(C, gap, 0, X, Y), lin.numpy())
        # forcing the affine expression at 0 gives the same numbers: the two forms meet there
        forced = alignment(C, gap)
        assert np.array_equal(forced._dp_block_affine(torch.from_numpy(C).to(torch.int32), torch.from_numpy(X), torch.from_numpy(lengths(X)),
                                                      torch.from_numpy(Y), torch.from_numpy(lengths(Y))).numpy(), lin.numpy())


def test_with_prohibitive_gaps_it_is_substitution():
    rng = np.random.default_rng(8)
    C = table(rng, 21, np.arange(1, 49))
    X, Y = torch.from_numpy(rng.integers(1, 21, (60, 8))), torch.from_numpy(rng.integers(1, 21, (9, 8)))
    assert 2 * (190 + 3) > 8 * C.max() and not 2 * 3 > 8 * C.max()
    assert torch.equal(alignment(C, 3, gap_open=190)(X, Y), substitution(C)(X, Y))     # the open alone forbids the gaps
    assert not torch.equal(alignment(C, 3)(X, Y), substitution(C)(X, Y))               # without it, gaps pay


def test_a_block_insertion_costs_one_open():
    rng = np.random.default_rng(12)
    C = table(rng, 21, np.arange(30, 60))                         # every substitution costs at least 30
    base = rng.integers(1, 21, 40)
    for g, gap, gap_open in ((1, 2, 11), (5, 2, 11), (9, 1, 20), (5, 3, 0)):
        assert gap_open + g * gap < 30                            # cheaper than any substitution
        longer = np.concatenate([base[:17], rng.integers(1, 21, g), base[17:]])
        X, Y = np.zeros((1, 49), dtype=np.int64), np.zeros((1, 49), dtype=np.int64)
        X[0, :40], Y[0, :40 + g] = base, longer
        for A, B in ((X, Y), (Y, X)):
            assert int(alignment(C, gap, gap_open=gap_open)(torch.from_numpy(A), torch.from_numpy(B))) == gap_open + g * gap
        assert int(definition(C, gap, gap_open, X, Y)[0, 0]) == gap_open + g * gap
    # five scattered single insertions are five events
    scattered = np.insert(base, [3, 11, 19, 27, 35], rng.integers(1, 21, 5))
    X, Y = np.zeros((1, 45), dtype=np.int64), np.zeros((1, 45), dtype=np.int64)
    X[0, :40], Y[0, :45] = base, scattered
    assert int(alignment(C, 2, gap_open=3)(torch.from_numpy(X), torch.from_numpy(Y))) == 5 * (3 + 2)


# ---------------------------------------------------------------- host logic through the stand-in
N, L = 120, 24


@pytest.fixture()
def pg(tmp_path, monkeypatch):
    fake_affine_native.install(monkeypatch)
    from prograph_amd import Prograph
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=16, seed=5, members=12)
    tok = tok.copy()
    tok[7] = tok[8]
    assert lengths(tok).max() == L
    f = tmp_path / "aln.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    del fake_aln_native.calls[:]
    return P, tok


def _arrays(got):
    return np.array([i for i, _ in got]), np.array([w for _, w in got])


def test_graph_and_search_routes(pg):
    from prograph_amd import _native
    P, tok = pg
    calls = fake_aln_native.calls
    rng = np.random.default_rng(3)
    C = table(rng, 21, 2 * np.arange(1, 7))
    dist = alignment(C, 5, gap_open=9)
    D = definition(C, 5, 9, tok, tok)
    assert (D != definition(C, 5, 0, tok, tok)).any()
    G = P.build_graph(k=5, distance=dist, output="csr")
    assert calls == [("operand", N, L, 21), ("affine_dense", N, 2, 5, 9), ("f16_knn", 5, 1, False)]
    wi, wd = knn_of(D, 5, 1)
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.first == 1
    assert np.array_equal(G.idx.numpy(), wi) and np.array_equal(G.dist.numpy(), wd)
    gi, gw = _arrays(P.build_graph(k=5, distance=dist, similarity=True))
    assert gw.dtype == np.float32 and np.array_equal(gi, wi) and np.array_equal(gw, (1 / (1 + torch.from_numpy(wd))).numpy())
    for name, comp, eps, thr in (("le", operator.le, 30, 30.0), ("lt", operator.lt, 30.5, 31.0), ("eq", operator.eq, 19, 19.0),
                                 ("ge", operator.ge, 90.5, 91.0), ("eq", operator.eq, 10.5, -1.0)):
        del calls[:]
        G = P.build_graph(eps=eps, distance=dist, comp=comp, output="csr")
        assert calls[:2] == [("operand", N, L, 21), ("affine_dense", N, 2, 5, 9)]
        assert calls[-1] == ("f16_eps", getattr(_native, "CMP_" + name.upper()), thr, False, False), calls
        ip, ix, w = csr_of(D, comp, eps)
        assert G.weights.dtype == torch.int16 and np.array_equal(G.indptr.numpy(), ip)
        assert np.array_equal(G.indices.numpy(), ix) and np.array_equal(G.weights.numpy(), w)
    sub = np.arange(50, 120)
    del calls[:]
    got = P.build_graph(eps=30, distance=dist, idxs=sub)
    assert calls[:2] == [("operand", 70, L, 21), ("affine_dense", 70, 2, 5, 9)]
    ip, ix, w = csr_of(D[np.ix_(sub, sub)], operator.le, 30)
    assert ip[-1] > 0
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    # search: rank 0 and d = 0 kept, queries wider than the dataset
    Q = np.zeros((5, L + 9), dtype=np.int64)
    Q[:, :L] = tok[[3, 50, 99, 100, 8]]
    Q[3, L:L + 6] = rng.integers(1, 21, 6)                        # longer than the dataset's rows
    Q[2, 11:] = 0                                                 # shorter
    DQ = definition(C, 5, 9, tok, Q)
    del calls[:]
    gi, gw = _arrays(P.search(Q, k=6, distance=dist))
    assert calls == [("operand", N, L, 21), ("operand", 5, L + 9, 21), ("affine_dense", 5, 2, 5, 9), ("f16_knn", 6, 0, False)]
    wi, wd = knn_of(DQ, 6, 0)
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd) and wd[4, 0] == 0 and set(wi[4, :2]) == {7, 8}
    del calls[:]
    got = P.search(Q, eps=30, distance=dist)
    assert calls[-1] == ("f16_eps", _native.CMP_LE, 30.0, False, True)
    ip, ix, w = csr_of(DQ, operator.le, 30, keep_zero=True)
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    hit, dmin = P.nearest_neighbour(synth.tokens_to_strings(tok[50:51])[0], distance=dist)
    assert list(hit.index) == [int(wi[1, 0])] and dmin == wd[1, 0]
    seq = P("Sequence")[8]
    assert list(P.neighbourhood(seq, 30, distance=dist).index) == list(np.nonzero(D[8] <= 30)[0])
    got = P.calc_neighbours(seq, eps=20, distance=dist, comp=operator.le)
    assert np.array_equal(np.sort(np.asarray(got)), np.nonzero(D[8] <= 20)[0])


def test_gap_open_zero_records_the_calls_of_the_linear_route(pg):
    P, tok = pg
    calls = fake_aln_native.calls
    C = table(np.random.default_rng(3), 21, 2 * np.arange(1, 7))
    seen = []
    for dist in (alignment(C, 5), alignment(C, 5, gap_open=0)):
        del calls[:]
        P.build_graph(k=5, distance=dist, output="csr")
        P.build_graph(eps=20, distance=dist)
        P.search(tok[:7], k=4, distance=dist)
        P.search(tok[:7], eps=12, distance=dist)
        seen.append(list(calls))
    assert seen[0] == seen[1] and seen[0][:3] == [("operand", N, L, 21), ("dense", N, 2, 5), ("f16_knn", 5, 1, False)]
    assert not [c for c in seen[1] if c[0] == "affine_dense"]


def test_routes_at_and_beyond_the_bounds(pg):
    P, tok = pg
    calls = fake_aln_native.calls
    rng = np.random.default_rng(4)
    C = table(rng, 21, [1, 2, 3])
    rows = np.arange(N - 12, N)
    narrow, wide = rows_of(rng, 21, rng.integers(1, 17, 12), 16), rows_of(rng, 21, rng.integers(100, 129, 12), 128)
    over = rows_of(rng, 21, rng.integers(100, 130, 12), 129)
    P.graph["W16"] = list(narrow[:1]) * (N - 12) + list(narrow)
    P.graph["W128"] = list(wide[:1]) * (N - 12) + list(wide)
    P.graph["W129"] = list(over[:1]) * (N - 12) + list(over)
    # width * max_cost + gap_open: 16 * 127 + 16 = 2048 native, + 17 = 2049 generic; 128 * 15 + 128 = 2048, + 129 = 2049;
    # 16 * 128 + 0 = 2048 stays native on the linear kernel, + 1 is generic; 129 positions are generic at any price
    for rep, mat, gap, gap_open, native in (("W16", narrow, 127, 16, "affine_dense"), ("W16", narrow, 127, 17, None),
                                            ("W128", wide, 15, 128, "affine_dense"), ("W128", wide, 15, 129, None),
                                            ("W16", narrow, 128, 0, "dense"), ("W16", narrow, 128, 1, None),
                                            ("W129", over, 1, 1, None)):
        dist = alignment(C, gap, gap_open=gap_open)
        assert mat.shape[1] * dist.max_cost + gap_open == (2048 if native else 2049) or mat.shape[1] == 129
        del calls[:]
        gi, gw = _arrays(P.build_graph(k=3, distance=dist, representation=rep, idxs=rows))
        assert [c[0] for c in calls if "dense" in c[0]] == ([native] if native else []), (rep, gap, gap_open)
        assert bool(calls) is bool(native)
        wi, wd = knn_of(definition(C, gap, gap_open, mat, mat), 3, 1)
        assert np.array_equal(gi, wi) and np.array_equal(gw, wd), (rep, gap, gap_open)
    # search: the wider of dataset and queries counts
    dist = alignment(C, 15, gap_open=128)
    del calls[:]
    gi, gw = _arrays(P.search(wide[:3], k=2, distance=dist))
    assert ("affine_dense", 3, 2, 15, 128) in calls
    wi, wd = knn_of(definition(C, 15, 128, tok, wide[:3]), 2, 0)
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd)
    del calls[:]
    gi, gw = _arrays(P.search(wide[:3], k=2, distance=alignment(C, 15, gap_open=129)))
    wi, wd = knn_of(definition(C, 15, 129, tok, wide[:3]), 2, 0)
    assert not calls and np.array_equal(gi, wi) and np.array_equal(gw, wd)
    del calls[:]
    got = P.build_graph(eps=12, distance=alignment(C, 4, gap_open=2), comp=lambda d, e: d <= e, idxs=np.arange(30))
    assert not calls                                              # a comp outside the five orderings: the generic loop
    ip, ix, w = csr_of(definition(C, 4, 2, tok[:30], tok[:30]), operator.le, 12)
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])


def test_block_rows(pg, monkeypatch):
    P, tok = pg
    calls = fake_aln_native.calls
    dist = alignment(table(np.random.default_rng(6), 21, 2 * np.arange(1, 7)), 5, gap_open=7)
    monkeypatch.setattr(type(P), "_BLOCK_ELEMS", N * 3)
    P.build_graph(k=4, distance=dist)
    assert [c[1] for c in calls if c[0] == "affine_dense"] == [64, 56]                 # never below 64 rows
    del calls[:]
    P.search(tok[:7], k=4, distance=dist)
    assert [c[1] for c in calls if c[0] == "affine_dense"] == [3, 3, 1]                # queries: down to one row
    monkeypatch.setattr(type(P), "_BLOCK_ELEMS", N * 100)
    del calls[:]
    P.build_graph(eps=12, distance=dist)
    assert [c[1] for c in calls if c[0] == "affine_dense"] == [100, 20]
    del calls[:]
    P.search(tok[:7], eps=12, distance=dist)
    assert [c[1] for c in calls if c[0] == "affine_dense"] == [7] and not [c for c in calls if c[0] == "dense"]


# ---------------------------------------------------------------- the C entry's argument checks
def test_argument_checks_of_the_c_entry_without_a_gpu():
    """`pg_alignment_affine_dense` returns the PG_E_* of `pg_alignment_dense` before any launch."""
    from prograph_amd import _native
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                      # never dereferenced on the host
    ok = dict(x=p, n=4, xnpad=256, xl=16, y=p, m=3, ynpad=256, yl=16, cost=p, gap=2, gap_open=5, out=p, ldo=4, ob=8, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.pg_alignment_affine_dense(a["x"], a["n"], a["xnpad"], a["xl"], a["y"], a["m"], a["ynpad"], a["yl"], a["cost"],
                                             a["gap"], a["gap_open"], a["out"], a["ldo"], a["ob"], a["stream"])

    BADARG, TOOLONG = -1, -2
    for kw in (dict(x=None), dict(y=None), dict(cost=None), dict(out=None), dict(n=0), dict(m=0), dict(xl=0), dict(yl=0),
               dict(ldo=3), dict(gap=0), dict(gap=256), dict(gap_open=-1), dict(gap_open=256), dict(xnpad=255), dict(xnpad=3),
               dict(ynpad=2), dict(ob=4)):
        assert call(**kw) == BADARG, kw
        assert b"pg_alignment_affine_dense" in lib.pg_last_error()
    for kw in (dict(xl=129), dict(yl=129)):
        assert call(**kw) == TOOLONG, kw
        assert b"at most 128 positions" in lib.pg_last_error()
    assert lib.pg_alignment_dense(p, 4, 256, 129, p, 3, 256, 16, p, 2, p, 4, 8, None) == TOOLONG      # as the linear entry
    assert lib.pg_version() == 3
    with pytest.raises(ValueError):
        _native.alignment_affine_dense(None, None, None, 1, 1, out_bytes=4)
