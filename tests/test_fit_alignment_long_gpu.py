"""
Fit alignment scores beyond 128 positions on the GPU: `pg_alignment_fit_long_dense` (prograph_amd/csrc/pg_aln_fit.hip) on
every entry against `definition` of tests/fit_testdata.py around every strip and slot boundary and at every strip count,
at 2048 x 2048 positions against the operator's torch expression on CPU tensors (itself held against `definition` in
tests/test_fit_alignment_cpu.py), the int32 routes of `build_graph` / `search` against the same calls with the long route
switched off, the long traceback against `canonical`, and both sides of the bound of the 16-bit cells.  Every comparison
is an every-entry equality.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from fit_testdata import canonical, definition, fragments, lengths, rows_of, score_table, seq
from prograph_amd import alignments, synth
from prograph_amd.distance import fit_alignment

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

GAPS = ((1, 11), (3, 0))


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def run(nat, S, gap, gap_open, X, Y, **kw):
    xo = nat.aln_long_operand(torch.from_numpy(np.ascontiguousarray(X).astype(np.uint8)), len(S))
    yo = nat.aln_long_operand(torch.from_numpy(np.ascontiguousarray(Y).astype(np.uint8)), len(S))
    assert xo.valid() and yo.valid() and nat.aln_fit_fits(X.shape[1], Y.shape[1], int(S.max()), gap, gap_open)
    return nat.alignment_fit_long_dense(xo, yo, nat.aln_local_score(S), gap, gap_open, **kw).cpu().numpy()


def table(rng, a=21):
    S = score_table(rng, a, -9, 6, diag=np.arange(2, 12))
    S[0, :] = S[:, 0] = 5                                         # padding would score if it were let in
    return S


def contain(rng, X, Y):
    """Make some columns hold a row, whole or all but a piece of it, in place; X rows keep or gain length."""
    lx, ly = lengths(X), lengths(Y)
    for c in range(min(len(X), 2 * len(Y))):
        r = c % len(Y)
        l = int(ly[r]) if c < len(Y) else int(ly[r]) * 2 // 3
        if l < 2 or l > X.shape[1]:
            continue
        at = int(rng.integers(0, X.shape[1] - l + 1))
        X[c, at:at + l] = Y[r, :l]
        if at + l > lx[c]:
            X[c, lx[c]:at] = rng.integers(1, 21, max(0, at - lx[c]))


# ---------------------------------------------------------------- 1. the dense kernel against the definition
@pytest.mark.parametrize("gap,gap_open", GAPS)
def test_lengths_around_the_strip_seams(nat, gap, gap_open):
    rng = np.random.default_rng(100 + gap)
    S = table(rng)
    lens = (129, 255, 256, 257, 300)
    Y = rows_of(rng, 21, lens, 300)
    X = rows_of(rng, 21, list(lens) * 3 + [0, 1, 128], 300)
    contain(rng, X, Y)
    want = definition(S, gap, gap_open, X, Y)
    assert want.max() > 300 and want.min() < -300
    got = run(nat, S, gap, gap_open, X, Y)
    assert got.dtype == np.int64 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    K = gap_open + gap * 300
    got = run(nat, S, gap, gap_open, X, Y, out_bytes=4, bias=K)   # int32 blocks with the selection's shift
    assert got.dtype == np.int32 and np.array_equal(got, want + K) and got.min() == 0
    assert np.array_equal(run(nat, S, gap, gap_open, X, Y, out_bytes=4, rows=(1, 4)), want[1:4])
    assert np.array_equal(run(nat, S, gap, gap_open, Y, X), definition(S, gap, gap_open, Y, X))
    assert np.array_equal(run(nat, S, gap, gap_open, X, Y[:2, :40]), definition(S, gap, gap_open, X, Y[:2, :40]))


@pytest.mark.parametrize("gap,gap_open", GAPS)
def test_every_strip_count_and_the_slot_boundary_at_1024(nat, gap, gap_open):
    """len y = 128 k for k = 1..16 (the end of a strip), one past several of them, 1024 / 1025 (eight strips fill the profile
    slots once, the ninth starts the second fill) and 2048, against short X rows so that the numpy loop stays small; and in
    the other order: len x at every strip count under one strip of Y."""
    rng = np.random.default_rng(200 + gap)
    S = table(rng)
    Y = rows_of(rng, 21, [128 * k for k in range(1, 17)] + [129, 1025, 1921, 2047, 1023], 2048)
    X = rows_of(rng, 21, [24, 17, 16, 1, 0, 24, 9], 24)
    X[0, :24], X[1, :17] = Y[3, 100:124], Y[15, 2031:2048]        # pieces of long rows: len y > len x by far
    want = definition(S, gap, gap_open, X, Y)
    assert want[15, 4] == -(gap_open + gap * 2048) and lengths(Y).max() == 2048
    got = run(nat, S, gap, gap_open, X, Y)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    back = definition(S, gap, gap_open, Y, X)                     # short rows, whole, inside long columns
    assert back[0, 3] == S[X[0], X[0]].sum() and back[1, 15] == S[X[1, :17], X[1, :17]].sum() and (back[4] == 0).all()
    got = run(nat, S, gap, gap_open, Y, X, out_bytes=4)
    assert np.array_equal(got, back), np.argwhere(got != back)[:5]


def test_a_lane_a_length_and_interior_zeros(nat):
    rng = np.random.default_rng(7)
    S = table(rng)
    X = rows_of(rng, 21, list(rng.permutation(np.arange(129, 401))[:64]) + list(range(400, 394, -1)), 400)      # a wave and a bit
    Y = rows_of(rng, 21, [400, 129, 257], 400)
    assert len(set(lengths(X[:64]))) == 64
    X[::3, 2], X[1::5, 0], X[::7, 128], Y[0, 127:130], Y[1, :16] = 0, 0, 0, 0, 0          # interior zeros: symbol 0
    contain(rng, X, Y)
    assert np.array_equal(run(nat, S, 2, 7, X, Y), definition(S, 2, 7, X, Y))


def test_padding_never_scores_across_strips(nat):
    """S[0][0] = 127 and S[a][0] = 9 at 256 positions, the widest the bound admits with a score of 127 in the table at gap
    1 / 0 (256 * 255 + 255 = 65 535): len y on both sides of two strip seams, both operand orders."""
    rng = np.random.default_rng(13)
    S = score_table(rng, 21, -6, 3, diag=np.arange(2, 9))
    S[0, :] = S[:, 0] = 9
    S[0, 0] = 127
    A = rows_of(rng, 21, [127, 128, 129, 144], 256)
    B = rows_of(rng, 21, [256, 255, 130, 1, 0, 128, 129, 200] + list(rng.integers(1, 257, 60)), 256)
    assert nat.aln_fit_fits(256, 256, 127, 1, 0) and not nat.aln_fit_fits(256, 256, 127, 1, 1)
    assert np.array_equal(run(nat, S, 1, 0, B, A), definition(S, 1, 0, B, A))
    assert np.array_equal(run(nat, S, 1, 0, A, B), definition(S, 1, 0, A, B))


# ---------------------------------------------------------------- 2. 2048 positions, and the bound
@pytest.mark.parametrize("top,gap,gap_open", [(11, 1, 11), (15, 3, 0)])
def test_2048_positions(nat, top, gap, gap_open):
    """3 x 5 at 2048 positions: len y = 2048, 1920 (the end of strip 15) and 1921 (one past it), max(S) = 11 (BLOSUM62's)
    at gap 1 / 11 and 15 at gap 3 / 0 (2048 * 33 + 255 = 67 839 is outside: 1978 positions are the widest there,
    1978 * 33 + 255 = 65 529): against the operator's torch expression on CPU tensors."""
    rng = np.random.default_rng(12 + top)
    S = np.full((21, 21), -4)
    S[np.arange(21), np.arange(21)] = rng.integers(4, top + 1, 21)
    S[1, 1] = top
    width = 2048 if top == 11 else 1978
    assert nat.aln_fit_fits(width, width, top, gap, gap_open) and (width == 2048 or not nat.aln_fit_fits(width + 1, width + 1, top, gap, gap_open))
    X = rows_of(rng, 21, (width, width - 1, width, 1025, 40), width)
    Y = rows_of(rng, 21, (width, 1920, 1921), width)
    X[0, :1920] = Y[1, :1920]                                     # holds row 1
    X[2], Y[0] = 1, 1                                             # ones against ones: width * top, the largest cell
    X[3, 20:1020] = Y[2, 900:1900]                                # a piece of row 2
    X[4, :40] = Y[1, 1000:1040]
    op = fit_alignment(S, gap, gap_open)
    want = op(torch.from_numpy(X), torch.from_numpy(Y)).numpy()          # the torch expression on CPU tensors
    got = run(nat, S, gap, gap_open, X, Y)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert got[0, 2] == width * top and got[1, 0] == S[Y[1, :1920], Y[1, :1920]].sum() and got[0, 4] < -1000
    dev = op(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())     # the operator takes the long kernel
    assert dev.dtype == torch.int64 and np.array_equal(dev.cpu().numpy(), want)


def test_both_sides_of_the_bound(nat, monkeypatch):
    """gap 2 / 0 under max(S) = 15 at width 2040: 2040 * 32 + 255 = 65 535 just fits, and the largest cell is reached (2040
    ones against 2040 ones); gap_open = 1 does not fit: the operator falls back to its torch expression and stays exact."""
    S = np.full((4, 4), -128)
    S[np.arange(4), np.arange(4)] = (3, 15, 7, 9)
    rng = np.random.default_rng(5)
    X = rows_of(rng, 4, (2040, 2040, 300, 0), 2040)
    Y = rows_of(rng, 4, (2040, 2040, 129), 2040)
    X[0], Y[0] = 1, 1
    X[2, 100:229] = Y[2, :129]
    assert nat.aln_fit_fits(2040, 2040, 15, 2, 0) and not nat.aln_fit_fits(2040, 2040, 15, 2, 1)
    want = fit_alignment(S, 2, 0)(torch.from_numpy(X), torch.from_numpy(Y)).numpy()
    assert want[0, 0] == 2040 * 15 and want[0, 3] == -2 * 2040 and want[2, 2] == S[Y[2, :129], Y[2, :129]].sum()
    assert np.array_equal(run(nat, S, 2, 0, X, Y), want)
    calls = []
    real = nat.alignment_fit_long_dense
    monkeypatch.setattr(nat, "alignment_fit_long_dense", lambda *a, **k: calls.append(1) or real(*a, **k))
    op = fit_alignment(S, 2, 1)
    got = op(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
    assert got.is_cuda and not calls and np.array_equal(got.cpu().numpy(), op(torch.from_numpy(X), torch.from_numpy(Y)).numpy())
    assert torch.equal(fit_alignment(S, 2, 0)(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()).cpu(), torch.from_numpy(want)) and calls


# ---------------------------------------------------------------- 3. the routes
N, W = 60, 400


@pytest.fixture(scope="module")
def pg(tmp_path_factory):
    from prograph_amd import Prograph
    rng = np.random.default_rng(21)
    tok = fragments(rng, 21, N, W, least=130)
    tok[0, :400] = rng.integers(1, 21, 400)
    tok[7] = tok[8]                                               # duplicates
    f = tmp_path_factory.mktemp("fitlong") / "long.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": rng.uniform(0, 1, N)}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P, tok


def _same(a, b):
    assert len(a) == len(b)
    for r in range(len(a)):
        assert np.array_equal(np.asarray(a[r][0]), np.asarray(b[r][0])) and np.array_equal(np.asarray(a[r][1]), np.asarray(b[r][1])), r


def test_routes_equal_the_torch_selection(pg, monkeypatch):
    from prograph_amd import _native
    P, tok = pg
    op = fit_alignment(score_table(np.random.default_rng(31), 21, -6, 2, diag=np.arange(3, 8)), 2, 3)
    Q = np.zeros((5, 200), dtype=np.int64)
    Q[:, :150] = tok[[0, 3, 9, 30, 8], 50:200]
    Q[2, 140:] = 0
    ran = []
    for name in ("alignment_fit_long_dense", "alignment_fit_dense", "alignment_semiglobal_long_dense", "i32_knn", "i32_eps"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _f=real, _n=name, **kw: (ran.append(_n), _f(*a, **kw))[1])
    knn = P.build_graph(k=5, distance=op)
    eps = max(1, int(np.median(np.array([w for _, w in knn])[:, 1])))

    def calls():
        return [P.build_graph(k=5, distance=op), P.build_graph(k=N - 1, distance=op), P.build_graph(eps=eps, distance=op),
                P.search(Q, k=3, distance=op), P.search(Q, eps=eps, distance=op), P.search(Q, k=N, distance=op)]
    del ran[:]
    native = calls()
    assert ran.count("alignment_fit_long_dense") >= 6 and ran.count("i32_knn") == 4 and ran.count("i32_eps") == 2
    assert not [n for n in ran if "semiglobal" in n or n == "alignment_fit_dense"]
    G = P.build_graph(k=5, distance=op, output="csr", store="FitLong")
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int32 and G.idx.is_cuda and G.similarity is False
    assert np.array_equal(P.degree("FitLong"), np.array([w for _, w in native[0]]).sum(1).astype(np.float32))
    assert sum(len(i) for i, _ in native[2]) > 0 and min(w.min() for _, w in native[1]) < 0
    del ran[:]
    monkeypatch.setattr(_native, "aln_long_ready", lambda: False)
    generic = calls()
    assert not ran
    for a, b in zip(native, generic):
        _same(a, b)


# ---------------------------------------------------------------- 4. the long traceback
def test_the_long_traceback_is_the_canonical_alignment(pg):
    P, tok = pg
    rng = np.random.default_rng(3)
    S = score_table(rng, 21, -6, 2, diag=np.arange(3, 8))
    op = fit_alignment(S, 2, 3)
    T = tok[:, :200].copy()
    T[lengths(tok) > 200, 199] = 1                                # rows cut at 200 end in a symbol
    xi, yi = rng.integers(0, N, 40), rng.integers(0, N, 40)
    xi[:2], yi[:2] = (8, 0), (7, 0)
    A = op.align(torch.from_numpy(T[xi]).cuda(), torch.from_numpy(T[yi]).cuda()).host()      # width 200: the strip kernel
    for p in range(40):
        want = canonical(S, 2, 3, seq(T[xi[p]]), seq(T[yi[p]]))
        got = tuple(int(getattr(A, f)[p]) for f in ("score", "x_begin", "x_end", "y_begin", "y_end", "n_ops", "identities"))
        assert got == want[:7] and A.ops[p, :want[5]].tolist() == want[7] and not A.ops[p, want[5]:].any(), (p, got, want)
    # 2048 x 2048 once, a row within a column that holds it after 100 symbols, against the host expression
    big = rows_of(rng, 21, (2048, 1948), 2048)
    big[0, 100:2048] = big[1, :1948]
    big[0, 700:703] = (3, 4, 5)
    B = op.align(torch.from_numpy(big[:1]).cuda(), torch.from_numpy(big[1:]).cuda()).host()
    *fields, ops = alignments.host_trace(alignments.FIT, S, 2, 3, big[:1], big[1:])
    assert [int(getattr(B, f)[0]) for f in ("score", "x_begin", "x_end", "y_begin", "y_end", "n_ops", "identities")] == [int(f[0]) for f in fields]
    assert np.array_equal(B.ops.numpy(), ops) and int(B.x_begin[0]) == 100 and int(B.x_end[0]) == 2048 and int(B.y_end[0]) == 1948
    # the edges of a graph on the int32 route: x is the containing column, the score the edge's weight
    G = P.build_graph(k=2, distance=op, output="csr")
    E = P.align(G, distance=op).host()
    idx, w = G.idx.cpu().numpy(), G.dist.cpu().numpy()
    assert len(E) == 2 * N and np.array_equal(E.score.numpy(), w.reshape(-1))
    for p in (0, 15, 16, 17, 119):
        want = canonical(S, 2, 3, seq(tok[int(idx[p // 2, p % 2])]), seq(tok[p // 2]))
        assert tuple(int(getattr(E, f)[p]) for f in ("score", "x_begin", "x_end", "y_begin", "y_end", "n_ops", "identities")) == want[:7]
