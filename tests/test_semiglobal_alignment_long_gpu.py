"""
Semi-global alignment scores beyond 128 positions on the GPU: `pg_alignment_semiglobal_long_dense`
(prograph_amd/csrc/pg_aln_semiglobal.hip) on every entry against `definition` of tests/semiglobal_testdata.py around every
strip and slot boundary, at 2048 positions against the operator's torch expression on CPU tensors, and `build_graph` /
`search` against the same calls with the long route switched off.  Every comparison is an every-entry equality.
"""
import itertools

import numpy as np
import pandas as pd
import pytest
import torch

from semiglobal_testdata import definition, lengths, rows_of, score_table
from prograph_amd import synth
from prograph_amd.distance import semiglobal_alignment

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

GAPS = ((1, 0), (3, 11))


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def run(nat, S, gap, gap_open, X, Y, **kw):
    xo = nat.aln_long_operand(torch.from_numpy(np.ascontiguousarray(X).astype(np.uint8)), len(S))
    yo = nat.aln_long_operand(torch.from_numpy(np.ascontiguousarray(Y).astype(np.uint8)), len(S))
    assert xo.valid() and yo.valid() and nat.aln_semiglobal_long_fits(X.shape[1], Y.shape[1], int(S.max()))
    return nat.alignment_semiglobal_long_dense(xo, yo, nat.aln_local_score(S), gap, gap_open, **kw).cpu().numpy()


def table(rng, a=21):
    S = score_table(rng, a, -9, 6, diag=np.arange(2, 12))
    S[0, :] = S[:, 0] = 5                                         # padding would score if it were let in
    return S


def related(rng, X, Y, inside=True):
    """Make some columns overlap some rows or (`inside`) lie inside them, in place; only the latter changes a length."""
    lx, ly = lengths(X), lengths(Y)
    for c in range(min(len(X), (3 if inside else 2) * len(Y))):
        r = c % len(Y)
        l = int(min(lx[c], ly[r]) * 2 // 3)
        if l < 2:
            continue
        if c // len(Y) == 0:
            X[c, lx[c] - l:lx[c]] = Y[r, :l]                      # x ends as y begins
        elif c // len(Y) == 1:
            X[c, :l] = Y[r, ly[r] - l:ly[r]]                      # x begins as y ends
        else:
            X[c, :lx[c]] = 0
            X[c, :l] = Y[r, (ly[r] - l) // 2:(ly[r] - l) // 2 + l]      # x lies inside y


# ---------------------------------------------------------------- 1. the dense kernel against the definition
@pytest.mark.parametrize("gap,gap_open", GAPS)
def test_lengths_around_the_strip_seams(nat, gap, gap_open):
    rng = np.random.default_rng(100 + gap)
    S = table(rng)
    lens = (129, 255, 256, 257, 300)
    Y = rows_of(rng, 21, lens, 300)
    X = rows_of(rng, 21, list(lens) * 3 + [0, 1, 128], 300)
    related(rng, X, Y)
    want = definition(S, gap, gap_open, X, Y)
    got = run(nat, S, gap, gap_open, X, Y)
    assert got.dtype == np.int64 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    got = run(nat, S, gap, gap_open, X, Y, out_bytes=4)           # int32 blocks = int64
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(run(nat, S, gap, gap_open, X, Y, out_bytes=4, rows=(1, 4)), want[1:4])
    assert np.array_equal(run(nat, S, gap, gap_open, Y, X), want.T)
    assert np.array_equal(run(nat, S, gap, gap_open, X, Y[:2, :40]), definition(S, gap, gap_open, X, Y[:2, :40]))


@pytest.mark.parametrize("gap,gap_open", GAPS)
def test_the_slot_boundary_at_1024(nat, gap, gap_open):
    """len y = 1024 and 1025: eight strips fill the profile slots once, the ninth starts the second fill; against short
    X rows so that the numpy loop stays small, and in the other order (len x beyond 1024, one strip of Y)."""
    rng = np.random.default_rng(200 + gap)
    S = table(rng)
    Y = rows_of(rng, 21, [1024, 1025, 1023], 1025)
    X = rows_of(rng, 21, [40, 17, 64, 65, 70, 1, 33, 70, 48], 70)
    related(rng, X, Y)
    want = definition(S, gap, gap_open, X, Y)
    assert np.array_equal(run(nat, S, gap, gap_open, X, Y), want)
    assert np.array_equal(run(nat, S, gap, gap_open, Y, X, out_bytes=4), want.T)


def test_every_pair_of_lengths_around_128_and_384(nat):
    rng = np.random.default_rng(3)
    S = table(rng)
    lens = (127, 128, 129, 384, 385)
    pairs = list(itertools.product(lens, lens))
    Y = rows_of(rng, 21, lens, 385)
    X = rows_of(rng, 21, list(lens) * 3, 385)
    related(rng, X, Y, inside=False)
    assert set(zip(np.repeat(lengths(Y), 15), np.tile(lengths(X), 5))) == set(pairs)
    for gap, gap_open in ((2, 5),):
        want = definition(S, gap, gap_open, X, Y)
        assert np.array_equal(run(nat, S, gap, gap_open, X, Y), want)


def test_a_lane_a_length_and_interior_zeros(nat):
    rng = np.random.default_rng(7)
    S = table(rng)
    X = rows_of(rng, 21, list(rng.permutation(np.arange(129, 401))[:64]) + list(range(400, 394, -1)), 400)      # a wave and a bit
    Y = rows_of(rng, 21, [400, 129, 257], 400)
    assert len(set(lengths(X[:64]))) == 64
    X[::3, 2], X[1::5, 0], X[::7, 128], Y[0, 127:130], Y[1, :16] = 0, 0, 0, 0, 0          # interior zeros: symbol 0
    related(rng, X, Y)
    assert np.array_equal(run(nat, S, 2, 7, X, Y), definition(S, 2, 7, X, Y))


def test_where_the_best_cell_lies(nat):
    """A table under which only equal symbols score: x = y[40:100] ends in row len x at column 100, inside strip 0 of a
    row of three strips; x = the last 30 symbols of y and then something else ends in column len y at outer step 30."""
    rng = np.random.default_rng(9)
    S = np.full((21, 21), -20)
    S[np.arange(21), np.arange(21)] = rng.integers(3, 9, 21)
    Y = rows_of(rng, 21, [300, 290, 384], 384, low=11)            # symbols 11..20
    X = np.zeros((70, 300), dtype=np.int64)
    X[:] = rows_of(rng, 11, [200] * 70, 300)                      # symbols 1..10: nothing in common with Y
    inner, tail = Y[0, 40:100], Y[0, 270:300]
    X[0] = 0
    X[0, :60] = inner
    X[1, :30] = tail
    want = definition(S, 30, 0, X, Y)
    assert want[0, 0] == S[inner, inner].sum() and want[0, 1] == S[tail, tail].sum() and (want[:, 2:] == 0).all()
    got = run(nat, S, 30, 0, X, Y)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(run(nat, S, 30, 0, Y, X), want.T)


def test_padding_never_scores_across_strips(nat):
    """The padding trap of the 128-position kernel's tests at 257 positions, the widest the bound admits with a score of
    127 in the table (2 * 257 * 127 + 255 = 65 533): len y on both sides of two strip seams, both operand orders."""
    rng = np.random.default_rng(13)
    S = score_table(rng, 21, -6, 3, diag=np.arange(2, 9))
    S[0, :] = S[:, 0] = 9
    S[0, 0] = 127
    A = rows_of(rng, 21, [127, 128, 129, 144], 257)
    B = rows_of(rng, 21, [257, 256, 130, 1, 0, 128, 129, 200] + list(rng.integers(1, 258, 60)), 257)
    for gap, gap_open in ((1, 0), (2, 5)):
        want = definition(S, gap, gap_open, B, A)
        assert np.array_equal(run(nat, S, gap, gap_open, B, A), want)
        assert np.array_equal(run(nat, S, gap, gap_open, A, B), want.T)


# ---------------------------------------------------------------- 2. 2048 positions
LONG = (2048, 2047, 1921, 1025, 3)


@pytest.mark.parametrize("top,gap,gap_open", [(11, 1, 0), (15, 3, 11)])
def test_2048_positions(nat, top, gap, gap_open):
    """max(S) = 11 (BLOSUM62's) and 15, the largest the bound admits at 2048 positions (2 * 2048 * 15 + 255 = 61 695;
    16 is outside): against the operator's torch expression on CPU tensors."""
    rng = np.random.default_rng(12 + top)
    S = np.full((21, 21), -4)
    S[np.arange(21), np.arange(21)] = rng.integers(4, top + 1, 21)
    S[1, 1] = top
    assert nat.aln_semiglobal_long_fits(2048, 2048, top) and not nat.aln_semiglobal_long_fits(2048, 2048, 16)
    X, Y = rows_of(rng, 21, LONG, 2048), rows_of(rng, 21, LONG, 2048)
    Y[1] = X[1]
    Y[2], X[2] = 1, 1                                             # 2048 ones against 2048 ones: 2048 * top, cells of 2 Z
    Y[3] = 0
    Y[3, :1000] = X[0, 1048:]                                     # y begins as x ends
    X[4] = 0
    X[4, :40] = Y[0, 1000:1040]                                   # a fragment of a 2048-row
    op = semiglobal_alignment(S, gap, gap_open)
    want = op(torch.from_numpy(X), torch.from_numpy(Y)).numpy()          # the torch expression on CPU tensors
    got = run(nat, S, gap, gap_open, X, Y)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert got[1, 1] == S[X[1, :2047], X[1, :2047]].sum() and got[2, 2] == 2048 * top
    assert got[3, 0] == S[Y[3, :1000], Y[3, :1000]].sum() and got[0, 4] == S[X[4, :40], X[4, :40]].sum()
    dev = op(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())     # the operator takes the long kernel
    assert dev.dtype == torch.int64 and np.array_equal(dev.cpu().numpy(), want)


# ---------------------------------------------------------------- 3. the routes
N, W = 200, 400


@pytest.fixture(scope="module")
def pg(tmp_path_factory):
    from prograph_amd import Prograph
    rng = np.random.default_rng(21)
    tok = rows_of(rng, 21, rng.integers(150, 401, N), W)
    tok[7] = tok[8]                                               # duplicates
    tok[40] = 0
    tok[40, :120] = tok[41, 60:180]                               # a fragment
    tok[50, :100] = tok[51, lengths(tok)[51] - 100:lengths(tok)[51]]          # 50 begins as 51 ends
    tok[0, :400] = rng.integers(1, 21, 400)
    f = tmp_path_factory.mktemp("semilong") / "long.csv"
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
    op = semiglobal_alignment(score_table(np.random.default_rng(31), 21, -6, 2, diag=np.arange(3, 8)), 2, 3)
    Q = np.zeros((5, W + 9), dtype=np.int64)
    Q[:, :W] = tok[[3, 50, 99, 100, 8]]
    Q[2, 140:] = 0
    ran = []
    for name in ("alignment_semiglobal_long_dense", "alignment_local_long_dense", "alignment_local_dense", "i32_knn", "i32_eps"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _f=real, _n=name, **kw: (ran.append(_n), _f(*a, **kw))[1])
    knn = P.build_graph(k=5, distance=op)
    eps = int(np.median(np.array([w for _, w in knn])[:, -1]))    # half of the rows have five at or above it

    def calls():
        return [P.build_graph(k=5, distance=op), P.build_graph(eps=eps, distance=op), P.search(Q, k=3, distance=op),
                P.search(Q, eps=eps, distance=op)]
    del ran[:]
    native = calls()
    assert ran.count("alignment_semiglobal_long_dense") >= 4 and ran.count("i32_knn") == 2 and ran.count("i32_eps") == 2
    assert not [n for n in ran if "local" in n]                   # never the local kernels
    G = P.build_graph(k=5, distance=op, output="csr", store="SemiLong")
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int32 and G.idx.is_cuda and G.similarity is False
    assert np.array_equal(P.degree("SemiLong"), np.array([w for _, w in native[0]]).sum(1).astype(np.float32))
    assert native[0][40][0][0] == 41 and native[0][7][0][0] == 8 and sum(len(i) for i, _ in native[1]) > 0
    del ran[:]
    monkeypatch.setattr(_native, "aln_long_ready", lambda: False)
    generic = calls()
    assert not ran
    for a, b in zip(native, generic):
        _same(a, b)
