"""
Alignment distances and local scores beyond 128 positions on the GPU: `pg_alignment_long_dense` /
`pg_alignment_local_long_dense` on every entry against the definitions of tests/long_testdata.py (global) and
tests/local_testdata.py (local), at 2048 positions against the operators' torch expression on CPU tensors, the int32
selection against a stable sort / mask, and `build_graph` / `search` against the same calls with the long route switched
off (the generic loop / the torch selection).  Every comparison is an every-entry equality.
"""
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import local_testdata
import long_testdata
from long_testdata import cost_table, csr_of, knn_of, lengths, rows_of
from prograph_amd import synth
from prograph_amd.distance import alignment, local_alignment

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

OPS = {"le": operator.le, "lt": operator.lt, "eq": operator.eq, "ge": operator.ge, "gt": operator.gt}
LENS = (0, 1, 127, 128, 129, 130, 143, 144, 145, 255, 256, 257, 300)      # around every strip and chunk seam
W = 300
# (alphabet, gap, gap_open, largest cost): 300 * 215 + 2 * 255 + 2 * 215 = 65 440 is the most 16-bit cells admit at 300
GLOBAL = [(5, 1, 0, 215), (32, 3, 11, 200), (32, 215, 255, 215)]
LOCAL = [(5, 1, 0), (32, 3, 11), (32, 255, 255)]


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def operand(nat, a, T):
    op = nat.aln_long_operand(torch.from_numpy(np.ascontiguousarray(T).astype(np.uint8)), a)
    assert op.valid()
    return op


def run(nat, kind, table, gap, gap_open, X, Y, **kw):
    xo, yo = operand(nat, len(table), X), operand(nat, len(table), Y)
    if kind == "global":
        assert nat.aln_long_fits(max(X.shape[1], Y.shape[1]), max(int(table.max()), gap), gap, gap_open)
        return nat.alignment_long_dense(xo, yo, nat.sub_cost(table), gap, gap_open, **kw).cpu().numpy()
    assert nat.aln_local_long_fits(X.shape[1], Y.shape[1], int(table.max()))
    return nat.alignment_local_long_dense(xo, yo, nat.aln_local_score(table), gap, gap_open, **kw).cpu().numpy()


def cases():
    out = [("global", a, e, o, top) for a, e, o, top in GLOBAL] + [("local", a, e, o, None) for a, e, o in LOCAL]
    return pytest.mark.parametrize("kind,a,gap,gap_open,top", out)


def table_of(rng, kind, a, top):
    if kind == "global":
        return cost_table(rng, a, top)
    S = local_testdata.score_table(rng, a, -9, 6, diag=np.arange(2, 12))
    S[0, :] = S[:, 0] = 5                                         # padding would score if it were let in
    return S


def define(kind, table, gap, gap_open, X, Y):
    f = long_testdata.definition if kind == "global" else local_testdata.definition
    return f(table, gap, gap_open, X, Y)


# ---------------------------------------------------------------- 1. the dense kernel against the definition
@cases()
def test_every_length_against_every_length(nat, kind, a, gap, gap_open, top):
    """13 rows of every length of LENS against 39 columns (each length three times, equal pairs among them: columns
    0..12 repeat the rows' symbols); int64 and int32, whole and as row ranges; both operands at their own widths."""
    rng = np.random.default_rng(100 * a + gap)
    T = table_of(rng, kind, a, top)
    Y = rows_of(rng, a, list(LENS), W)
    X = np.concatenate([Y, rows_of(rng, a, list(LENS) * 2, W)])
    want = define(kind, T, gap, gap_open, X, Y)
    got = run(nat, kind, T, gap, gap_open, X, Y)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    if kind == "global":
        assert (np.diag(want[:, :13]) == 0).all()
    got = run(nat, kind, T, gap, gap_open, X, Y, out_bytes=4)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    for r0, r1 in ((3, 13), (0, 1), (4, 12)):
        assert np.array_equal(run(nat, kind, T, gap, gap_open, X, Y, out_bytes=4, rows=(r0, r1)), want[r0:r1])
    # X wide on the short Y path and the reverse: the operands' widths need not agree
    assert np.array_equal(run(nat, kind, T, gap, gap_open, X, Y[:2, :40]), want[:2])
    assert np.array_equal(run(nat, kind, T, gap, gap_open, X[:2, :40], Y), want[:, :2])


@pytest.mark.parametrize("kind,a,gap,gap_open,top", [("global", 21, 2, 7, 90), ("local", 21, 2, 7, None)])
def test_a_lane_a_length_and_interior_zeros(nat, kind, a, gap, gap_open, top):
    rng = np.random.default_rng(7)
    T = table_of(rng, kind, a, top)
    X = rows_of(rng, a, list(rng.permutation(np.arange(1, 301))[:64]) + list(range(300, 294, -1)), W)      # a wave and a bit
    Y = rows_of(rng, a, [300, 129, 257], W)
    assert len(set(lengths(X[:64]))) == 64
    assert np.array_equal(run(nat, kind, T, gap, gap_open, X, Y), define(kind, T, gap, gap_open, X, Y))
    X[::3, 2], X[1::5, 0], X[::7, 128], Y[0, 127:130], Y[1, :16] = 0, 0, 0, 0, 0          # interior zeros: symbol 0
    X[7, 100:] = 0
    X[7, 260] = 3                                                 # zeros inside, a symbol after them
    assert lengths(X)[7] == 261
    assert np.array_equal(run(nat, kind, T, gap, gap_open, X, Y), define(kind, T, gap, gap_open, X, Y))


@pytest.mark.parametrize("kind,a,gap,gap_open,top", [("global", 21, 1, 11, 60), ("local", 21, 1, 11, None)])
def test_two_row_groups_two_column_tiles(nat, kind, a, gap, gap_open, top):
    """9 rows x 300 columns: two row groups and two column tiles, both partial; more items than one workgroup's share
    when the workspace holds one workgroup only."""
    rng = np.random.default_rng(8)
    T = table_of(rng, kind, a, top)
    X, Y = rows_of(rng, a, rng.integers(100, 301, 300), W), rows_of(rng, a, rng.integers(100, 301, 9), W)
    X[17, :150] = Y[4, 20:170]                                    # something to find
    want = define(kind, T, gap, gap_open, X, Y)
    assert np.array_equal(run(nat, kind, T, gap, gap_open, X, Y, out_bytes=4), want)
    # the smallest workspace: one workgroup loops over all four items
    import ctypes
    xo, yo = operand(nat, a, X), operand(nat, a, Y)
    one = ctypes.c_int64(0)
    assert nat.lib().pg_alignment_long_workspace(W, ctypes.byref(one), None) == 0 and one.value == 256 * W * 4
    ws = torch.empty(one.value, dtype=torch.uint8, device=xo.buf.device)
    out = torch.empty((9, 300), dtype=torch.int64, device=xo.buf.device)
    tab = nat.sub_cost(T) if kind == "global" else nat.aln_local_score(T)
    entry = nat.lib().pg_alignment_long_dense if kind == "global" else nat.lib().pg_alignment_local_long_dense
    args = [xo.buf.data_ptr(), 300, xo.npad, W, yo.buf.data_ptr(), 9, yo.npad, W, tab.data_ptr(), gap, gap_open, out.data_ptr(), 300, 8]
    assert entry(*args, ws.data_ptr(), one.value, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert entry(*args, ws.data_ptr(), one.value - 1, None) == -1          # PG_E_BADARG: less than one workgroup's share


# ---------------------------------------------------------------- 2. 2048 positions
LONG = (2048, 2047, 1921, 1920, 1025, 3)


def test_2048_positions_global(nat):
    rng = np.random.default_rng(11)
    C = cost_table(rng, 21, 31)                                   # 2048 * 31 + 2 * 11 + 2 * 3 <= 65 535
    X, Y = rows_of(rng, 21, LONG, 2048), rows_of(rng, 21, LONG, 2048)
    g = 40
    Y[0, :2048 - g] = np.delete(X[0], np.arange(700, 700 + g))    # x without one block of g symbols
    Y[0, 2048 - g:] = 0
    Y[1] = X[1]
    for gap, gap_open in ((1, 0), (3, 11)):
        op = alignment(C, gap, gap_open)
        want = op(torch.from_numpy(X), torch.from_numpy(Y)).numpy()          # the torch expression on CPU tensors
        got = run(nat, "global", C, gap, gap_open, X, Y)
        assert np.array_equal(got, want)
        assert got[1, 1] == 0 and got[0, 0] == gap_open + g * gap
        dev = op(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())     # the operator takes the long kernel
        assert dev.dtype == torch.int64 and np.array_equal(dev.cpu().numpy(), want)


def test_2048_positions_local(nat):
    rng = np.random.default_rng(12)
    S = np.full((21, 21), -8)
    S[np.arange(21), np.arange(21)] = rng.integers(4, 32, 21)     # a positive diagonal, the rest negative
    S[1, 1] = 31                                                  # 2048 * 31 + 255 <= 65 535: the largest cell of the route
    X, Y = rows_of(rng, 21, LONG, 2048), rows_of(rng, 21, LONG, 2048)
    Y[1] = X[1]
    Y[2] = 1                                                      # 2048 ones against
    X[2] = 1                                                      # 2048 ones: 63 488
    Y[3] = 0
    Y[3, :40] = X[0, 1000:1040]                                   # a fragment of a 2048-row
    for gap, gap_open in ((1, 0), (3, 11)):
        op = local_alignment(S, gap, gap_open)
        want = op(torch.from_numpy(X), torch.from_numpy(Y)).numpy()
        got = run(nat, "local", S, gap, gap_open, X, Y)
        assert np.array_equal(got, want)
        assert got[1, 1] == S[X[1, :2047], X[1, :2047]].sum() and got[2, 2] == 2048 * 31 == 63488          # row 1: 2047 symbols
        assert got[3, 0] == S[Y[3, :40], Y[3, :40]].sum()
        dev = op(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
        assert dev.dtype == torch.int64 and np.array_equal(dev.cpu().numpy(), want)


# ---------------------------------------------------------------- 3. padding and the 16-bit edge
def test_padding_never_scores_across_strips(nat):
    """The table of the 128-position kernel's trap: S[0][0] = 127 and S[a][0] > 0, so a padding byte let into a profile,
    or a cell past len x folded into the maximum, shows.  len y on both sides of a strip seam, both operand orders."""
    rng = np.random.default_rng(13)
    S = local_testdata.score_table(rng, 21, -6, 3, diag=np.arange(2, 9))
    S[0, :] = S[:, 0] = 9
    S[0, 0] = 127
    A = rows_of(rng, 21, [127, 128, 129, 144], W)
    B = rows_of(rng, 21, [300, 256, 130, 1, 0, 128, 129, 200] + list(rng.integers(1, 301, 60)), W)
    for gap, gap_open in ((1, 0), (2, 5)):
        want = local_testdata.definition(S, gap, gap_open, B, A)
        assert np.array_equal(run(nat, "local", S, gap, gap_open, B, A), want)
        assert np.array_equal(run(nat, "local", S, gap, gap_open, A, B), want.T)


def test_a_cell_at_the_bound(nat):
    """Constant rows drive H to the largest value the route predicate admits at 300 positions: 300 pairs at 215 = 64 500,
    and one pair plus a run of 299 = 215 + 255 + 299 * 215 = 64 755, reached through E and through F; the sums formed
    before a min reach 65 440.  One more unit of cost is outside the predicate."""
    from prograph_amd import _native
    C = np.zeros((21, 21), dtype=np.int64)
    C[3, 7] = C[7, 3] = 215
    assert _native.aln_long_fits(300, 215, 215, 255) and not _native.aln_long_fits(300, 216, 215, 255)
    X, Y = np.full((70, W), 3), np.full((9, W), 7)
    Y[1, 1:] = 0                                                  # a single 7: the run is in X
    X[5, 1:] = 0                                                  # a single 3: the run is in Y
    X[6, :] = 0
    want = long_testdata.definition(C, 215, 255, X, Y)
    assert want[0, 0] == 64500 and want[1, 0] == 64755 and want[0, 5] == 64755 and want[0, 6] == 255 + 300 * 215
    assert np.array_equal(run(nat, "global", C, 215, 255, X, Y), want)
    assert np.array_equal(run(nat, "global", C, 215, 255, Y, X, out_bytes=4), want.T)


# ---------------------------------------------------------------- 4. the int32 selection
@pytest.mark.parametrize("m,n", [(7, 1), (5, 64), (9, 65), (3, 1000)])
def test_i32_selection(nat, m, n):
    rng = np.random.default_rng(m * n)
    D = rng.choice(np.array([0, 0, 1, 5, 5, 65535, 65536, 70000, 70000, 2**31 - 1]), (m, n)).astype(np.int64)
    D[0] = 70000                                                  # a row of ties
    block = torch.from_numpy(D.astype(np.int32)).cuda()
    for desc in (False, True):
        order = np.argsort(-D if desc else D, axis=1, kind="stable")
        for first in (0, 1):
            for k in (1, 63, 64, 100):
                if first + k > 64 and not 64 - first < k:
                    continue
                idx, w = nat.i32_knn(block, k, first=first, descending=desc)
                assert idx.dtype == torch.int32 and w.dtype == torch.int32 and idx.shape == (m, k)
                have = max(0, min(k, n - first))
                want = order[:, first:first + have]
                assert np.array_equal(idx.cpu().numpy()[:, :have], want), (desc, first, k)
                assert np.array_equal(w.cpu().numpy()[:, :have], np.take_along_axis(D, want, 1))
                assert (idx.cpu().numpy()[:, have:] == -1).all() and (w.cpu().numpy()[:, have:] == 0).all()
    for name, comp in OPS.items():
        for thr in (-1, 0, 5, 65535, 70000, 2**31 - 1, 2**40):
            for keep_zero in (False, True):
                ip, ix, w = nat.i32_eps(block, getattr(nat, "CMP_" + name.upper()), thr, keep_zero=keep_zero)
                wp, wx, ww = csr_of(D, comp, thr, keep_zero=keep_zero)
                assert w.dtype == torch.int32 and np.array_equal(ip.cpu().numpy(), wp), (name, thr, keep_zero)
                assert np.array_equal(ix.cpu().numpy(), wx) and np.array_equal(w.cpu().numpy(), ww)


# ---------------------------------------------------------------- 5. the routes
N = 120


@pytest.fixture(scope="module")
def pg(tmp_path_factory):
    from prograph_amd import Prograph
    rng = np.random.default_rng(21)
    tok = rows_of(rng, 21, rng.integers(100, 301, N), W)
    tok[7] = tok[8]                                               # duplicates
    tok[30] = tok[90]
    tok[40] = 0
    tok[40, :120] = tok[41, 60:180]                               # fragments
    tok[50] = 0
    tok[50, :100] = tok[51, :100]
    tok[0, :300] = rng.integers(1, 21, 300)
    f = tmp_path_factory.mktemp("long") / "long.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": rng.uniform(0, 1, N)}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P, tok


def _arrays(got):
    return [np.asarray(i) for i, _ in got], [np.asarray(w) for _, w in got]


def _same(a, b):
    (ai, aw), (bi, bw) = _arrays(a), _arrays(b)
    assert len(ai) == len(bi)
    for r in range(len(ai)):
        assert np.array_equal(ai[r], bi[r]) and np.array_equal(aw[r], bw[r]), r


def _distances(rng):
    S = local_testdata.score_table(rng, 21, -6, 2, diag=np.arange(3, 8))
    return [alignment(cost_table(rng, 21, 9), 2), alignment(cost_table(rng, 21, 30), 1, gap_open=11), local_alignment(S, 2, 3)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_routes_equal_the_generic_loop(pg, which, monkeypatch):
    from prograph_amd import _native
    P, tok = pg
    op = _distances(np.random.default_rng(31))[which]
    Q = np.zeros((5, W + 9), dtype=np.int64)
    Q[:, :W] = tok[[3, 50, 99, 100, 8]]
    Q[3, 250:W + 6] = 5
    Q[2, 140:] = 0
    eps = int(np.median(np.array(_arrays(P.build_graph(k=5, distance=op))[1])[:, -1]))         # half of the rows have five within it
    ran = []
    for name in ("alignment_long_dense", "alignment_local_long_dense", "i32_knn", "i32_eps"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _f=real, _n=name, **kw: (ran.append(_n), _f(*a, **kw))[1])
    def calls():
        return [P.build_graph(k=5, distance=op), P.build_graph(eps=eps, distance=op), P.search(Q, k=3, distance=op),
                P.search(Q, eps=eps, distance=op), P.build_graph(eps=eps, distance=op, comp=operator.lt, idxs=np.arange(20, 100))]
    monkeypatch.setattr(type(P), "_BLOCK_ELEMS", N * 2 * 70)      # int32 blocks of 70 rows: two row blocks, three for k
    native = calls()
    dense = "alignment_long_dense" if which < 2 else "alignment_local_long_dense"
    assert ran.count(dense) == 2 + 2 + 1 + 1 + 1 and ran.count("i32_knn") == 3 and ran.count("i32_eps") == 4
    G = P.build_graph(k=5, distance=op, output="csr", store="Long")
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int32 and G.idx.is_cuda
    idx, w = _arrays(native[0])
    assert np.array_equal(G.idx.cpu().numpy(), np.array(idx)) and np.array_equal(G.dist.cpu().numpy(), np.array(w))
    assert np.array_equal(P.degree("Long"), np.array(w).sum(1).astype(np.float32))
    assert sum(len(i) for i in _arrays(native[1])[0]) > N and sum(len(i) for i in _arrays(native[3])[0]) > 5
    del ran[:]
    monkeypatch.setattr(_native, "aln_long_ready", lambda: False)
    generic = calls()
    assert not ran
    for a, b in zip(native, generic):
        _same(a, b)
