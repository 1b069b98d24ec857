"""
The inputs and yardsticks of tests/test_alignment_lengths_gpu.py without a GPU (tests/aln_lengths_testdata.py): the Y sets
hold the lengths they are said to hold, and those lengths reach every (strip count, NC of the last strip) pair, every
position of the select chain and every nb of the second profile fill - asserted over the generated rows, not described;
the X operands are what the kernels' edges need; the three `definition` functions agree with the operators' torch
expressions on CPU tensors on a subsample (every eighth row of S and A, the two longest rows of B) and with
trace_testdata.brute_force on sequences of up to 5 symbols; and the related columns give the score modes something to
find.  Everything here is asserted from the inputs and the references alone.
"""
import itertools

import numpy as np
import pytest
import torch

import aln_lengths_testdata as D
import trace_testdata
from long_testdata import lengths, rows_of
from prograph_amd import _native
from prograph_amd.distance import alignment, local_alignment, semiglobal_alignment

OPERATOR = {"global": alignment, "local": local_alignment, "semiglobal": semiglobal_alignment}
NCS, POSITIONS = set(range(1, 9)), set(range(1, 17))


# ---------------------------------------------------------------- 1. the lengths and what they reach
def test_set_s_every_length_every_instance_every_select():
    lens = D.lens_s()
    assert sorted(lens) == list(range(129)) and lens != sorted(lens)
    assert np.array_equal(lengths(D.y("S")), lens) and D.y("S").shape == (129, 128)
    assert {D.strips(l) for l in lens} == {0, 1}
    assert {(D.last_nc(l), D.select_pos(l)) for l in lens} == {(0, 0)} | set(itertools.product(NCS, POSITIONS))
    # neighbouring rows of a workgroup (8 rows) differ in NC, from whichever row a range starts
    assert all(len({D.last_nc(l) for l in lens[r:r + 8]}) >= 3 for r in range(len(lens) - 7))


def test_set_a_every_length_in_a_first_and_in_a_second_last_strip():
    lens = D.lens_a()
    assert sorted(lens) == list(range(257)) and lens != sorted(lens)
    assert np.array_equal(lengths(D.y("A")), lens) and D.y("A").shape == (257, 256)
    reached = {(D.strips(l), D.last_nc(l), D.select_pos(l)) for l in lens}
    assert reached == {(0, 0, 0)} | set(itertools.product((1, 2), NCS, POSITIONS))
    assert {tuple(D.fills(l)) for l in lens} == {(), (1,), (2,)}
    assert all(len({(D.strips(l), D.last_nc(l)) for l in lens[r:r + 8]}) >= 3 for r in range(len(lens) - 7))


def test_set_b_every_strip_count_with_every_instance_and_every_second_fill():
    lens = D.lens_b()
    formula = [128 * s + 16 * nc + 1 + (5 * s + 3 * nc) % 16 for s in range(2, 16) for nc in range(8)]
    assert len(formula) == 112 and max(formula) == 2033 and len(set(lens)) == 114
    assert sorted(lens) == sorted(formula + [2047, 2048])
    assert np.array_equal(lengths(D.y("B")), lens) and D.y("B").shape == (114, 2048)
    assert {(D.strips(l), D.last_nc(l)) for l in lens} == set(itertools.product(range(3, 17), NCS))
    for s, nc in itertools.product(range(2, 16), range(8)):
        assert D.last_nc(D.b_length(s, nc)) == nc + 1 and D.strips(D.b_length(s, nc)) == s + 1
    assert {D.select_pos(l) for l in lens} == POSITIONS
    for nc in NCS:                                                # 5 s mod 16 takes 14 values over s = 2..15
        assert len({D.select_pos(l) for l in lens if D.last_nc(l) == nc}) >= 14
    for s in range(3, 17):
        assert len({D.select_pos(l) for l in lens if D.strips(l) == s}) >= 8
    assert {D.fills(l)[0] for l in lens} == set(range(3, 9))
    assert {D.fills(l)[1] for l in lens if len(D.fills(l)) > 1} == set(range(1, 9))         # nb of the second fill
    assert all(len(D.fills(l)) == 1 + (l > 1024) and sum(D.fills(l)) == D.strips(l) for l in lens)
    assert lens != sorted(lens)
    assert all(len({D.strips(l) for l in lens[r:r + 8]}) >= 3 for r in range(0, len(lens) - 7, 8))
    # the rows of the test with both operands long: one per NC, of 5, 9, 12 and 16 strips
    many = [int(l) for l in lengths(D.y_many())]
    assert many == D.B_MANY and {D.last_nc(l) for l in many} == NCS
    assert sorted({D.strips(l) for l in many}) == [5, 9, 12, 16]


def test_the_helpers_are_the_kernels_arithmetic():
    for l in range(0, 2049):
        ns = (l + 127) // 128                                     # the kernels' own expressions
        assert D.strips(l) == ns
        if l:
            rest = l - 128 * (ns - 1)
            assert D.last_nc(l) == (rest + 15) >> 4
            assert D.select_pos(l) == rest - ((rest - 1) & ~15) == rest - 16 * (D.last_nc(l) - 1)
        assert D.fills(l) == [min(8, ns - s0) for s0 in range(0, ns, 8)]


def test_the_x_operands():
    X = D.x("x47")
    lx = lengths(X)
    assert X.shape == (70, 47) and X.shape[1] % 4 and np.array_equal(lx, D.lens_x47())
    assert list(lx[64:]) == [47, 1, 0, 33, 16, 17]
    assert len(set(lx[:64])) > 30 and lx[:64].max() <= 47
    X2 = D.x("x128")
    lx2 = lengths(X2)
    assert X2.shape == (130, 128) and list(lx2[124:]) == [128, 127, 0, 1, 16, 17] and np.array_equal(lx2, D.lens_x128())
    assert {D.last_nc(l) for l in lx2} == {0} | NCS               # transposed: every instance on the lane side too
    X3 = D.x("x199")
    lx3 = lengths(X3)
    assert X3.shape == (64, 199) and X3.shape[1] % 4 and len(set(lx3)) == 64 and lx3.min() == 1 and lx3.max() == 199
    for T in (X, X2, X3, D.y("S"), D.y("A"), D.y("B")):
        l = lengths(T)
        inside = np.arange(T.shape[1])[None, :] < l[:, None]
        assert T.min() == 0 and T.max() == D.SYMS - 1 and ((T == 0) & inside).any() and not T[~inside].any()
        assert not T.flags.writeable
    for name in ("S", "A", "B"):                                  # deterministic
        assert np.array_equal(D.generate_y(name), D.y(name))
    for name in ("x47", "x128", "x199"):
        again, related = D.generate_x(name)
        assert np.array_equal(again, D.x(name)) and related == D.related(name)
        assert all(l >= 16 for _, _, _, _, l in related)          # a related column takes at least a chunk of its row


def test_tables_penalties_and_the_kernels_bounds():
    S = D.score()
    assert (S == S.T).all() and (S[0] == 5).all() and S[1:, 1:].min() >= -9 and S.max() <= 11
    assert (np.diag(S)[1:] >= 2).all()
    for top in (15, 31, 215, 255):
        C = D.cost(top)
        assert (C == C.T).all() and C.max() == top and C.min() == 0 and not np.diag(C).any()
    assert _native.aln_long_fits(300, 215, 215, 255) and not _native.aln_long_fits(300, 216, 215, 255)
    assert _native.aln_long_fits(2048, 31, 3, 11) and not _native.aln_long_fits(2048, 32, 3, 11)
    for xw, yw in ((199, 2048), (256, 256)):
        assert _native.aln_local_long_fits(xw, yw, int(S.max())) and _native.aln_semiglobal_long_fits(xw, yw, int(S.max()))
    everywhere = {(m, e, o) for m in D.MODES for e, o in D.GAPS}
    assert {(m, e, o) for m, e, o, _ in D.CASES_A} == everywhere | {("global", 215, 255)}
    assert {(m, e, o) for m, e, o, _ in D.CASES_B} == {(m, e, o) for m in D.MODES for e, o in D.GAPS}
    assert {(m, e, o) for m, e, o, _ in D.CASES_S} == {(m, e, o) for m in D.MODES for e, o in D.GAPS + ((255, 255),)}
    # where the fp16 output of the kernels up to 128 positions is exact: every value within 2048
    assert 128 * 15 + 11 <= 2048 and 128 * int(S.max()) <= 2048


# ---------------------------------------------------------------- 2. the yardsticks against the operators' torch expression
def _operator(mode, gap, gap_open, top, X, Y):
    op = OPERATOR[mode](D.table_of(mode, top), gap, gap_open)
    got = op(torch.from_numpy(np.array(X)), torch.from_numpy(np.array(Y)))          # copies: the inputs are read-only
    assert got.dtype == torch.int64 and not got.is_cuda
    return got.numpy()


@pytest.mark.parametrize("mode,gap,gap_open,top", D.CASES_S)
def test_definitions_equal_the_operators_on_set_s(mode, gap, gap_open, top):
    X, Y = D.x("x128"), D.y("S")[::8]
    assert len(Y) == 17
    want = D.DEFINITION[mode](D.table_of(mode, top), gap, gap_open, X, Y)
    assert want.shape == (17, 130) and np.array_equal(_operator(mode, gap, gap_open, top, X, Y), want)


@pytest.mark.parametrize("mode,gap,gap_open,top", D.CASES_A)
def test_definitions_equal_the_operators_on_set_a(mode, gap, gap_open, top):
    X, Y = D.x("x47"), D.y("A")[::8]
    assert len(Y) == 33
    want = D.DEFINITION[mode](D.table_of(mode, top), gap, gap_open, X, Y)
    assert want.shape == (33, 70) and np.array_equal(_operator(mode, gap, gap_open, top, X, Y), want)
    assert np.array_equal(_operator(mode, gap, gap_open, top, Y, X), want.T)      # both are symmetric in their operands


@pytest.mark.parametrize("mode,gap,gap_open,top", D.CASES_B)
def test_definitions_equal_the_operators_on_the_longest_rows_of_set_b(mode, gap, gap_open, top):
    X, Y = D.x("x47"), D.y("B")
    rows = [D.row_of_length(Y, 2048), D.row_of_length(Y, 2047)]
    want = D.DEFINITION[mode](D.table_of(mode, top), gap, gap_open, X, Y[rows])
    assert np.array_equal(_operator(mode, gap, gap_open, top, X, Y[rows]), want)
    if mode != "global":                                          # the related columns of these rows: something to find
        S = D.score()
        found = [(c, kind, r, l) for c, kind, which, r, l in D.related("x47") if which == "B"]
        assert sorted(kind for _, kind, _, _ in found) == [D.PIECE, D.BEGINNING, D.END, D.OVERLAP]
        assert {r for _, _, r, _ in found} == set(rows)
        for c, kind, r, l in found:
            piece = X[c, :l]
            assert want[rows.index(r), c] >= S[piece, piece].sum() >= 2 * l, (c, kind)


# ---------------------------------------------------------------- 3. the related columns
@pytest.mark.parametrize("name,which", [("x47", "A"), ("x128", "S")])
def test_related_columns_give_the_scores_something_to_find(name, which):
    X, Y, S = D.x(name), D.y(which), D.score()
    found = [(c, kind, r, l) for c, kind, w, r, l in D.related(name) if w == which]
    assert {kind for _, kind, _, _ in found} == {D.PIECE, D.BEGINNING, D.END, D.OVERLAP}
    cols, rows = sorted({c for c, _, _, _ in found}), sorted({r for _, _, r, _ in found})
    lx, ly = lengths(X), lengths(Y)
    for mode in ("local", "semiglobal"):
        want = D.DEFINITION[mode](S, 3, 11, X[cols], Y[rows])
        others = [r for r in range(len(Y)) if r not in rows][:8]
        unrelated = np.median(D.DEFINITION[mode](S, 3, 11, X[cols], Y[others]), axis=0)
        for c, kind, r, l in found:
            piece = X[c, :l]
            own = S[piece, piece].sum()                           # the piece aligned with itself, its ends free
            assert want[rows.index(r), cols.index(c)] >= own > unrelated[cols.index(c)], (mode, c, kind)
            if kind == D.OVERLAP:
                assert l < lx[c] and np.array_equal(piece, Y[r, ly[r] - l:ly[r]])  # in column len y, at step l < len x
            if kind == D.PIECE and ly[r] > l:
                assert l == lx[c]                                 # found in row len x, at a column j < len y


def test_related_columns_of_the_test_with_both_operands_long():
    X, Y = D.x("x199"), D.y_many()
    ly = lengths(Y)
    found = D.related("x199")
    assert [kind for _, kind, _, _, _ in found] == [D.PIECE, D.BEGINNING, D.END, D.OVERLAP] * 2
    for (c, kind, which, r, l), row in zip(found, range(8)):
        assert which == "B" and np.array_equal(D.y("B")[r], Y[row]) and l >= 85
        y, p = Y[row, :ly[row]], X[c, :l]
        seam = 1024 if ly[row] > 1024 + l else 128                # a piece lies across the seam of the second fill
        at = {D.PIECE: seam - l // 2, D.BEGINNING: 0}.get(kind, ly[row] - l)
        assert np.array_equal(y[at:at + l], p)


# ---------------------------------------------------------------- 4. the yardsticks against a brute force
@pytest.mark.parametrize("mode,gap,gap_open", [("global", 3, 11), ("local", 3, 2), ("semiglobal", 2, 5)])
def test_definitions_equal_a_brute_force_on_short_sequences(mode, gap, gap_open):
    """Every alignment path of every admissible pair of substrings, sequences of 0..5 symbols with symbol 0 among them.
    Small penalties in the score modes, so that gapped alignments are among the best."""
    rng = np.random.default_rng(41)
    T = D.cost(15) if mode == "global" else D.score()
    X, Y = rows_of(rng, 6, [0, 1, 2, 3, 4, 5, 5, 4], 5), rows_of(rng, 6, [5, 0, 3, 1, 4, 2, 5], 5)
    X[5, 1], Y[0, 2], X[6] = 0, 0, Y[0]
    X[6, 3] = 0
    want = D.DEFINITION[mode](T, gap, gap_open, X, Y)
    code = getattr(trace_testdata, mode.upper())
    for r in range(len(Y)):
        for c in range(len(X)):
            assert trace_testdata.brute_force(code, T, gap, gap_open, X[c], Y[r]) == want[r, c], (mode, r, c)
