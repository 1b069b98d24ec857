"""
Without a GPU: the C oracle's plain Wagner-Fischer matrix (`c_oracle.lev_matrix`, orc_lev_matrix) pinned against the two
numpy references, and what the sets of tests/lev_every_testdata.py cover, asserted from the lengths alone - the claims the
GPU file tests/test_levenshtein_every_length_gpu.py relies on.
"""
import numpy as np
import pytest

import lev_every_testdata as EV
import lev_long_testdata as LL
import lev_testdata as LT
from oracle import c_oracle as C


# ---------------------------------------------------------------- 1. the reference
def test_oracle_matrix_equals_the_numpy_reference_on_the_long_set():
    X, Y = LL.long_x(), LL.long_y()
    got = C.lev_matrix(X, Y)
    assert got.shape == (13, 64) and got.dtype == np.int64 and np.array_equal(got, LL.long_matrix())
    got32 = C.lev_matrix(X, Y, dtype=np.int32)
    assert got32.dtype == np.int32 and np.array_equal(got32, LL.long_matrix())
    assert np.array_equal(C.lev_matrix(Y, X), LL.long_matrix().T)            # the operands the other way round


def test_oracle_matrix_equals_the_double_loop_up_to_260_positions():
    X, Y = LL.long_x(), LL.long_y()
    xs = [r for r, l in enumerate(LL.X_LENS) if l <= 260]
    ys = [i for i, l in enumerate(LL.Y_LENS) if l <= 260]
    assert len(xs) >= 25 and len(ys) >= 8
    want = LT.wagner_fischer(X[xs][:, :260], Y[ys][:, :260])
    assert np.array_equal(C.lev_matrix(X[xs][:, :260], Y[ys][:, :260]), want)
    assert np.array_equal(C.lev_matrix(X[xs][:, :260], Y[ys]), want)         # operands of different widths
    assert np.array_equal(C.lev_matrix(X[xs], Y[ys][:, :257]), want)
    E = EV.set_e()                                                           # and on rows of the new set
    rows, cols = np.arange(0, 258, 9), np.arange(3, 258, 5)
    assert np.array_equal(EV.d_ee()[np.ix_(rows, cols)], LT.wagner_fischer(E[cols], E[rows]))


def test_oracle_matrix_on_empty_rows_and_homopolymers():
    lens = np.array([0, 1, 2, 127, 128, 129, 1000, 2047, 2048, 0])
    H = np.zeros((len(lens), 2048), dtype=np.uint8)
    for r, l in zip(H, lens):
        r[:l] = 31
    assert np.array_equal(C.lev_matrix(H, H), np.abs(lens[:, None] - lens[None, :]))     # 2048 x 2048 among them
    R = np.random.default_rng(3).integers(1, 32, (4, 300)).astype(np.uint8)
    Z = np.zeros((2, 7), dtype=np.uint8)
    assert np.array_equal(C.lev_matrix(R, Z), np.full((2, 4), 300))          # d(empty, x) = len x, both ways
    assert np.array_equal(C.lev_matrix(Z, R), np.full((4, 2), 300))
    assert np.array_equal(C.lev_matrix(Z, Z), np.zeros((2, 2)))
    G = R.copy()
    G[1, 100:] = 0                                                           # the prefix ends at the first zero
    G[1, 200] = 5
    assert C.lev_matrix(G[1:2], R[1:2])[0, 0] == 200
    with pytest.raises(ValueError):
        C.lev_matrix(np.ones((1, 2049), np.uint8), R)
    with pytest.raises(TypeError):
        C.lev_matrix(R, R, dtype=np.int16)


# ---------------------------------------------------------------- 2. what the lengths cover
def test_coverage_functions():
    f = [(l, EV.chunks(l), EV.segments(l), EV.tail(l)) for l in (0, 1, 32, 33, 127, 128, 129, 160, 161, 2047, 2048)]
    assert f == [(0, 0, 0, 0), (1, 1, 1, 1), (32, 1, 1, 32), (33, 1, 2, 1), (127, 1, 4, 31), (128, 1, 4, 32),
                 (129, 2, 1, 1), (160, 2, 1, 32), (161, 2, 2, 1), (2047, 16, 4, 31), (2048, 16, 4, 32)]
    for l in range(1, 2049):
        assert 128 * (EV.chunks(l) - 1) + 32 * (EV.segments(l) - 1) + EV.tail(l) == l
        w, bit = EV.last_row(l)
        assert 128 * (EV.blocks(l) - 1) + 32 * w + bit == l - 1 and 0 <= w < 4 and 0 <= bit < 32
    assert EV.last_row(0) is None and EV.blocks(0) == 0
    assert [EV.instance(w) for w in (1, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048)] == [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]


def test_set_e_holds_every_length_mixed_in_every_wave():
    E, le = EV.set_e(), EV.lens_e()
    assert E.shape == (258, 257) and sorted(le) == list(range(258)) and np.array_equal(LT.lengths(E), le)
    assert E.max() == 31 and all((r[:l] != 0).all() and not r[l:].any() for r, l in zip(E, le))
    for w in range(0, 256, 64):                                              # no full wave of columns is all short or all long
        wave = le[w:w + 64]
        assert min(wave) < 64 and max(wave) > 192 and {EV.blocks(l) for l in wave} >= {1, 2}
    # as texts: every (segments, tail) of a first and a second chunk; as patterns: every (dword, bit) of two blocks
    assert {(EV.chunks(l), EV.segments(l), EV.tail(l)) for l in le} >= {(c, s, t) for c in (1, 2) for s in range(1, 5) for t in range(1, 33)}
    assert {(EV.blocks(l),) + EV.last_row(l) for l in le if l} >= {(b, w, i) for b in (1, 2) for w in range(4) for i in range(32)}
    assert {LL.FAMILIES[r % 7] for r in range(258)} == set(LL.FAMILIES)
    D = EV.d_ee()
    assert D.shape == (258, 258) and (np.diag(D) == 0).all() and np.array_equal(D, D.T)
    assert ((D > 0) & (D <= 8)).sum() >= 500 and (D >= 200).sum() >= 500      # related rows near, unrelated rows far
    la = np.array(le)
    assert (np.abs(la[:, None] - la[None, :]) <= D).all() and (D <= np.maximum(la[:, None], la[None, :])).all()
    # the rows that fit each instance's operand
    assert [len(EV.at_width(E, w)[1]) for w in (128, 256, 257, 1024, 2048)] == [129, 257, 258, 258, 258]
    assert [EV.instance(w) for w in (128, 256, 257, 1024, 2048)] == list(EV.INSTANCES)


def test_set_t_holds_every_chunk_count_segment_count_and_tail():
    T, lt = EV.set_t(), EV.lens_t()
    assert T.shape == (58, 2048) and np.array_equal(LT.lengths(T), lt) and T.max() <= 31
    formula = [EV.t_length(c, g) for c in range(2, 16) for g in range(4)]
    assert sorted(lt) == sorted(formula + [2047, 2048]) and len(set(lt)) == 58
    assert min(formula) == 271 and max(formula) == 2041
    assert {(EV.chunks(l), EV.segments(l)) for l in formula} == {(c, s) for c in range(3, 17) for s in range(1, 5)}
    assert {EV.tail(l) for l in formula} == set(range(1, 33))
    assert {EV.tail(l) % 2 for l in formula if EV.chunks(l) == 16} == {0, 1}  # odd and even trip counts at 16 chunks
    assert (EV.chunks(2047), EV.segments(2047), EV.tail(2047)) == (16, 4, 31)
    D = EV.d_t_ep()
    assert D.shape == (58, 288) and D.dtype == np.int64
    la, lb = np.array(lt), np.array(EV.lens_ep())
    assert (np.abs(la[:, None] - lb[None, :]) <= D).all() and (D <= np.maximum(la[:, None], lb[None, :])).all()
    DP, gap = D[:, 258:], np.abs(la[:, None] - lb[None, 258:])                # long texts against long patterns:
    assert ((DP > 0) & (DP <= 16)).sum() >= 10 and (DP - gap <= 16).sum() >= 500    # a few edits beyond the length gap
    assert (DP - gap >= 100).sum() >= 300                                     # and unrelated ones


def test_set_p_puts_the_last_row_in_every_dword_of_every_block_count():
    P, lp = EV.set_p(), EV.lens_p()
    assert P.shape == (30, 2048) and np.array_equal(LT.lengths(P), lp) and P.max() <= 31
    formula = lp[:28]
    assert [EV.blocks(l) for l in formula] == [b for b in range(3, 17) for _ in range(2)] and lp[28:] == [2047, 2048]
    places = [EV.last_row(l) for l in formula]
    assert len(set(places)) == 28
    for w in range(4):
        bits = sorted(bit for ww, bit in places if ww == w)
        assert len(bits) == 7 and bits[0] == 0 and bits[-1] == 31             # r = 1 and r = 32 of the dword
        assert {b % 2 for b in bits[1:-1]} == {0, 1}
    for b in range(3, 17):                                                    # the two rows of a block count: two dwords
        assert len({EV.last_row(l)[0] for l in formula if EV.blocks(l) == b}) == 2
    assert EV.set_ep().shape == (288, 2048) and np.array_equal(LT.lengths(EV.set_ep()), EV.lens_ep())
    D = EV.d_e_ep()
    assert D.shape == (258, 288) and not D.flags.writeable
    la, lb = np.array(EV.lens_e()), np.array(EV.lens_ep())
    assert (np.abs(la[:, None] - lb[None, :]) <= D).all() and (D <= np.maximum(la[:, None], lb[None, :])).all()


@pytest.mark.parametrize("nb", [4, 8, 16])
def test_long_lane_columns_put_a_top_block_pattern_in_every_wave(nb):
    cols, lens = EV.long_lane_columns(nb), np.array(EV.lens_ep())
    assert lens[cols].max() <= 128 * nb and set(range(258)) <= set(cols.tolist())
    assert set(cols.tolist()) == {c for c in range(288) if lens[c] <= 128 * nb}    # every row of P that fits is there
    for w in range(0, len(cols), 64):
        wave = lens[cols[w:w + 64]]
        assert max(EV.blocks(l) for l in wave) == nb and min(wave) < 64        # nbw = NB beside short lanes
