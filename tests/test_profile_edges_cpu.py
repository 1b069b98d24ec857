"""
What the profile kernels' edge tests rest on, without a GPU (inputs: tests/profile_edges_testdata.py).

`definition` of tests/profile_testdata.py is held against `brute_force` on profiles drawn from {-128, -1, 0, 1, 127} and
against the operator's torch expression on a sample of every family; an empty profile scores 0 under it; every input set is
shown, from the data, to hold what tests/test_profile_extremes_gpu.py and tests/test_profile_lengths_gpu.py are about; and
the three `fits` predicates are pinned on both sides of every bound those files run at.
"""
import numpy as np
import pytest
import torch

import profile_edges_testdata as D
from local_testdata import lengths
from profile_testdata import MODES, brute_force, definition
from prograph_amd import _native
from prograph_amd.distance import profile_alignment


# ---------------------------------------------------------------- the yardstick at the extremes
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gap,gap_open", D.GAPS)
def test_the_recurrence_is_the_worded_definition_at_extreme_entries(mode, gap, gap_open):
    """Profiles of 1..4 positions over three symbols: a spiky one and one of each other family, against every kind of row of
    up to 4 symbols (symbol 0 only inside a row)."""
    rng = np.random.default_rng(gap)
    profiles = [D.family("spiky", rng, l, 3) for l in (1, 2, 3, 4, 4)] + [D.family(name, rng, l, 3) for name, l in
                                                                         (("ceiling", 4), ("floor", 3), ("nonneg", 4), ("trap", 3))]
    assert all(set(np.unique(P)) <= set(D.SPIKES) for P in profiles[:7])
    rows = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [2, 1, 0, 0], [0, 2, 0, 0], [1, 1, 1, 0], [2, 0, 1, 0], [1, 2, 2, 1], [0, 0, 1, 2],
                     [2, 2, 0, 1], [1, 1, 1, 1]])
    got = definition(mode, profiles, gap, gap_open, rows)
    lens = lengths(rows)
    for q, P in enumerate(profiles):
        for c in range(len(rows)):
            assert got[q, c] == brute_force(mode, P, gap, gap_open, list(rows[c, :lens[c]])), (q, c)
    assert (got > 0).any() and ((got < 0).any() if mode == "fit" else (got >= 0).all())


@pytest.mark.parametrize("mode", MODES)
def test_the_operator_on_cpu_tensors_equals_the_definition_on_every_family(mode):
    """Profiles of 1, 17 and 40 positions of every family in one call and in a call of their own."""
    rows = D.short_rows(21)[::6, :40]
    at = [k for k, P in enumerate(D.short_profiles(21)) if len(P) in (1, 17)]
    rng = np.random.default_rng(40)
    profiles = [D.short_profiles(21)[k] for k in at] + [D.family(name, rng, 40, 21) for name in D.FAMILIES]
    for gap, gap_open in ((3, 11), (255, 255)):
        want = definition(mode, profiles, gap, gap_open, rows)
        op = profile_alignment(mode, gap, gap_open)
        assert np.array_equal(op(torch.from_numpy(rows.copy()), profiles).numpy(), want)
        for f in range(len(D.FAMILIES)):
            assert np.array_equal(op(torch.from_numpy(rows.copy()), profiles[f::5]).numpy(), want[f::5]), D.FAMILIES[f]


@pytest.mark.parametrize("mode", MODES)
def test_an_empty_profile_scores_nothing(mode):
    """What the C entries answer for a length of 0 or less (plus out_bias in mode 2): H[0][0] = 0 is the only cell."""
    X = D.short_rows(21)[:9]
    for gap, gap_open in ((1, 0), (3, 11), (255, 255)):
        got = definition(mode, [np.zeros((0, 21), dtype=np.int64), D.short_profiles(21)[7]], gap, gap_open, X)
        assert (got[0] == 0).all() and np.array_equal(got[1:], definition(mode, [D.short_profiles(21)[7]], gap, gap_open, X))


# ---------------------------------------------------------------- the short sets hold what their tests are about
@pytest.mark.parametrize("a", D.SYMBOLS)
def test_families_have_their_ranges_and_rows_their_lengths(a):
    profiles, X = D.short_profiles(a), D.short_rows(a)
    assert len(profiles) == 35 and [len(P) for P in profiles] == [l for l in D.SHORT_LENS for _ in D.FAMILIES]
    for name in D.FAMILIES:
        mine = [profiles[k] for k in D.members(name)]
        assert [len(P) for P in mine] == list(D.SHORT_LENS) and all(P.shape[1] == a for P in mine)
        for P in mine:                                            # every single profile: so does any call of the family
            assert (-min(0, int(P.min())), max(0, int(P.max()))) == D.RANGE[name], name
            assert P.max() >= 1                                   # the operator takes it
        buf, _, l, bias, top = _native.profile_pack(mine)
        assert (bias, top, l) == D.RANGE[name] + (128,) and buf.shape == (7, 32, 128)
        assert buf.max() == bias + top and (buf[:, :a].min() == 0)
        if name in ("ceiling", "spiky"):
            assert buf.max() == 255                               # byte 255 is in the operand
    assert D.RANGE["nonneg"][0] == 0 and D.RANGE["floor"] == (128, 1)
    buf, _, _, bias, top = _native.profile_pack(profiles)
    assert (bias, top) == (128, 127)                              # the call of all families
    assert all(np.unique(P).tolist() == [-128, 127] for P in (profiles[k] for k in D.members("ceiling")))
    assert all(set(np.unique(P)) <= set(D.SPIKES) for P in (profiles[k] for k in D.members("spiky")))
    for P in (profiles[k] for k in D.members("trap")):
        assert (P[:, 0] == 127).all() and P[:, 1:].max() <= 3
    assert X.shape == (134, 128) and sorted(lengths(X[:130])) == sorted(list(range(129)) + [77])
    inner = [(X[r, :lengths(X)[r]] == 0).any() for r in range(134)]
    assert sum(inner[:130]) >= 20 and inner[133] and X.max() == a - 1 and X.min() == 0
    assert lengths(X[130:]).tolist() == [128, 127, 64, 128] and (X[130] == 1).all()
    for r0, r1 in D.ROW_RANGES:
        assert r0 % 8 and (r1 - 1) // 8 >= r0 // 8 and r1 <= 35
    assert any((r1 - 1) // 8 > r0 // 8 for r0, r1 in D.ROW_RANGES)


def test_the_ceiling_reaches_its_cells():
    """min(len x, L) * 127 against the constant rows: 16 256 at 128 against 128, in every mode at gap 1 / 0 (fit: L <= len x;
    a shorter row leaves L - len x positions unaligned)."""
    X = D.short_rows(21)[130:]
    ceiling = [D.short_profiles(21)[k] for k in D.members("ceiling")]
    for mode in MODES:
        got = definition(mode, ceiling, 1, 0, X)
        for q, L in enumerate(D.SHORT_LENS):
            for c, lx in enumerate((128, 127, 64)):
                if mode != "fit" or L <= lx:
                    assert got[q, c] == min(lx, L) * 127, (mode, L, lx)
                else:
                    assert got[q, c] == lx * 127 - (L - lx)
        assert got[6, 0] == 16256 == got.max()
        assert got[6, 3] < 16256                                  # the interior 0 meets the -128 of position 64
    assert 16 * 127 <= 2048 < 17 * 127 and D.SHORT_LENS[:D.FEW] == (1, 15, 16)


@pytest.mark.parametrize("mode,gap,gap_open", [("local", 1, 0), ("semiglobal", 1, 0), ("semiglobal", 3, 11), ("semiglobal", 255, 255),
                                               ("fit", 255, 255), ("fit", 255, 128), ("fit", 254, 255)])
def test_the_floor_is_at_work(mode, gap, gap_open):
    """The floor family's terms, left to the recurrence, go below -Z: the saturating subtraction holds them at 0 = -Z.  (Fit
    at 1 / 0 and 3 / 11 stays 1 and 3 above it, -255 against -256 and -520 against -523: an H of fit is never below
    -(o + j e), so only an E, an F or an aligned-pair term of -128 can pass -Z, and they do at the large penalties.)"""
    floor = [D.short_profiles(21)[k] for k in D.members("floor")]
    x = D.short_rows(21)[130]
    assert len(floor[-1]) == 128 and lengths(x[None])[0] == 128
    Z = D.cell_offset(mode, gap, gap_open, 128, 128, D.RANGE["floor"][1])
    assert Z == {"local": 0, "semiglobal": 128, "fit": gap_open + 128 * (gap + 1)}[mode]
    low, _ = D.table_low(mode, floor[-1], gap, gap_open, list(x))
    assert low < -Z, (low, Z)
    # the floor-less loop is the definition's recurrence: fit has no floor, and its score is the best of column L
    for P in (floor[-1], floor[3], D.short_profiles(21)[D.members("spiky")[4]]):
        _, column = D.table_low("fit", P, gap, gap_open, list(x[:70]))
        assert max(column) == definition("fit", [P], gap, gap_open, x[None, :70])[0, 0]


# ---------------------------------------------------------------- the long sets
def test_the_length_sets_hold_every_strip_count_chunk_count_and_fill():
    assert sorted(D.LENS_A) == list(range(1, 258)) and D.LENS_A != tuple(range(1, 258)) and len(D.LENS_B) == 32 and max(D.LENS_B) == 2048
    assert {1024, 1025, 2047, 2048} <= set(D.LENS_B)
    for ns in (1, 2, 3):                                          # set A: every NC of a last strip at 1, 2 and 3 strips
        assert {D.last_nc(l) for l in D.LENS_A if D.strips(l) == ns} == ({1} if ns == 3 else set(range(1, 9)))
    assert {D.strips(l) for l in D.LENS_B} == set(range(3, 17))
    assert {D.strips(l) for l in D.LENS_A + D.LENS_B} == set(range(1, 17))
    assert {D.last_nc(l) for l in D.LENS_B} == set(range(1, 9))
    ends = {(l - 1) % 128 + 1 for l in D.LENS_B}                  # the positions of the last strip
    assert set(D.B_ENDS) <= ends and len(D.B_ENDS) == 16
    for nc in range(1, 9):                                        # both ends of every NC
        assert {16 * nc - 15, 16 * nc} <= ends and D.last_nc(16 * nc - 15) == D.last_nc(16 * nc) == nc
    second = {D.fills(l)[1] for l in D.LENS_B if len(D.fills(l)) == 2}
    assert second == set(range(1, 9)) and all(D.fills(l)[0] == 8 for l in D.LENS_B if len(D.fills(l)) == 2)
    assert D.fills(1024) == [8] and D.fills(1025) == [8, 1] and D.fills(2048) == [8, 8]
    assert D.LENS_C == (1, 17, 128) and all(D.strips(l) == 1 for l in D.LENS_C)
    # one workgroup: 17 profiles = three groups of 8, 300 rows = two column tiles, a long profile before a short one
    assert len(D.LENS_ONE) == 17 and D.ONE_ROWS > 256 and D.LENS_ONE[:7] == (2048, 5, 129, 1, 1025, 128, 300)
    ns = [D.strips(l) for l in D.LENS_ONE]
    assert sum(a > b for a, b in zip(ns, ns[1:])) >= 6 and sum(a < b for a, b in zip(ns, ns[1:])) >= 6 and {1, 2, 3, 5, 9, 16} <= set(ns)
    for which, lens in (("A", D.LENS_A), ("B", D.LENS_B), ("C", D.LENS_C), ("one", D.LENS_ONE)):
        profiles = D.long_profiles(which)
        assert tuple(len(P) for P in profiles) == lens
        assert all(P.min() >= -6 and P.max() == 9 and P.shape[1] == 21 for P in profiles)
    for which, shape in (("A", (64, 131)), ("B", (24, 37)), ("one", (300, 131))):
        X = D.long_rows(which)
        lx = lengths(X)
        assert X.shape == shape and shape[1] % 4 and lx.max() == shape[1] and lx.min() == 0 and X.max() == 20
        assert sum((X[r, :lx[r]] == 0).any() for r in range(len(X))) >= len(X) // 8
    buf, lens, l, bias, top = _native.profile_pack(D.long_profiles("A"))
    assert (l, buf.shape[2], bias, top) == (257, 384, 6, 9)


# ---------------------------------------------------------------- the bounds
def test_the_fits_predicates_at_their_edges():
    loc, semi, fit = _native.aln_local_long_fits, _native.aln_semiglobal_long_fits, _native.aln_fit_fits
    # up to 128 positions with top = 127
    assert D.local_cell(128, 128, 127) == 16511 and loc(128, 128, 127) and D.semiglobal_cell(128, 128, 127) == 32767 and semi(128, 128, 127)
    assert D.fit_cell(128, 127, 255, 128) == 65535 and fit(128, 128, 127, 255, 128)
    assert D.fit_cell(128, 127, 254, 255) == 65534 and fit(128, 128, 127, 254, 255)
    assert D.fit_cell(128, 127, 255, 255) == 65662 and not fit(128, 128, 127, 255, 255)
    assert not fit(128, 128, 127, 255, 129)
    assert D.fit_cell(128, 1, 255, 255) == 33406 and fit(128, 128, 1, 255, 255)          # the floor family: every pair
    assert D.fit_cell(16, 127, 255, 255) == 8654 and fit(128, 16, 127, 255, 255)         # the profiles of 1, 15, 16 positions
    for gap, gap_open in D.FIT_GAPS:
        assert fit(128, 128, 127, gap, gap_open) == ((gap, gap_open) != (255, 255))
    # 2048 x 2048
    assert D.local_cell(2048, 2048, 31) == 63743 and loc(2048, 2048, 31)
    assert D.local_cell(2048, 2048, 32) == 65791 and not loc(2048, 2048, 32)
    assert D.semiglobal_cell(2048, 2048, 15) == 61695 and semi(2048, 2048, 15)
    assert D.semiglobal_cell(2048, 2048, 16) == 65791 and not semi(2048, 2048, 16)
    assert D.fit_cell(2048, 15, 1, 255) == 63998 and fit(2048, 2048, 15, 1, 255)
    assert D.fit_cell(2048, 15, 2, 0) == 65791 and not fit(2048, 2048, 15, 2, 0)
    assert D.fit_cell(2048, 14, 3, 255) == 63998 and fit(2048, 2048, 14, 3, 255)
    # top = 127 against wide rows: the last profile lengths that fit
    assert D.local_cell(2048, 514, 127) == 65533 and loc(2048, 514, 127) and D.local_cell(2048, 515, 127) == 65660 and not loc(2048, 515, 127)
    assert D.semiglobal_cell(2048, 257, 127) == 65533 and semi(2048, 257, 127)
    assert D.semiglobal_cell(2048, 258, 127) == 65787 and not semi(2048, 258, 127)
    # the widths: min() of the two for local and semi-global, the profile's alone for fit; 2049 never
    assert loc(514, 2048, 127) and semi(257, 2048, 127) and fit(2048, 128, 127, 255, 128) and not fit(128, 2048, 127, 255, 128)
    assert not loc(2049, 1, 1) and not semi(1, 2049, 1) and not fit(2049, 1, 1, 1, 0)
    op = profile_alignment("fit", 255, 255)
    assert op._fits(128, 128, 1) and not op._fits(128, 128, 127) and op._select_bias(128) == 255 + 255 * 128


def test_the_search_profiles_leave_the_fp16_route():
    """40 * 127 > 2048: nine profiles of at most 40 positions with top = 127 select from int32 blocks in every mode."""
    for mode in MODES:
        op = profile_alignment(mode, 20, 50)
        assert not op._f16_route(40, 40, 127) and op._fits(40, 40, 127)
        assert op._f16_route(40, 40, 9 if mode != "fit" else 1)
