"""
The inputs of the profile kernels' edge tests (tests/test_profile_edges_cpu.py pins them; tests/test_profile_extremes_gpu.py
and tests/test_profile_lengths_gpu.py run them): profile FAMILIES at the ends of the operand contract of
include/prograph_hip.h - entries -128..127, bias 0..128, top 0..127 - and the profile LENGTH SETS of the strip-mined kernel.
Everything is built from seeds.  The yardstick stays `definition` of tests/profile_testdata.py; `table_low` here is the same
recurrence WITHOUT any floor, one pair at a time, which says how far below -Z a mode's cells would go.  Of prograph_amd only
constants are imported.
"""
import functools

import numpy as np

from aln_lengths_testdata import fills, last_nc, strips                      # pure arithmetic on a length
from local_testdata import lengths, rows_of
from profile_testdata import definition, random_profile
from prograph_amd._native import ALN_LONG_CELL_MAX, ALN_LONG_MAX_L, ALN_MAX_L

assert (ALN_MAX_L, ALN_LONG_MAX_L, ALN_LONG_CELL_MAX) == (128, 2048, 65535)

# ---------------------------------------------------------------- the families
FAMILIES = ("ceiling", "floor", "nonneg", "spiky", "trap")
RANGE = {"ceiling": (128, 127), "floor": (128, 1), "nonneg": (0, 127), "spiky": (128, 127), "trap": (6, 127)}     # (bias, top)
SPIKES = (-128, -1, 0, 1, 127)
SYMBOLS = (2, 21, 32)
SHORT_LENS = (1, 15, 16, 17, 64, 127, 128)
FEW = 3                                                          # the profiles of 1, 15 and 16 positions: 16 * 127 <= 2048
GAPS = ((1, 0), (3, 11), (255, 255))                             # local and semi-global
FIT_GAPS = GAPS + ((255, 128), (254, 255))                       # fit: those the bound admits for the call's top
ROW_RANGES = ((5, 6), (7, 9), (3, 20))                           # start inside a group of 8 profiles, cross one


def _two_places(rng, P):
    """Two different flat positions of P."""
    return rng.choice(P.size, 2, replace=False)


def family(name, rng, l, a):
    """One (l, a) profile of the family; every profile holds its family's least and largest entry, so that a call of any of
    its profiles has the (bias, top) of RANGE.
        ceiling  127 everywhere, -128 at (l // 2, symbol 0): a row of one symbol >= 1 gains 127 a position
        floor    -128 everywhere but +1 at every fifth position: top = 1, so Z is small and the cells fall 128 a step
        nonneg   0..127 with a 0 and a 127: bias = 0, a real score of 0 and a masked byte are the same byte
        spiky    random from SPIKES with a -128 and a 127
        trap     127 for symbol 0 at every position, -6..3 elsewhere with a -6: a padding byte that scored would gain 127"""
    if name == "ceiling":
        P = np.full((l, a), 127)
        P[l // 2, 0] = -128
    elif name == "floor":
        P = np.full((l, a), -128)
        j = np.arange(0, l, 5)
        P[j, 1 + j % (a - 1)] = 1
    elif name == "nonneg":
        P = rng.integers(0, 128, (l, a))
        P.flat[_two_places(rng, P)] = (0, 127)
    elif name == "spiky":
        P = rng.choice(np.array(SPIKES), (l, a))
        P.flat[_two_places(rng, P)] = (-128, 127)
    else:
        assert name == "trap"
        P = rng.integers(-6, 4, (l, a))
        P[:, 0] = 127
        P[rng.integers(0, l), rng.integers(1, a)] = -6
    return P


@functools.lru_cache(maxsize=None)
def short_profiles(a):
    """The 35 profiles of one alphabet in the order of the call that holds them all - every family at length 1, then every
    family at 15, ... - so that a group of 8 profiles mixes families and lengths; read-only."""
    rng = np.random.default_rng(2000 + a)
    out = tuple(family(name, rng, l, a) for l in SHORT_LENS for name in FAMILIES)
    for P in out:
        P.setflags(write=False)
    return out


def members(name):
    """The places of a family's seven profiles in `short_profiles`, by ascending length."""
    return [k * len(FAMILIES) + FAMILIES.index(name) for k in range(len(SHORT_LENS))]


N_CONSTANT = 4


@functools.lru_cache(maxsize=None)
def short_rows(a):
    """134 rows of 128 positions: "a lane a length" - 130 rows, every length 0..128, an interior 0 in every fifth - and four
    constant rows that drive the ceiling: 128 ones, 127 of the last symbol, 64 ones, 128 ones around an interior 0."""
    rng = np.random.default_rng(1000 + a)
    lanes = rows_of(rng, a, list(rng.permutation(129)) + [77], 128)
    lanes[(np.arange(130) % 5 == 0) & (lengths(lanes) > 4), 3] = 0
    const = np.zeros((N_CONSTANT, 128), dtype=np.int64)
    const[0], const[1, :127], const[2, :64], const[3] = 1, a - 1, 1, 1
    const[3, 64] = 0
    X = np.concatenate([lanes, const])
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def short_want(a, mode, gap, gap_open):
    """The yardstick's (35, 134) matrix: one pass, shared by every call of the case (a profile's scores do not depend on its
    companions, so a family's own call and the call of all families are held against the same rows of it)."""
    D = definition(mode, short_profiles(a), gap, gap_open, short_rows(a))
    D.setflags(write=False)
    return D


def select_bias(mode, gap, gap_open, width_y):
    """The shift the search route gives fit blocks: -(the least fit score) of a profile `width_y` long."""
    return gap_open + gap * width_y if mode == "fit" else 0


def table_low(mode, P, gap, gap_open, x):
    """The least value the recurrence forms for one profile against one token list - an aligned-pair term
    H[i-1][j-1] + P[j][x_i], an E[i][j] or an F[i][j], i, j >= 1 - under the mode's row 0 with NO floor at all (local:
    without its `and 0`): plain Python integers, -inf as None.  The kernels form each of these as a saturating subtraction.
    Returns (that least value, [H[i][L] for i = 0..len x]): the maximum of the list is the fit score, which ties this loop to
    `definition`."""
    e, o, L = int(gap), int(gap_open), len(P)

    def mx(*v):
        v = [t for t in v if t is not None]
        return max(v) if v else None

    H = [0] + [(-(o + j * e) if mode == "fit" else 0) for j in range(1, L + 1)]
    E = [None] * (L + 1)
    low, column = 0, [H[L]]
    for xi in x:
        Hn, F = [0] * (L + 1), None
        for j in range(1, L + 1):
            E[j] = mx(None if E[j] is None else E[j] - e, H[j] - o - e)
            F = mx(None if F is None else F - e, Hn[j - 1] - o - e)
            t = H[j - 1] + int(P[j - 1][xi])
            Hn[j] = mx(t, E[j], F)
            low = min(low, t, E[j], F)
        H = Hn
        column.append(H[L])
    return low, column


def cell_offset(mode, gap, gap_open, width_x, width_y, top):
    """Z of the mode's kernels (prograph_amd/csrc/pg_aln_score.h): a cell holds H + Z, saturating at 0 = -Z."""
    if mode == "local":
        return 0
    if mode == "semiglobal":
        return min(width_x, width_y) * top
    return gap_open + width_y * (gap + top)


# ---------------------------------------------------------------- the strip-mined kernel's length sets
LONG_CASES = (("local", 3, 11), ("semiglobal", 1, 0), ("fit", 2, 5))          # one penalty pair a mode
LONG_SYMS = 21
A_WIDTH, A_ROWS = 131, 64                                        # no multiple of 4, above 128: the long kernel's rows
B_WIDTH, B_ROWS = 37, 24
LENS_A = tuple(int(l) for l in np.random.default_rng(601).permutation(np.arange(1, 258)))     # ONE call: yl = 257, lpad = 384
B_ENDS = tuple(r for nc in range(1, 9) for r in (16 * nc - 15, 16 * nc))      # both ends of every NC of a last strip


def lens_b():
    """s * 128 + r for s = 2..15, two r a strip count, the 16 ends of B_ENDS in turn (so every end occurs, most of them
    twice), and 1024 / 1025 / 2047 / 2048: 3 to 16 strips, every nb 1..8 of the second fill, 32 profiles."""
    lens = [s * 128 + B_ENDS[(2 * k + u) % 16] for k, s in enumerate(range(2, 16)) for u in (0, 1)]
    lens += [1024, 1025, 2047, 2048]
    return tuple(lens[i] for i in np.random.default_rng(603).permutation(len(lens)))


LENS_B = lens_b()
LENS_C = (1, 17, 128)                                            # the long kernel on short operands
# one workgroup, one boundary column: a long profile is followed by a short one, the strip counts differ from row to row
LENS_ONE = (2048, 5, 129, 1, 1025, 128, 300, 16, 513, 17, 257, 640, 127, 385, 256, 2, 33)
ONE_ROWS, ONE_WIDTH = 300, 131


def _rows(seed, a, lens, width, every):
    rng = np.random.default_rng(seed)
    T = rows_of(rng, a, lens, width)
    T[(np.arange(len(T)) % every == 0) & (lengths(T) > 8), 7] = 0          # interior zeros: symbol 0
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def long_rows(which):
    """"A": 64 rows of width 131 with lengths 0..131; "B": 24 of width 37; "one": 300 of width 131, two column tiles."""
    if which == "A":
        rng = np.random.default_rng(610)
        return _rows(611, LONG_SYMS, [0, 1, 131, 130, 128, 129, 127, 4] + list(rng.integers(0, A_WIDTH + 1, A_ROWS - 8)), A_WIDTH, 4)
    if which == "B":
        rng = np.random.default_rng(620)
        return _rows(621, LONG_SYMS, [37, 36, 0, 1, 16, 17] + list(rng.integers(0, B_WIDTH + 1, B_ROWS - 6)), B_WIDTH, 4)
    assert which == "one"
    rng = np.random.default_rng(630)
    return _rows(631, LONG_SYMS, [131, 0, 1, 130] + list(rng.integers(0, ONE_WIDTH + 1, ONE_ROWS - 4)), ONE_WIDTH, 4)


@functools.lru_cache(maxsize=None)
def long_profiles(which):
    lens, seed = {"A": (LENS_A, 641), "B": (LENS_B, 642), "C": (LENS_C, 643), "one": (LENS_ONE, 644)}[which]
    rng = np.random.default_rng(seed)
    out = tuple(random_profile(rng, l, LONG_SYMS) for l in lens)
    for P in out:
        P.setflags(write=False)
    return out


def definition_by_length(mode, profiles, gap, gap_open, X, chunk):
    """`definition` over `chunk` profiles at a time in the order of their lengths, the rows put back in the order given: a
    pass fills its tables to the longest profile of its chunk only."""
    order = np.argsort([len(P) for P in profiles], kind="stable")
    D = np.concatenate([definition(mode, [profiles[k] for k in order[q:q + chunk]], gap, gap_open, X) for q in range(0, len(order), chunk)])
    out = np.empty_like(D)
    out[order] = D
    return out


@functools.lru_cache(maxsize=None)
def long_want(which, mode, gap, gap_open, part=None):
    """The yardstick's matrix of a length set against its rows ("C": against the 134 short rows of 21 symbols); `part` 0 or
    1: of the profiles part::2 alone, half the work."""
    X = short_rows(LONG_SYMS) if which == "C" else long_rows(which)
    profiles = long_profiles(which) if part is None else long_profiles(which)[part::2]
    D = definition_by_length(mode, profiles, gap, gap_open, X, {"A": 43, "B": 32, "C": 3, "one": 4}[which])
    D.setflags(write=False)
    return D


# ---------------------------------------------------------------- the bounds of the 16-bit cells, with max P for max S
def local_cell(width_x, width_y, top):
    return min(width_x, width_y) * top + 255


def semiglobal_cell(width_x, width_y, top):
    return 2 * min(width_x, width_y) * top + 255


def fit_cell(width_y, top, gap, gap_open):
    return gap_open + width_y * (gap + 2 * top) + 255


def matched(rng, length, a, top, other=-4):
    """A profile whose position j scores `top` for one symbol s_j >= 1 and `other` for the rest, and the row s: the row
    scores length * top against it in every mode (nothing is left unaligned)."""
    s = rng.integers(1, a, length)
    P = np.full((length, a), other)
    P[np.arange(length), s] = top
    return P, s
