"""
The inputs of the alignment length tests (tests/test_alignment_lengths_cpu.py, tests/test_alignment_lengths_gpu.py): Y rows
of every length the kernels dispatch on, X operands at widths that are no multiple of 4, the tables and the penalties,
all from fixed seeds.  What the lengths cover is computed here from the lengths alone (`strips`, `last_nc`, `select_pos`,
`fills`) and asserted by the CPU file.  The yardsticks are the suite's own: long_testdata.definition (global),
local_testdata.definition, semiglobal_testdata.definition.  Nothing under prograph_amd/ imports this file.

The Y sets
    S   one row of every length 0..128, shuffled: the kernels up to 128 positions, every NC = ceil(len y / 16) and every
        position of the select chain
    A   one row of every length 0..256, shuffled: the same in strip 0 and in a second, last strip
    B   for every strip index s = 2..15 of the last strip and every nc = 0..7 one row of
        128 s + 16 nc + 1 + (5 s + 3 nc) % 16 positions, and rows of 2047 and 2048, shuffled: every strip count 3..16
        with every NC of the last strip, all 16 select positions, the second profile fill with every nb = 1..8
"""
import functools

import numpy as np

import local_testdata
import long_testdata
import semiglobal_testdata
from local_testdata import score_table
from long_testdata import cost_table, lengths, rows_of

SYMS = 21
XW, XSW = 47, 128                  # the widths of the two X operands; 47 is no multiple of 4
GAPS = ((1, 0), (3, 11))           # (gap, gap_open) everywhere
STRIP, CHUNK, SLOTS = 128, 16, 8   # positions per strip, cells per chunk of the row routine, profile slots in LDS
MODES = ("global", "local", "semiglobal")
DEFINITION = {"global": long_testdata.definition, "local": local_testdata.definition,
              "semiglobal": semiglobal_testdata.definition}


# ---------------------------------------------------------------- what a length makes a kernel do
def strips(l):
    """Strips of 128 positions that hold a position of a row of l symbols."""
    return -(-int(l) // STRIP)


def last_nc(l):
    """NC of the last strip: the template instance the switch picks (0: no strip at all)."""
    l = int(l)
    return -(-(l - STRIP * (strips(l) - 1)) // CHUNK) if l else 0


def select_pos(l):
    """The position 1..16 of len y inside its chunk: which of the 16 selects is the answer (0: an empty row)."""
    return (int(l) - 1) % CHUNK + 1 if l else 0


def fills(l):
    """nb of every profile fill of a row of l symbols: its strips in groups of eight slots."""
    return [min(SLOTS, strips(l) - s0) for s0 in range(0, strips(l), SLOTS)]


# ---------------------------------------------------------------- the lengths
def lens_s():
    return [int(l) for l in np.random.default_rng(501).permutation(129)]


def lens_a():
    return [int(l) for l in np.random.default_rng(502).permutation(257)]


def b_length(s, nc):
    return 128 * s + 16 * nc + 1 + (5 * s + 3 * nc) % 16


def lens_b():
    lens = [b_length(s, nc) for s in range(2, 16) for nc in range(8)] + [2047, 2048]
    return [lens[i] for i in np.random.default_rng(503).permutation(len(lens))]


def lens_x47():
    return [int(l) for l in np.random.default_rng(504).integers(0, XW + 1, 64)] + [47, 1, 0, 33, 16, 17]


def lens_x128():
    return [int(l) for l in np.random.default_rng(505).integers(0, XSW + 1, 124)] + [128, 127, 0, 1, 16, 17]


def lens_x199():
    """64 lanes of 64 different lengths in 1..200 (the test of both operands long): the longest is 199, the width."""
    lens = [int(l) for l in np.random.default_rng(506).permutation(np.arange(2, 199))[:62]] + [199, 1]
    return [lens[i] for i in np.random.default_rng(507).permutation(64)]


B_MANY = [b_length(s, nc) for s, nc in ((4, 0), (4, 5), (8, 1), (8, 6), (11, 2), (11, 7), (15, 3), (15, 4))]


# ---------------------------------------------------------------- the rows
def _interior_zeros(rng, T, every):
    """Symbol 0 inside some rows (never the last symbol, so no length changes)."""
    lens = lengths(T)
    for r in range(0, len(T), every):
        if lens[r] >= 3:
            T[r, rng.integers(0, lens[r] - 1, max(1, lens[r] // 40))] = 0
    assert np.array_equal(lengths(T), lens)


def _rows(seed, lens, width, every):
    rng = np.random.default_rng(seed)
    T = rows_of(rng, SYMS, lens, width)
    _interior_zeros(rng, T, every)
    return T


Y_SETS = {"S": (lens_s, 511), "A": (lens_a, 512), "B": (lens_b, 513)}


def generate_y(name):
    """Set S, A or B, generated anew."""
    lens, seed = Y_SETS[name]
    lens = lens()
    return _rows(seed, lens, max(lens), 5)


@functools.lru_cache(maxsize=None)
def y(name):
    """Set S, A or B: generated once per process, read-only."""
    T = generate_y(name)
    T.setflags(write=False)
    return T


def row_of_length(Y, l):
    r = np.nonzero(lengths(Y) == l)[0]
    assert len(r) == 1
    return int(r[0])


# kinds of a related column: x is a piece of the row (across a seam where the row has one), x is the row's beginning, x is
# the row's end, x begins as the row ends and goes on with symbols of its own
PIECE, BEGINNING, END, OVERLAP = range(4)


def _relate(X, c, kind, y):
    """Make column c of X related to the sequence y (a row without its padding), keeping len x; returns the number of
    symbols taken from y."""
    lx, ly = int(lengths(X)[c]), len(y)
    l = min(lx, ly) if kind != OVERLAP else min(lx, ly) // 2
    assert l >= 2
    if kind == PIECE:
        seam = SLOTS * STRIP if ly > SLOTS * STRIP + l else STRIP if ly > STRIP + l else ly // 2
        p = min(max(0, seam - l // 2), ly - l)
        X[c, :l] = y[p:p + l]
    elif kind == BEGINNING:
        X[c, :l] = y[:l]
    else:
        X[c, :l] = y[ly - l:]
    if l == lx and X[c, l - 1] == 0:
        X[c, l - 1] = SYMS - 1                                    # the last symbol is never 0, as in rows_of
    assert int(lengths(X)[c]) == lx
    return l


# The X operands: (seed, lengths, width) and the related columns as (column, kind, Y set, length of the Y row).  x47 and
# x128 relate their fixed last columns and some of their longest random ones, x199 its longest random ones.
X_OPERANDS = {"x47": (521, lens_x47, XW), "x128": (522, lens_x128, XSW), "x199": (523, lens_x199, 199)}
RELATED = {
    "x47": [(64, PIECE, "A", 256), (67, BEGINNING, "A", 200), (69, END, "A", 129), (68, END, "A", 77),
            (11, PIECE, "B", 2048), (12, BEGINNING, "B", 2047), (15, END, "B", 2048), (37, OVERLAP, "B", 2047),
            (9, OVERLAP, "A", 255), (0, OVERLAP, "A", 144), (19, PIECE, "A", 31)],
    "x128": [(124, PIECE, "S", 128), (125, BEGINNING, "S", 127), (7, END, "S", 128), (87, OVERLAP, "S", 113),
             (113, PIECE, "S", 97), (23, END, "S", 81), (45, OVERLAP, "S", 65), (94, BEGINNING, "S", 49),
             (118, END, "S", 33), (18, OVERLAP, "S", 100)],
    "x199": [(c, kind, "B", l)
             for c, kind, l in zip((33, 30, 15, 10, 58, 55, 27, 32), (PIECE, BEGINNING, END, OVERLAP) * 2, B_MANY)],
}


def generate_x(name):
    """(X, related), generated anew: `related` lists (column, kind, Y set, row, symbols taken) of the related columns."""
    seed, lens, width = X_OPERANDS[name]
    X = _rows(seed, lens(), width, 4)
    related = []
    for c, kind, which, l in RELATED[name]:
        Y = y(which)
        r = row_of_length(Y, l)
        related.append((c, kind, which, r, _relate(X, c, kind, Y[r, :l])))
    return X, tuple(related)


@functools.lru_cache(maxsize=None)
def _x(name):
    X, related = generate_x(name)
    X.setflags(write=False)
    return X, related


def x(name):
    """The X operand x47, x128 or x199: generated once per process, read-only."""
    return _x(name)[0]


def related(name):
    return _x(name)[1]


def y_many():
    """Eight rows of set B, one per NC of the last strip, of 5, 9, 12 and 16 strips."""
    Y = y("B")
    return Y[[row_of_length(Y, l) for l in B_MANY]]


# ---------------------------------------------------------------- tables and penalties
def score():
    S = score_table(np.random.default_rng(531), SYMS, -9, 6, diag=np.arange(2, 12))
    S[0, :] = S[:, 0] = 5                                         # padding would score if it were let in
    return S


def cost(top):
    return cost_table(np.random.default_rng(540 + top), SYMS, top)


def table_of(mode, top=None):
    return cost(top) if mode == "global" else score()


# (mode, gap, gap_open, largest cost of the global table) per set.  S: costs up to 15 keep every distance within 2048,
# where fp16 is exact (128 * 15 + 11); (255, 255) with costs up to 255 is the 16-bit edge of the kernels up to 128
# positions.  A: 256 * 215 + 2 * 255 + 2 * 215 <= 65 535.  B: 2048 * 31 + 2 * 11 + 2 * 3 <= 65 535, 32 is outside.
SCORES = [(m, e, o, None) for m in ("local", "semiglobal") for e, o in GAPS]
CASES_S = ([("global", e, o, 15) for e, o in GAPS] + [("global", 255, 255, 255)] + SCORES
           + [(m, 255, 255, None) for m in ("local", "semiglobal")])
LINEAR_S = [(1, 15), (3, 15), (255, 255)]                         # (gap, largest cost) of pg_alignment_dense
CASES_A = [("global", e, o, 215) for e, o in GAPS] + [("global", 215, 255, 215)] + SCORES
CASES_B = [("global", e, o, 31) for e, o in GAPS] + SCORES
CASES_MANY = [("global", 3, 11, 31), ("local", 3, 11, None), ("semiglobal", 3, 11, None)]


@functools.lru_cache(maxsize=None)
def want(which, mode, gap, gap_open, top):
    """The yardstick's (rows of the Y set, columns of its X operand) matrix, computed once per process and read-only."""
    xn, yn = {"S": ("x128", "S"), "A": ("x47", "A"), "B": ("x47", "B"), "many": ("x199", None)}[which]
    X, Y = x(xn), (y(yn) if yn else y_many())
    D = DEFINITION[mode](table_of(mode, top), gap, gap_open, X, Y)
    D.setflags(write=False)
    return D
