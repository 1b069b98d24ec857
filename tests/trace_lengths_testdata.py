"""
The inputs of the per-pair alignment length tests (tests/test_alignment_trace_lengths_cpu.py, ..._gpu.py): the traceback
kernels (pg_alignment_trace, pg_alignment_trace_long, their fit entries) and the statistics kernel (pg_alignment_stats) at
every length, every operand width, every strip count and the extremes of the count words, all from fixed seeds.  The
yardstick is `oracle.c_oracle.align_trace` (orc_align_trace), which the CPU file pins to trace_testdata.definition and
fit_testdata.canonical.  What the lengths cover is computed here from the lengths alone (`nd`, `yg`, `stats_instance`,
`strips`, `tail_dwords`) and asserted by the CPU file.  Nothing under prograph_amd/ imports this file.

The sets (uint8, zero right-padded, six symbols 0..5; a row never ends in symbol 0)
    YS   one row of every length 0..128, shuffled, width 128; every fifth row has interior zeros
    XS   64 rows at width 128: lengths 0, 1, 15, 16, 17, 63, 64, 65, 127, 128 and random ones; half of them cut from rows
         of YS with a symbol changed and a symbol dropped, so that alignments are long and have real gaps
    XN   64 rows at width 47: lengths 0, 1, 47 and random ones, half of them related to YS likewise
    YL   one row of every length of aln_lengths_testdata.lens_b() (strip counts 3..16, every tail) and of 0, 1, 127, 128,
         129, 255, 256, 257, width 2048, shuffled: the 64 lanes of a wave differ in their strip counts
    XL   64 rows of 64 different lengths in 1..199, width 199, half of them cut from the rows B_MANY of YL
    EXTREMES   the hand-built pairs that drive a field of a count word to 128 and fill a row of ops
"""
import functools

import numpy as np

import aln_lengths_testdata as L
from trace_testdata import GLOBAL, LOCAL, SEMIGLOBAL

FIT = 3
MODES = (GLOBAL, LOCAL, SEMIGLOBAL, FIT)
A = 6
EXTREME = "extreme"
GAPS = ((2, 0), (2, 11))            # (gap, gap_open) with the small-entry tables
GAPS_EXTREME = (255, 255)           # with the extreme tables
STRIP = 128
B_MANY = L.B_MANY


def table(mode, kind=None):
    """Six symbols and small entries, so that ties abound (the tables of tests/test_alignment_stats_gpu.py; fit has a
    score table of its own seed).  EXTREME: cost 255 off the diagonal; scores 127 and -128."""
    rng = np.random.default_rng(11 + mode)
    if kind == EXTREME:
        return (255 * (1 - np.eye(A, dtype=np.int64))) if mode == GLOBAL else np.where(np.eye(A, dtype=bool), 127, -128)
    if mode == GLOBAL:
        T = rng.integers(1, 4, (A, A))
        return np.triu(T, 1) + np.triu(T, 1).T
    T = rng.integers(-3, 2, (A, A))
    T = np.triu(T) + np.triu(T, 1).T
    T[np.arange(A), np.arange(A)] = rng.integers(1, 5, A)
    T[0, 1] = T[1, 0] = 2                                                   # S[a][0] > 0: padding must not pair
    return T


# ---------------------------------------------------------------- what a length or a width makes a kernel do
def lengths(T):
    """Index of the last non-zero + 1 per row."""
    T = np.atleast_2d(np.asarray(T))
    return np.where(T != 0, np.arange(1, T.shape[1] + 1), 0).max(axis=1, initial=0)


def nd(yl):
    """Direction dwords per row of the workspace: eight cells of a y operand of WIDTH yl to a dword."""
    return -(-int(yl) // 8)


def yg(yl):
    """Token dwords of a y operand of width yl that the kernels stage."""
    return -(-int(yl) // 4)


def stats_instance(yl):
    """YMAX of the pg_alignment_stats instance that a y operand of width yl runs."""
    return 32 if yl <= 32 else 64 if yl <= 64 else 128


def strips(l):
    """Strips of 128 columns that a y row of l symbols runs in the long tracer (0: an empty row runs none)."""
    return -(-int(l) // STRIP)


def tail_dwords(l):
    """Direction dwords of the last strip of a y row of l symbols: 1..16 (0: an empty row)."""
    l = int(l)
    return -(-(l - STRIP * (strips(l) - 1)) // 8) if l else 0


# ---------------------------------------------------------------- the rows
def _rows(rng, lens, width):
    T = np.zeros((len(lens), width), dtype=np.uint8)
    for r, l in enumerate(lens):
        T[r, :l] = rng.integers(1, A, l)
    return T


def _interior_zeros(rng, T, every):
    lens = lengths(T)
    for r in range(0, len(T), every):
        if lens[r] >= 3:
            T[r, rng.integers(0, lens[r] - 1, max(1, lens[r] // 40))] = 0
    assert np.array_equal(lengths(T), lens)


def _relate(rng, X, rows, Y):
    """Rows `rows` of X become pieces of rows of Y at least as long, one symbol changed and one dropped, their lengths kept."""
    ly = lengths(Y)
    for r in rows:
        l = int(lengths(X[r:r + 1])[0])
        longer = np.flatnonzero(ly >= l + 1)
        if l < 4 or not len(longer):
            continue
        src = Y[int(rng.choice(longer))]
        p = int(rng.integers(0, int(lengths(src[None])[0]) - l))
        piece = np.delete(src[p:p + l + 1], int(rng.integers(1, l)))        # one symbol of the source dropped: a real gap
        piece[int(rng.integers(0, l - 1))] = rng.integers(1, A)
        if piece[-1] == 0:
            piece[-1] = A - 1
        X[r, :l] = piece
    return X


def lens_ys():
    return [int(l) for l in np.random.default_rng(601).permutation(129)]


def lens_xs():
    return [0, 1, 15, 16, 17, 63, 64, 65, 127, 128] + [int(l) for l in np.random.default_rng(602).integers(0, 129, 54)]


def lens_xn():
    return [0, 1, 47] + [int(l) for l in np.random.default_rng(603).integers(0, 48, 61)]


LONG_EDGES = (0, 1, 127, 128, 129, 255, 256, 257)


def lens_yl():
    lens = sorted(set(L.lens_b()) | set(LONG_EDGES))
    return [lens[i] for i in np.random.default_rng(604).permutation(len(lens))]


def lens_xl():
    return L.lens_x199()


@functools.lru_cache(maxsize=None)
def _sets():
    rng = np.random.default_rng(610)
    ys = _rows(rng, lens_ys(), 128)
    _interior_zeros(rng, ys, 5)
    xs = _relate(rng, _rows(rng, lens_xs(), 128), range(10, 64, 2), ys)
    xs = xs[np.random.default_rng(611).permutation(64)]
    xn = _relate(rng, _rows(rng, lens_xn(), 47), range(3, 64, 2), ys)
    xn = xn[np.random.default_rng(612).permutation(64)]
    yl = _rows(rng, lens_yl(), 2048)
    _interior_zeros(rng, yl, 5)
    many = yl[[lens_yl().index(l) for l in B_MANY]]
    xl = _relate(rng, _rows(rng, lens_xl(), 199), range(0, 64, 2), many)
    out = dict(YS=ys, XS=xs, XN=xn, YL=yl, XL=xl, B_MANY=many.copy())
    for v in out.values():
        v.setflags(write=False)
    return out


def rows(name):
    """YS, XS, XN, YL, XL or B_MANY (the eight rows of YL of the lengths B_MANY): generated once per process, read-only."""
    return _sets()[name]


# ---------------------------------------------------------------- pair lists
def product(ny, nx, seed):
    """Every pair (y row, x row) of ny x nx rows in a shuffled order: (yi, xi)."""
    p = np.random.default_rng(seed).permutation(ny * nx)
    return (p // nx).astype(np.int32), (p % nx).astype(np.int32)


def lanes_first(ny, nx):
    """Every pair of ny x nx rows with the y row changing fastest: the 64 lanes of a wave hold 64 different y rows."""
    p = np.arange(ny * nx)
    return (p % ny).astype(np.int32), (p // ny).astype(np.int32)


def width_rows(w):
    """(rows of YS, rows of XN) of the operand width w = 1..128 (test B): 16 rows of YS - the empty one, rows whose cut to w
    symbols reaches into the last token dword and the last direction dword of the width, the full width, shorter ones -
    and 8 rows of XN, the empty one, the shortest and the widest among them: 128 pairs."""
    rng = np.random.default_rng(700 + w)
    ly, lx = np.array(lens_ys()), lengths(rows("XN"))
    want = [0, w, min(w + 1, 128), 128, 4 * ((w - 1) // 4) + 1, 8 * ((w - 1) // 8) + 1, max(w - 1, 0), w // 2]
    want += [int(v) for v in rng.integers(0, w + 1, 8)] + [int(v) for v in rng.permutation(129)]   # longer rows are cut to w
    picked = list(dict.fromkeys(int(np.flatnonzero(ly == l)[0]) for l in want))[:16]
    xr = [int(np.flatnonzero(lx == l)[0]) for l in (0, 1, 47)]
    xr += [int(v) for v in rng.permutation(np.setdiff1d(np.arange(64), xr))[:5]]
    return np.array(picked), np.array(xr)


# ---------------------------------------------------------------- the extremes of test C
def _pad(seq, width=128):
    row = np.zeros(width, dtype=np.uint8)
    row[:len(seq)] = seq
    return row


@functools.lru_cache(maxsize=None)
def extremes():
    """The hand-built pairs at widths 128 x 128: a list of dicts name, mode, table, gap, gap_open, x, y (rows of 128) and
    `expect`, the closed-form fields {field: value} that the test asserts beside the oracle's answer; x_gaps / y_gaps /
    pairs are counted from the ops."""
    rng = np.random.default_rng(620)
    full = rng.integers(1, A, 128).astype(np.uint8)
    empty = np.zeros(128, dtype=np.uint8)
    lo, hi = rng.integers(1, 3, 128).astype(np.uint8), rng.integers(3, 5, 128).astype(np.uint8)        # disjoint alphabets
    motif = rng.integers(1, 4, 64).astype(np.uint8)
    out = []

    def add(name, mode, kind, gap, gap_open, x, y, **expect):
        out.append(dict(name=name, mode=mode, table=table(mode, kind), gap=gap, gap_open=gap_open, x=_pad(x), y=_pad(y),
                        expect=expect))
    for mode in MODES:                                                      # identical rows of 128
        S = table(mode)
        score = 0 if mode == GLOBAL else int(S[full, full].sum())
        add(f"identical {mode}", mode, None, 2, 11, full, full, score=score, x_begin=0, x_end=128, y_begin=0, y_end=128,
            n_ops=128, identities=128, pairs=128, x_gaps=0, y_gaps=0)
    add("global full x, empty y", GLOBAL, None, 2, 11, full, empty, score=11 + 256, x_begin=0, x_end=128, y_begin=0, y_end=0,
        n_ops=128, identities=0, pairs=0, x_gaps=128, y_gaps=0)
    add("global empty x, full y", GLOBAL, None, 2, 11, empty, full, score=11 + 256, x_begin=0, x_end=0, y_begin=0, y_end=128,
        n_ops=128, identities=0, pairs=0, x_gaps=0, y_gaps=128)
    add("fit empty x, full y", FIT, None, 2, 11, empty, full, score=-(11 + 256), x_begin=0, x_end=0, y_begin=0, y_end=128,
        n_ops=128, identities=0, pairs=0, x_gaps=0, y_gaps=128)
    add("fit full x, empty y", FIT, None, 2, 11, full, empty, score=0, x_begin=0, x_end=0, y_begin=0, y_end=0,
        n_ops=0, identities=0, pairs=0, x_gaps=0, y_gaps=0)
    for gap_open in (0, 255):                                               # all 256 columns are gaps: ops has no zero tail
        add(f"disjoint, cost 255, gap_open {gap_open}", GLOBAL, EXTREME, 1, gap_open, lo, hi, score=256 + 2 * gap_open,
            x_begin=0, x_end=128, y_begin=0, y_end=128, n_ops=256, identities=0, pairs=0, x_gaps=128, y_gaps=128)
    add("local 128 matches at 127", LOCAL, EXTREME, 255, 255, full, full, score=128 * 127, x_begin=0, x_end=128, y_begin=0,
        y_end=128, n_ops=128, identities=128, pairs=128, x_gaps=0, y_gaps=0)
    add("semi-global suffix / prefix overlap", SEMIGLOBAL, EXTREME, 2, 11, np.concatenate([np.full(64, 5), motif]),
        np.concatenate([motif, np.full(64, 4)]), score=64 * 127, x_begin=64, x_end=128, y_begin=0, y_end=64, n_ops=64,
        identities=64, pairs=64, x_gaps=0, y_gaps=0)
    add("fit y of 128 equal to x", FIT, EXTREME, 255, 255, full, full, score=128 * 127, x_begin=0, x_end=128, y_begin=0,
        y_end=128, n_ops=128, identities=128, pairs=128, x_gaps=0, y_gaps=0)
    return out


# ---------------------------------------------------------------- the cross-strip tie of test E
TIE_M, TIE_N = [1, 2] * 4, [3, 4] * 4
TIE_X = TIE_N + [5] * 20 + TIE_M                                            # 36 symbols


def tie_table():
    """2 on the diagonal of symbols 0..4, -3 elsewhere: the filler 5 matches nothing, itself included."""
    S = np.full((A, A), -3)
    S[np.arange(5), np.arange(5)] = 2
    return S


def tie_ends():
    """Where the second motif ends in y: for every seam s = 1..15 the column 128 s exactly (the last of strip s - 1), 128 s + 1
    (the first of strip s) and one inside strip s."""
    return [e for s in range(1, 16) for e in (128 * s, 128 * s + 1, 128 * s + 9 + (37 * s) % 100)]


def tie_rows():
    """(X, Y) of the construction of test_the_cross_strip_tie (tests/test_alignment_trace_long_gpu.py): x = N filler M, one
    row; y = M filler N with N ending at each column of tie_ends(), width 2048.  M pairs with M at the cells up to
    (36, 8) and N with N up to (8, end), 16 either way; the canonical end cell is the one of the smaller i."""
    ends = tie_ends()
    Y = np.zeros((len(ends), 2048), dtype=np.uint8)
    for r, end in enumerate(ends):
        y = TIE_M + [5] * (end - 16) + TIE_N
        Y[r, :len(y)] = y
    return np.array([TIE_X], dtype=np.uint8), Y
