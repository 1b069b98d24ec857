"""
The inputs of the every-length tests of the Levenshtein kernel beyond 128 positions
(tests/test_levenshtein_every_length_cpu.py, tests/test_levenshtein_every_length_gpu.py): rows of every length the kernel
dispatches on, from fixed seeds, and their references from the C oracle's plain Wagner-Fischer (`c_oracle.lev_matrix`,
pinned in the CPU file).  What a length makes the kernel do is computed here from the length alone (`chunks`, `segments`,
`tail`, `blocks`, `instance`, `last_row`) and asserted by the CPU file.  Nothing under prograph_amd/ imports this file;
tests/lev_long_testdata.py and its sets stay as they are.

The sets (tokens 1..31, zero right-padded; the families of the long set in turn, all around the one `LL.parent()`, so that
related rows lie a few edits apart and unrelated ones about as far as their lengths)
    E   one row of every length 0..257, shuffled, so that a wave of 64 columns holds mixed lengths: as patterns every
        position of a dword in the first two blocks and the first row of a third; as texts every tail of a first, a
        second and a third chunk
    T   long texts: one row of 128 c + 32 g + 1 + (7 c + 5 g) % 32 positions for c = 2..15, g = 0..3, and rows of 2047
        and 2048: every chunk count 3..16, every number of segments of the last chunk, every length 1..32 of the last
        segment
    P   long patterns: for every block count b = 3..16 two rows of 128 (b - 1) + r positions, and rows of 2047 and 2048:
        the last row in each of the four dwords of its block, at bit 0, at bit 31 and at odd and even bits between

The references, once per process and read-only: `d_e_ep()` (texts E against patterns E followed by P; `d_ee()` is its
first 258 columns) and `d_t_ep()` (texts T against the same patterns).  Measured on 8 CPU threads: d_ee alone 0.2 s,
d_e_ep 0.5 s, d_t_ep 1.0 s, and about 1 s once for the first call of a process - nothing is thinned.
"""
import functools

import numpy as np

import lev_long_testdata as LL
from lev_testdata import lengths
from oracle import c_oracle as C

BLOCK, SEG = 128, 32               # pattern rows per block = text positions per chunk; text positions per segment
E_WIDTH, WIDTH = 257, 2048
INSTANCES = (1, 2, 4, 8, 16)


# ---------------------------------------------------------------- what a length makes the kernel do
def chunks(la):
    """Chunks of 128 text positions the kernel's outer loop takes for a text of la tokens."""
    return -(-int(la) // BLOCK)


def _last_chunk(la):
    """`cnt` of the last chunk: 1..128 (0: an empty text, no chunk at all)."""
    return int(la) - BLOCK * (chunks(la) - 1) if la else 0


def segments(la):
    """Segments of 32 positions that run in the last chunk (1..4; 0: an empty text)."""
    return -(-_last_chunk(la) // SEG)


def tail(la):
    """Positions of the last segment of the last chunk, the `cnt` segment() is called with there (1..32; 0: empty)."""
    return _last_chunk(la) - SEG * (segments(la) - 1) if la else 0


def blocks(lb):
    """Pattern blocks of 128 rows that hold a row of a pattern of lb tokens (what `nbw` is the wave maximum of)."""
    return -(-int(lb) // BLOCK)


def instance(width):
    """The block count the kernel is instantiated at for a pattern operand of this width."""
    b = blocks(width)
    return next(nb for nb in INSTANCES if b <= nb)


def last_row(lb):
    """(dword, bit) of the last pattern row inside its block, where rows_word() ends (None: an empty pattern)."""
    return (((int(lb) - 1) % BLOCK) // 32, (int(lb) - 1) % 32) if lb else None


# ---------------------------------------------------------------- the lengths
def lens_e():
    return [int(l) for l in np.random.default_rng(601).permutation(E_WIDTH + 1)]


def t_length(c, g):
    return BLOCK * c + SEG * g + 1 + (7 * c + 5 * g) % 32


def lens_t():
    lens = [t_length(c, g) for c in range(2, 16) for g in range(4)] + [2047, 2048]
    return [lens[i] for i in np.random.default_rng(602).permutation(len(lens))]


P_BITS = (1, 32, 2, 7, 16, 21, 30)   # the last row's place 1..32 in its dword: both ends, odd and even ones between


def p_rows():
    """(blocks b, r) of the 28 formula rows of P: row i has b = 3 + i // 2 and its last row in dword (i + i // 4) % 4,
    so that every (dword, place) occurs once and the two rows of a block count lie in different dwords."""
    return [(3 + i // 2, 32 * ((i + i // 4) % 4) + P_BITS[i // 4]) for i in range(28)]


def lens_p():
    return [BLOCK * (b - 1) + r for b, r in p_rows()] + [2047, 2048]


# ---------------------------------------------------------------- the rows
def _indel(L):
    """The parent's prefix after a deletion at 100 and an insertion in the middle: L tokens again, everything between
    the two shifted by one position (a run of negative then positive deltas across the block boundaries)."""
    p = LL.parent()
    if L < 260:
        return LL._mutant(L)
    row = list(p[:L + 1])
    del row[100]
    row.insert(L // 2, 1 + int(p[L // 2]) % 31)
    return np.array(row[:L])


def _row(rng, L, fam, v):
    p, j = LL.parent(), np.arange(L)
    if fam == "homopolymer":                                         # Eq all ones: the carry runs through whole blocks
        return np.full(L, 31)
    if fam == "period2":                                             # the two phases: a shift of one position
        return np.array([16, 31])[(j + v) % 2]
    if fam == "period3":
        return np.array([7, 24, 31])[(j + v) % 3]
    if fam == "parent_piece":                                        # suffix, middle, a piece from 100 on
        o = (LL.WIDTH - L, (LL.WIDTH - L) // 2, min(100, LL.WIDTH - L))[v % 3]
        return p[o:o + L]
    if fam == "mutant":                                              # substitutions at the block boundaries | an indel pair
        return LL._mutant(L) if v % 2 == 0 else _indel(L)
    if fam == "prefix":
        return p[:L]
    return rng.integers(1, 32, L)


def _rows(seed, lens, width, families):
    rng = np.random.default_rng(seed)
    T = np.zeros((len(lens), width), dtype=np.uint8)
    for r, L in enumerate(lens):
        T[r, :L] = _row(rng, L, families[r % len(families)], r // len(families))
    assert np.array_equal(lengths(T), lens)
    T.setflags(write=False)
    return T


T_FAMILIES = ("prefix", "mutant")
P_FAMILIES = ("prefix", "mutant", "parent_piece", "period3", "mutant", "homopolymer", "prefix")


@functools.lru_cache(maxsize=None)
def set_e():
    """(258, 257) uint8: row r has lens_e()[r] tokens of family LL.FAMILIES[r % 7]; read-only."""
    return _rows(611, lens_e(), E_WIDTH, LL.FAMILIES)


@functools.lru_cache(maxsize=None)
def set_t():
    """(58, 2048) uint8: prefixes and mutants of the parent; read-only."""
    return _rows(612, lens_t(), WIDTH, T_FAMILIES)


@functools.lru_cache(maxsize=None)
def set_p():
    """(30, 2048) uint8; read-only."""
    return _rows(613, lens_p(), WIDTH, P_FAMILIES)


def at_width(T, width):
    """The rows of T that fit `width`, at that width (cut or zero-padded), and their row numbers in T."""
    T = np.asarray(T)
    rows = np.nonzero(lengths(T) <= width)[0]
    out = np.zeros((len(rows), width), dtype=np.uint8)
    w = min(width, T.shape[1])
    out[:, :w] = T[rows, :w]
    return out, rows


@functools.lru_cache(maxsize=None)
def set_ep():
    """E followed by P at width 2048: the pattern operand of the references, (288, 2048); read-only."""
    EP = np.concatenate([at_width(set_e(), WIDTH)[0], set_p()])
    EP.setflags(write=False)
    return EP


def lens_ep():
    return lens_e() + lens_p()


# ---------------------------------------------------------------- the references
@functools.lru_cache(maxsize=None)
def d_e_ep():
    """(258, 288) int64: texts E against patterns E followed by P; read-only."""
    D = C.lev_matrix(set_ep(), set_e())
    D.setflags(write=False)
    return D


def d_ee():
    """(258, 258): texts E against patterns E (a view of d_e_ep())."""
    return d_e_ep()[:, :len(set_e())]


@functools.lru_cache(maxsize=None)
def d_t_ep():
    """(58, 288) int64: texts T against patterns E followed by P; read-only."""
    D = C.lev_matrix(set_ep(), set_t())
    D.setflags(write=False)
    return D


def long_lane_columns(nb):
    """Columns of set_ep() for the pattern operand of instance nb in which every wave of 64 columns holds a pattern whose
    last row lies in the instance's top block: the columns of E in order, the rows of P that fit 128 nb positions spread
    among them, and in every wave one of the rows of P of exactly nb blocks (taken in turn, at a lane that moves)."""
    ne, lp = len(lens_e()), lens_p()
    top = [ne + i for i, l in enumerate(lp) if blocks(l) == nb]
    rest = [ne + i for i, l in enumerate(lp) if blocks(l) < nb]
    assert top
    cols = list(range(ne))
    for i, c in enumerate(rest):                                     # the shorter rows of P: anywhere
        cols.insert((i * 37 + 11) % len(cols), c)
    n_waves = -(-len(cols) // 63)                                    # 63 of these columns and one long lane per wave
    out = []
    for w in range(n_waves):
        part = cols[63 * w:63 * (w + 1)]
        part.insert((w * 23 + 5) % (len(part) + 1), top[w % len(top)])
        out += part
    assert sorted(set(out) - set(top)) == sorted(cols)
    return np.array(out)
