"""
Inputs and the reference shared by the tests of the Levenshtein kernel beyond 128 positions (CPU and GPU).

Reference (`wagner_fischer_rows`): the Wagner-Fischer table in numpy, row-vectorised - for one text (a Y row) the rows
D[i][.] of all N patterns at once as an (N, LX + 1) table, per text symbol one `minimum` (deletion | substitution or
match) and one `minimum.accumulate` (the insertions of a row: v[j] = j + min_{k <= j} (c[k] - k)).  It shares nothing
with the C oracle, whose `orc_lev_pair` stops at 128 positions, and is pinned in tests/test_levenshtein_long_cpu.py
entry for entry against `lev_testdata.wagner_fischer` (the plain double loop) and against the C oracle on set B.

Long set: `long_x()`, 64 rows of width 2048 with 64 different lengths - every block boundary of the 128-row pattern blocks
and its neighbours up to 2048 - in the families of set B with tokens up to 31; `long_y()`, 13 rows whose lengths are
block and chunk boundaries and their neighbours, the even ones exact copies of the X row of that length (distance 0),
the odd ones prefixes of the parent with substitutions at the boundaries (small distances).  `long_matrix()` is the one
(13, 64) reference every test indexes; what the tests need from the set is asserted from it in the CPU tests.
"""
import numpy as np

from lev_testdata import lengths

REQUIRED = (0, 1, 2, 127, 128, 129, 130, 255, 256, 257, 383, 384, 385, 511, 512, 513, 1023, 1024, 1025, 1535, 1537,
            2046, 2047, 2048)
OTHERS = (3, 5, 17, 31, 32, 33, 63, 64, 65, 96, 100, 126, 131, 192, 200, 254, 258, 300, 320, 350, 382, 386, 400, 448,
          500, 510, 514, 600, 640, 700, 768, 800, 900, 1000, 1022, 1026, 1100, 1280, 1536, 1800)
X_LENS = tuple(sorted(REQUIRED + OTHERS))
Y_LENS = (0, 1, 127, 128, 129, 255, 256, 257, 384, 1024, 1025, 2047, 2048)
EDGES = (127, 128, 255, 256, 1023, 1024)          # 0-based positions of a mutant's edits
FAMILIES = ("homopolymer", "period2", "period3", "parent_piece", "mutant", "prefix", "uniform")
WIDTH = 2048
ALPHABET = "ACDEFGHIKLMNPQRSTVWYBJOUXZabcde"      # 31 letters: token t is letter t - 1

_cache = {}


def strings(T):
    lut = np.array([""] + list(ALPHABET))
    return ["".join(lut[r[r > 0]]) for r in np.asarray(T)]


def wagner_fischer_rows(X, Y):
    """(M, N) int64 edit distances of the rows of Y against the rows of X (zeros are trailing padding)."""
    X, Y = np.atleast_2d(np.asarray(X)).astype(np.int32), np.atleast_2d(np.asarray(Y)).astype(np.int32)
    lx, ly = lengths(X), lengths(Y)
    LX = int(lx.max(initial=0))
    X = X[:, :LX]
    j = np.arange(LX + 1, dtype=np.int32)
    out = np.empty((len(Y), len(X)), dtype=np.int64)
    at = lx[:, None].astype(np.intp)
    for r, y in enumerate(Y):
        v = np.broadcast_to(j, (len(X), LX + 1)).copy()                  # D[0][j] = j
        for i in range(1, int(ly[r]) + 1):
            c = np.empty_like(v)
            c[:, 0] = i
            np.minimum(v[:, 1:] + 1, v[:, :-1] + (X != y[i - 1]), out=c[:, 1:])
            v = np.minimum.accumulate(c - j, axis=1) + j
        out[r] = np.take_along_axis(v, at, 1)[:, 0]
    return out


def parent():
    if "parent" not in _cache:
        p = np.random.default_rng(4096).integers(1, 32, WIDTH)
        p[[0, 127, 128, 255, 256, 1023, 1024, 2047]] = 31, 16, 31, 16, 31, 16, 31, 16
        _cache["parent"] = p
    return _cache["parent"]


def x_layout(r):
    """(length, family, variant) of X row r."""
    return X_LENS[r], FAMILIES[r % len(FAMILIES)], r // len(FAMILIES)


def _mutant(L):
    row = parent()[:L].copy()
    for e in EDGES:
        if e < L:
            row[e] = 1 + row[e] % 31                                     # another token, still in 1..31
    return row


def long_x():
    """(64, 2048) uint8, deterministic; the same (read-only) array on every call."""
    if "x" in _cache:
        return _cache["x"]
    rng = np.random.default_rng(2048)
    p, j = parent(), np.arange(WIDTH)
    T = np.zeros((len(X_LENS), WIDTH), dtype=np.uint8)
    for r in range(len(X_LENS)):
        L, fam, v = x_layout(r)
        if fam == "homopolymer":                                         # Eq all ones: the carry runs through whole blocks
            row = np.full(L, 31)
        elif fam == "period2":                                           # the two phases: a shift of one position
            row = np.array([16, 31])[(j[:L] + v) % 2]
        elif fam == "period3":
            row = np.array([7, 24, 31])[(j[:L] + v) % 3]
        elif fam == "parent_piece":                                      # suffix, middle, prefix of the one parent
            o = (WIDTH - L, (WIDTH - L) // 2, 0)[v % 3]
            row = p[o:o + L]
        elif fam == "mutant":
            row = _mutant(L)
        elif fam == "prefix":
            row = p[:L]
        else:
            row = rng.integers(1, 32, L)
        T[r, :L] = row
    T.setflags(write=False)
    _cache["x"] = T
    return T


def long_y():
    """(13, 2048) uint8: even rows copy the X row of their length, odd rows are the parent's prefix with a substitution
    at every position of EDGES and at the last position."""
    if "y" in _cache:
        return _cache["y"]
    X = long_x()
    T = np.zeros((len(Y_LENS), WIDTH), dtype=np.uint8)
    for i, L in enumerate(Y_LENS):
        if i % 2 == 0:
            T[i] = X[X_LENS.index(L)]
        else:
            row = _mutant(L)
            row[L - 1] = 1 + row[L - 1] % 31
            T[i, :L] = row
    T.setflags(write=False)
    _cache["y"] = T
    return T


def long_matrix():
    """The (13, 64) reference distances of long_y() against long_x(); the same (read-only) array on every call."""
    if "d" not in _cache:
        d = wagner_fischer_rows(long_x(), long_y())
        d.setflags(write=False)
        _cache["d"] = d
    return _cache["d"]


def csr_from_matrix(D, comp, eps, keep_zero=False, wdtype=np.int16):
    keep = comp(D, eps) & ((D >= 0) if keep_zero else (D > 0))
    r, c = np.nonzero(keep)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    return indptr, c.astype(np.int32), D[r, c].astype(wdtype)


def knn_from_matrix(D, k, first, wdtype=np.int16):
    order = np.argsort(D, axis=1, kind="stable")[:, first:first + k]
    return order.astype(np.int32), np.take_along_axis(D, order, 1).astype(wdtype)
