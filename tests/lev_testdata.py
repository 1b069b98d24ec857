"""
Inputs and oracle-side references shared by the Levenshtein tests (CPU and GPU).

Set A: 1000 clustered variable-length rows (lengths 96..128, clusters of 50) plus 60 unrelated rows (uniform tokens
1..20, lengths 40..128), permuted.  Properties the tests rely on - and assert from the oracle's results, so that a
changed generator cannot make them vacuous: for k = 16 most rows have their 16th neighbour within 8 edits and the
unrelated ones do not; duplicates occur; no row has 63 neighbours within 8 edits.

Set B (`set_b`): 441 rows of width 128 whose lengths walk through `LENS` - every dword boundary of the 128-bit pattern
and its two neighbours - in interleaved families with small, structured distances and tokens up to 31.  What the GPU
tests need from it is asserted from the references alone in tests/test_levenshtein_lengths_cpu.py.
`wagner_fischer` is the second reference: the textbook recurrence in numpy, independent of the C oracle.
"""
import ctypes
import operator

import numpy as np

from oracle import c_oracle as C
from prograph_amd import synth


def set_a():
    tok, _ = synth.clustered_varlen_tokens(1000, Lmax=128, Lmin=96, members=50)
    rng = np.random.default_rng(7)
    extra = np.zeros((60, 128), dtype=np.uint8)
    for i in range(60):
        l = int(rng.integers(40, 129))
        extra[i, :l] = rng.integers(1, 21, l)
    T = np.concatenate([tok, extra])
    return np.ascontiguousarray(T[rng.permutation(len(T))])


def pair_matrix(X, Y):
    """(M, N) unbanded distances from the C oracle, pair by pair."""
    return np.array([[C.lev_pair(y, x, 128) for x in X] for y in Y], dtype=np.int64)


def csr_from_banded(T, comp, eps):
    """The epsilon graph (0 < d, comp(d, eps)), eps <= 8, from the oracle's banded kNN lists: complete because no row has
    a 63rd rank within the band (asserted)."""
    idx, d = C.lev_knn(T, 63, band=8)
    assert (d[:, 62] > 8).all(), "a row has 63 in-band neighbours: the lists are not the whole neighbourhood"
    indptr, cols, wts = [0], [], []
    for i in range(len(T)):
        keep = (d[i] <= 8) & (d[i] > 0) & comp(d[i].astype(np.int64), eps)
        o = np.argsort(idx[i][keep], kind="stable")
        cols.append(idx[i][keep][o]); wts.append(d[i][keep][o])
        indptr.append(indptr[-1] + int(keep.sum()))
    return np.array(indptr, dtype=np.int64), np.concatenate(cols).astype(np.int32), np.concatenate(wts).astype(np.uint8)


def csr_from_matrix(D, comp, eps, keep_zero=False):
    keep = comp(D, eps) & ((D >= 0) if keep_zero else (D > 0))
    r, c = np.nonzero(keep)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    return indptr, c.astype(np.int32), D[r, c].astype(np.uint8)


def knn_from_matrix(D, k, first):
    order = np.argsort(D, axis=1, kind="stable")[:, first:first + k]
    return order.astype(np.int32), np.take_along_axis(D, order, 1).astype(np.uint8)


# ---------------------------------------------------------------- set B
LENS = (0, 1, 2, 7, 8, 9, 30, 31, 32, 33, 34, 62, 63, 64, 65, 66, 95, 96, 97, 127, 128)
EDGES = (31, 32, 33, 63, 64, 65, 95, 96)      # 0-based positions around the dword boundaries: a mutant has an edit there
MUTANT_PARENTS = (33, 64, 65, 96, 128)
FAMILIES = ("homopolymer", "period2", "period3", "parent_piece", "mutant", "duplicate", "uniform")
B_BLOCKS = 21                                  # 21 blocks of len(LENS) rows: every (family, length) three times

_set_b = None


def set_b_layout(r):
    """(length, family, variant) of row r: length LENS[r % 21], so that any 21 consecutive rows hold every length; the
    family moves on by one with every row and every block, so that each family takes each length once in 7 blocks."""
    b, i = divmod(r, len(LENS))
    return LENS[i], FAMILIES[(b + i) % len(FAMILIES)], b // len(FAMILIES)


def _mutant(rng, parent, L, variant):
    """`parent[:p]`, p the variant-th of MUTANT_PARENTS within 3 of L, after 1..9 edits that leave L tokens: the |L - p|
    deletions or insertions the length needs plus substitutions, the first edit at a position of EDGES."""
    ps = [p for p in MUTANT_PARENTS if abs(p - L) <= 3]
    if not ps:                                                    # the short lengths: a prefix with one substitution
        row = list(parent[:L])
        if L:
            row[L // 2] = 1 + row[L // 2] % 31
        return row, 0, []
    p = ps[variant % len(ps)]
    row, net = list(parent[:p]), L - p
    kinds = ["del"] * -net + ["ins"] * net                        # deletions first: the row never outgrows 128
    kinds += ["sub"] * int(rng.integers(0 if kinds else 1, 10 - len(kinds)))
    assert 1 <= len(kinds) <= 9
    at = []
    for e, kind in enumerate(kinds):
        pos = int(rng.choice([q for q in EDGES if q < len(row)])) if e == 0 else int(rng.integers(0, len(row)))
        at.append(pos)
        if kind == "del":
            del row[pos]
        elif kind == "ins":
            row.insert(pos, int(rng.integers(1, 32)))
        else:
            row[pos] = 1 + row[pos] % 31                          # another token, still in 1..31
    assert len(row) == L
    return row, p, at


def set_b():
    """(441, 128) uint8, deterministic; the same (read-only) array on every call."""
    global _set_b
    if _set_b is not None:
        return _set_b
    rng = np.random.default_rng(2024)
    parent = rng.integers(1, 32, 128)
    parent[[0, 31, 32, 64, 96, 127]] = 31, 16, 31, 16, 31, 16
    n = B_BLOCKS * len(LENS)
    T = np.zeros((n, 128), dtype=np.uint8)
    j = np.arange(128)
    for r in range(n):
        L, fam, v = set_b_layout(r)
        if fam == "homopolymer":                                  # Eq all ones: the carry runs through all four dwords
            row = np.full(L, (31, 16, 31)[v])
        elif fam == "period2":                                    # variants 0 / 1: x = y[1:]; 2: one symbol doubled mid-way
            row = np.array([16, 31])[(j[:L] + (v == 1) - ((v == 2) & (j[:L] >= L // 2))) % 2]
        elif fam == "period3":                                    # the three phases
            row = np.array([7, 24, 31])[(j[:L] + v) % 3]
        elif fam == "parent_piece":                               # prefix, suffix, middle of the one parent
            o = (0, 128 - L, (128 - L) // 2)[v]
            row = parent[o:o + L]
        elif fam == "mutant":
            row = _mutant(rng, parent, L, v)[0]
        elif fam == "uniform":
            row = rng.integers(1, 32, L)
        else:
            continue
        T[r, :L] = row
    for r in range(n):                                            # exact duplicates: the same slot 1, 3 or 5 blocks on
        L, fam, v = set_b_layout(r)
        if fam == "duplicate":
            src = (r + (1 + 2 * v) * len(LENS)) % n
            assert set_b_layout(src)[1] != "duplicate" and set_b_layout(src)[0] == L
            T[r] = T[src]
    T.setflags(write=False)
    _set_b = T
    return T


def lengths(T):
    """Index of the last non-zero + 1 per row."""
    T = np.asarray(T)
    return np.where(T != 0, np.arange(1, T.shape[1] + 1), 0).max(axis=1, initial=0)


def wagner_fischer(X, Y):
    """(M, N) int64 edit distances of the rows of Y against the rows of X (zeros are trailing padding): the Wagner-Fischer
    table D[i][j] = min(D[i-1][j-1] + (y_i != x_j), D[i-1][j] + 1, D[i][j-1] + 1), the plain double loop over positions,
    all pairs at once (the rows of Y taken length by length, so that the outer loop stops at the last row of their
    tables).  Shares nothing with the C oracle."""
    X, Y = np.atleast_2d(np.asarray(X, dtype=np.int64)), np.atleast_2d(np.asarray(Y, dtype=np.int64))
    lx, ly = lengths(X), lengths(Y)
    Xt = np.ascontiguousarray(X[:, :lx.max(initial=0)].T)        # Xt[j - 1]: symbol j of every column sequence
    N, LX = len(X), len(Xt)
    out = np.empty((len(Y), N), dtype=np.int64)
    for l in np.unique(ly):
        rows = np.nonzero(ly == l)[0]
        D = np.empty((LX + 1, len(rows), N), dtype=np.int64)      # one table row for every pair: D[j] = D[i][j]
        D[:] = np.arange(LX + 1)[:, None, None]
        for i in range(1, l + 1):
            yi = Y[rows, i - 1][:, None]
            diag = D[0].copy()
            D[0] = i
            for j in range(1, LX + 1):
                up = D[j].copy()
                D[j] = np.minimum(diag + (yi != Xt[j - 1]), np.minimum(up, D[j - 1]) + 1)
                diag = up
        out[rows] = np.take_along_axis(D, np.broadcast_to(lx[None, None, :], (1, len(rows), N)), 0)[0]
    return out


def oracle_pairs(X, Y, band=128):
    """(M, N) int64 of orc_lev_pair(y, x, band), pair by pair like `pair_matrix`, without a numpy round trip per pair."""
    X, Y = np.ascontiguousarray(X, dtype=np.uint8), np.ascontiguousarray(Y, dtype=np.uint8)
    f = C.lib().orc_lev_pair
    f.restype = ctypes.c_int
    lx, ly = [int(v) for v in lengths(X)], [int(v) for v in lengths(Y)]
    px = [ctypes.c_void_p(X.ctypes.data + c * X.strides[0]) for c in range(len(X))]
    py = [ctypes.c_void_p(Y.ctypes.data + r * Y.strides[0]) for r in range(len(Y))]
    return np.array([[f(py[r], ly[r], px[c], lx[c], band) for c in range(len(X))] for r in range(len(Y))], dtype=np.int64)


_set_b_matrix = None


def set_b_matrix():
    """The (441, 441) unbanded distances of set B from the C oracle; the same (read-only) array on every call."""
    global _set_b_matrix
    if _set_b_matrix is None:
        _set_b_matrix = oracle_pairs(set_b(), set_b())
        _set_b_matrix.setflags(write=False)
    return _set_b_matrix


OPS = {"le": operator.le, "lt": operator.lt, "eq": operator.eq, "ge": operator.ge, "gt": operator.gt}
