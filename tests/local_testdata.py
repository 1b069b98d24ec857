"""
The yardstick of the local alignment tests (tests/test_local_alignment_cpu.py, tests/test_local_alignment_gpu.py):
`definition`, Gotoh's three tables with the zero floor as a plain numpy double loop over the positions of the two
sequences, and `brute_force`, every pair of substrings and every alignment path of them.  Nothing under prograph_amd/
imports this file.
"""
import numpy as np

NEG = -(1 << 40)


def lengths(T):
    """Index of the last non-zero + 1 per row."""
    T = np.asarray(T)
    return np.where(T != 0, np.arange(1, T.shape[1] + 1), 0).max(axis=1, initial=0)


def definition(S, gap, gap_open, X, Y):
    """(M, N) int64: max over i <= len x, j <= len y of H[i][j], i over the positions of x and j over those of y, all
    (M, N) pairs at once.  A cell beyond a pair's own lengths is computed (it feeds no cell inside them: a cell reads
    lower i and j only) and kept out of the maximum."""
    S, X, Y = np.asarray(S, dtype=np.int64), np.atleast_2d(np.asarray(X, dtype=np.intp)), np.atleast_2d(np.asarray(Y, dtype=np.intp))
    lx, ly = lengths(X), lengths(Y)
    LX, LY, M, N, e, o = int(lx.max(initial=0)), int(ly.max(initial=0)), len(Y), len(X), int(gap), int(gap_open)
    best = np.zeros((M, N), dtype=np.int64)
    H = np.zeros((LY + 1, M, N), dtype=np.int64)                  # row i - 1, then row i
    E = np.full((LY + 1, M, N), NEG, dtype=np.int64)              # E[0][j] = -inf
    for i in range(1, LX + 1):
        sx = S[X[:, i - 1]]                                       # (N, A): the scores of x_i against every symbol
        diag = H[0].copy()                                        # H[i-1][0] = 0
        F = np.full((M, N), NEG, dtype=np.int64)                  # F[i][0] = -inf
        in_x = (i <= lx)[None, :]
        for j in range(1, LY + 1):
            E[j] = np.maximum(E[j] - e, H[j] - o - e)             # from row i - 1 of the same column
            F = np.maximum(F - e, H[j - 1] - o - e)               # H[j - 1] is row i already
            h = np.maximum(np.maximum(0, diag + sx[:, Y[:, j - 1]].T), np.maximum(E[j], F))
            diag = H[j].copy()
            H[j] = h
            best = np.where(in_x & (j <= ly)[:, None], np.maximum(best, h), best)
    return best


def brute_force(S, gap, gap_open, x, y):
    """The best of all alignments of all pairs of a substring of x and a substring of y (token lists), each path walked
    to its end: a column pairs two symbols, or leaves one of x unaligned (kind 1), or one of y (kind 2); an unaligned
    column costs `gap`, plus `gap_open` unless the column before it is of the same kind.  The empty alignment scores 0."""
    def walk(a, b, i, j, last):
        if i == len(a) and j == len(b):
            return 0
        best = NEG
        if i < len(a) and j < len(b):
            best = max(best, int(S[a[i]][b[j]]) + walk(a, b, i + 1, j + 1, 0))
        if i < len(a):
            best = max(best, -gap - (0 if last == 1 else gap_open) + walk(a, b, i + 1, j, 1))
        if j < len(b):
            best = max(best, -gap - (0 if last == 2 else gap_open) + walk(a, b, i, j + 1, 2))
        return best
    best = 0
    for a0 in range(len(x)):
        for a1 in range(a0 + 1, len(x) + 1):
            for b0 in range(len(y)):
                for b1 in range(b0 + 1, len(y) + 1):
                    best = max(best, walk(x[a0:a1], y[b0:b1], 0, 0, 0))
    return best


def score_table(rng, a, lo, hi, diag=None):
    """A symmetric (a, a) table with entries in lo..hi; `diag`: the values the diagonal is drawn from."""
    S = np.triu(rng.integers(lo, hi + 1, (a, a)), 1)
    S = S + S.T
    S[np.arange(a), np.arange(a)] = rng.integers(lo, hi + 1, a) if diag is None else rng.choice(np.asarray(diag), a)
    return S


def rows_of(rng, a, lens, width, low=1):
    """Rows of tokens low..a-1 with the given lengths (the last symbol never 0), zero right-padded to `width`."""
    T = np.zeros((len(lens), width), dtype=np.int64)
    for r, l in enumerate(lens):
        T[r, :l] = rng.integers(low, a, l)
        if l and T[r, l - 1] == 0:
            T[r, l - 1] = a - 1
    return T


def knn_of(D, k, first):
    """Ranks first..first+k-1 of the stable descending (score, column) order."""
    order = np.argsort(-D, axis=1, kind="stable")[:, first:first + k]
    return order, np.take_along_axis(D, order, 1)


def csr_of(D, comp, eps, diagonal=True):
    """{(r, c): s > 0, comp(eps, s)} (without c == r when `diagonal` is False) as (indptr, indices, scores)."""
    keep = comp(eps, D) & (D > 0)
    if not diagonal:
        keep &= ~np.eye(len(D), dtype=bool)
    r, c = np.nonzero(keep)
    return np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64), c, D[r, c]
