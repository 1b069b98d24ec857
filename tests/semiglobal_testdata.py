"""
The yardstick of the semi-global alignment tests (tests/test_semiglobal_alignment_cpu.py, ..._gpu.py, ..._long_gpu.py):
`definition`, Gotoh's three tables WITHOUT a floor as a plain numpy double loop over the positions of the two sequences,
the result read from the last row and the last column of every pair's table, and `brute_force`, the worded definition:
every free prefix / suffix choice and every alignment path of the rest.  Nothing under prograph_amd/ imports this file.
"""
import numpy as np

from local_testdata import csr_of, knn_of, lengths, rows_of, score_table          # noqa: F401 (shared with the tests)

NEG = -(1 << 40)


def definition(S, gap, gap_open, X, Y):
    """(M, N) int64: max(max_i H[i][len y], max_j H[len x][j]), i over the positions of x and j over those of y, all
    (M, N) pairs at once.  The tables are filled to the longest x and y; a pair reads column len y after every outer
    step i <= len x and the cells j <= len y of row i when the outer loop reaches its len x (a cell reads lower i and j
    only, so cells beyond a pair's own lengths feed nothing that is read)."""
    S, X, Y = np.asarray(S, dtype=np.int64), np.atleast_2d(np.asarray(X, dtype=np.intp)), np.atleast_2d(np.asarray(Y, dtype=np.intp))
    lx, ly = lengths(X), lengths(Y)
    LX, LY, M, N, e, o = int(lx.max(initial=0)), int(ly.max(initial=0)), len(Y), len(X), int(gap), int(gap_open)
    best = np.zeros((M, N), dtype=np.int64)                       # H[0][len y] = 0; row 0 when len x = 0
    H = np.zeros((LY + 1, M, N), dtype=np.int64)                  # row i - 1, then row i; H[0][j] = 0
    E = np.full((LY + 1, M, N), NEG, dtype=np.int64)              # E[0][j] = -inf
    at = np.broadcast_to(ly[None, :, None], (1, M, N))
    in_y = (np.arange(LY + 1)[:, None] <= ly[None, :])[:, :, None]          # (LY + 1, M, 1): j <= len y
    for i in range(1, LX + 1):
        sx = S[X[:, i - 1]]                                       # (N, A): the scores of x_i against every symbol
        diag = H[0].copy()                                        # H[i-1][0] = 0
        F = np.full((M, N), NEG, dtype=np.int64)                  # F[i][0] = -inf
        for j in range(1, LY + 1):
            E[j] = np.maximum(E[j] - e, H[j] - o - e)             # from row i - 1 of the same column
            F = np.maximum(F - e, H[j - 1] - o - e)               # H[j - 1] is row i already
            h = np.maximum(diag + sx[:, Y[:, j - 1]].T, np.maximum(E[j], F))
            diag = H[j].copy()
            H[j] = h
        col = np.take_along_axis(H, at, 0)[0]                     # H[i][len y]
        best = np.where((i <= lx)[None, :], np.maximum(best, col), best)
        row = np.where(in_y, H, NEG).max(axis=0)                  # max over j <= len y of H[i][j]
        best = np.where((i == lx)[None, :], np.maximum(best, row), best)
    return best


def brute_force(S, gap, gap_open, x, y):
    """The worded definition on two token lists: drop a prefix of at most one of the two and a suffix of at most one of
    them, then align what is left globally, each path walked to its end: a column pairs two symbols, or leaves one of x
    unaligned (kind 1), or one of y (kind 2); an unaligned column costs `gap`, plus `gap_open` unless the column before it
    is of the same kind."""
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
    best = NEG
    for a0 in range(len(x) + 1):
        for b0 in range(len(y) + 1):
            if a0 and b0:
                continue                                          # a prefix of at most one
            for a1 in range(a0, len(x) + 1):
                for b1 in range(b0, len(y) + 1):
                    if a1 < len(x) and b1 < len(y):
                        continue                                  # a suffix of at most one
                    best = max(best, walk(x[a0:a1], y[b0:b1], 0, 0, 0))
    return best
