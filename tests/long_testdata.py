"""
The yardstick of the tests of the alignment kernels beyond 128 positions (tests/test_alignment_long_cpu.py,
tests/test_alignment_long_gpu.py): `definition`, the affine global recurrence (Gotoh's H, E, F) as the plain numpy double
loop over the positions of the two sequences of tests/test_alignment_affine_gpu.py's yardstick, here with all (M, N)
pairs in one pass - the tables are filled to the longest y and every pair reads H[len x][len y] when the outer loop
reaches its len x - so that 300 x 300 positions take about a second.  gap_open = 0 is the linear penalty.  The local
scores' yardstick is tests/local_testdata.py.  Nothing under prograph_amd/ imports this file.
"""
import numpy as np

INF = 1 << 40


def lengths(T):
    """Index of the last non-zero + 1 per row."""
    T = np.asarray(T)
    return np.where(T != 0, np.arange(1, T.shape[1] + 1), 0).max(axis=1, initial=0)


def definition(C, gap, gap_open, X, Y):
    """(M, N) int64: H[len x][len y] of the affine recurrence, i over the positions of x, j over those of y."""
    C, X, Y = np.asarray(C, dtype=np.int64), np.atleast_2d(np.asarray(X, dtype=np.intp)), np.atleast_2d(np.asarray(Y, dtype=np.intp))
    lx, ly = lengths(X), lengths(Y)
    LX, LY, M, N, e, o = int(lx.max(initial=0)), int(ly.max(initial=0)), len(Y), len(X), int(gap), int(gap_open)
    H = np.empty((LY + 1, M, N), dtype=np.int64)
    H[:] = (o + np.arange(LY + 1) * e)[:, None, None]             # row 0: H[0][j] = o + j e,
    H[0] = 0                                                      # H[0][0] = 0
    E = np.full((LY + 1, M, N), INF, dtype=np.int64)              # E[0][j] = inf
    at = np.broadcast_to(ly[None, :, None], (1, M, N))
    out = np.take_along_axis(H, at, 0)[0].copy()                  # len x = 0
    for i in range(1, LX + 1):
        cx = C[X[:, i - 1]]                                       # (N, A): the costs of x_i against every symbol
        diag = H[0].copy()
        H[0] = o + i * e
        F = np.full((M, N), INF, dtype=np.int64)                  # F[i][0] = inf
        for j in range(1, LY + 1):
            up = H[j].copy()
            E[j] = np.minimum(E[j] + e, up + o + e)
            F = np.minimum(F + e, H[j - 1] + o + e)
            H[j] = np.minimum(diag + cx[:, Y[:, j - 1]].T, np.minimum(E[j], F))
            diag = up
        done = lx == i
        if done.any():
            out[:, done] = np.take_along_axis(H, at, 0)[0][:, done]
    return out


def cost_table(rng, a, top):
    """A symmetric (a, a) cost table with a zero diagonal and entries up to `top`, `top` among them."""
    C = np.triu(rng.integers(0, top + 1, (a, a)), 1)
    C[0, a - 1] = top
    return C + C.T


def rows_of(rng, a, lens, width, low=1):
    """Rows of tokens low..a-1 with the given lengths (the last symbol never 0), zero right-padded to `width`."""
    T = np.zeros((len(lens), width), dtype=np.int64)
    for r, l in enumerate(lens):
        T[r, :l] = rng.integers(low, a, l)
        if l and T[r, l - 1] == 0:
            T[r, l - 1] = a - 1
    return T


def knn_of(D, k, first, descending=False):
    """Ranks first..first+k-1 of the stable (value, column) order."""
    order = np.argsort(-D if descending else D, axis=1, kind="stable")[:, first:first + k]
    return order, np.take_along_axis(D, order, 1)


def csr_of(D, comp, eps, keep_zero=False, diagonal=True):
    """{(r, c): comp(d, eps), d > 0 (d >= 0 with keep_zero)} (without c == r when `diagonal` is False)."""
    keep = comp(D, eps) & ((D >= 0) if keep_zero else (D > 0))
    if not diagonal:
        keep &= ~np.eye(len(D), dtype=bool)
    r, c = np.nonzero(keep)
    return np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64), c, D[r, c]
