"""
The yardstick of the fit alignment tests (tests/test_fit_alignment_cpu.py, ..._gpu.py, ..._long_gpu.py): `definition`,
Gotoh's three tables WITHOUT a floor as a plain numpy double loop over the positions of the two sequences, row 0 charged
for the prefix of y and the result read from column len y alone; `brute_force`, the worded definition: every substring of
x and every alignment path of all of y against it; and `canonical`, the trace rule for one pair on plain Python lists.
Nothing under prograph_amd/ imports this file.
"""
import numpy as np

from local_testdata import lengths, rows_of, score_table          # noqa: F401 (shared with the tests)

NEG = -(1 << 40)


def definition(S, gap, gap_open, X, Y):
    """(M, N) int64: max over i = 0..len x of H[i][len y], i over the positions of x and j over those of y, all (M, N)
    pairs at once.  The tables are filled to the longest x and y; a pair reads column len y after every outer step
    i <= len x (a cell reads lower i and j only, so cells beyond a pair's own lengths feed nothing that is read)."""
    S, X, Y = np.asarray(S, dtype=np.int64), np.atleast_2d(np.asarray(X, dtype=np.intp)), np.atleast_2d(np.asarray(Y, dtype=np.intp))
    lx, ly = lengths(X), lengths(Y)
    LX, LY, M, N, e, o = int(lx.max(initial=0)), int(ly.max(initial=0)), len(Y), len(X), int(gap), int(gap_open)
    H = np.zeros((LY + 1, M, N), dtype=np.int64)                  # row i - 1, then row i
    H[1:] = -(o + e * np.arange(1, LY + 1))[:, None, None]        # H[0][j] = -(o + j e): all of y is paid for
    E = np.full((LY + 1, M, N), NEG, dtype=np.int64)              # E[0][j] = -inf
    at = np.broadcast_to(ly[None, :, None], (1, M, N))
    best = np.take_along_axis(H, at, 0)[0].copy()                 # H[0][len y]
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
    return best


def global_walk(S, gap, gap_open, a, b):
    """The best global alignment of token lists a and b, each path walked to its end: a column pairs two symbols, or leaves
    one of a unaligned (kind 1), or one of b (kind 2); an unaligned column costs `gap`, plus `gap_open` unless the column
    before it is of the same kind."""
    def walk(i, j, last):
        if i == len(a) and j == len(b):
            return 0
        best = NEG
        if i < len(a) and j < len(b):
            best = max(best, int(S[a[i]][b[j]]) + walk(i + 1, j + 1, 0))
        if i < len(a):
            best = max(best, -gap - (0 if last == 1 else gap_open) + walk(i + 1, j, 1))
        if j < len(b):
            best = max(best, -gap - (0 if last == 2 else gap_open) + walk(i, j + 1, 2))
        return best
    return walk(0, 0, 0)


def brute_force(S, gap, gap_open, x, y):
    """The worded definition on two token lists: the best, over every substring of x (the empty one included), of the
    global score of ALL of y against it."""
    best = global_walk(S, gap, gap_open, [], y)
    for a0 in range(len(x)):
        for a1 in range(a0 + 1, len(x) + 1):
            best = max(best, global_walk(S, gap, gap_open, x[a0:a1], y))
    return best


def canonical(S, gap, gap_open, x, y):
    """The canonical fit alignment of y (whole) within x (free ends), token lists: the full tables in plain Python, the
    end cell the best H[i][len y] with ties to the smallest i, the walk of prograph_amd/alignments.py (the diagonal wins a
    tie, then E; open wins a tie), stopping in state H at j = 0 and leaving the j remaining symbols of y unaligned at
    i = 0.  Returns (score, x_begin, x_end, y_begin, y_end, n_ops, identities, ops list)."""
    e, o, lx, ly = int(gap), int(gap_open), len(x), len(y)
    H = [[0] * (ly + 1) for _ in range(lx + 1)]
    E = [[NEG] * (ly + 1) for _ in range(lx + 1)]
    F = [[NEG] * (ly + 1) for _ in range(lx + 1)]
    for j in range(1, ly + 1):
        H[0][j] = -(o + j * e)
    for i in range(1, lx + 1):
        for j in range(1, ly + 1):
            E[i][j] = max(E[i - 1][j] - e, H[i - 1][j] - o - e)
            F[i][j] = max(F[i][j - 1] - e, H[i][j - 1] - o - e)
            H[i][j] = max(H[i - 1][j - 1] + int(S[x[i - 1]][y[j - 1]]), E[i][j], F[i][j])
    bi = max(range(lx + 1), key=lambda i: (H[i][ly], -i))
    i, j, state, ops, ident = bi, ly, 0, [], 0
    while True:
        if state == 0:
            if j == 0:
                break
            if i == 0:
                ops += [3] * j
                j = 0
                break
            if H[i][j] == H[i - 1][j - 1] + int(S[x[i - 1]][y[j - 1]]):
                ops.append(1)
                ident += int(x[i - 1] == y[j - 1])
                i, j = i - 1, j - 1
            else:
                state = 1 if H[i][j] == E[i][j] else 2
        elif state == 1:
            ops.append(2)
            if E[i][j] == H[i - 1][j] - o - e:
                state = 0
            i -= 1
        else:
            ops.append(3)
            if F[i][j] == H[i][j - 1] - o - e:
                state = 0
            j -= 1
    return H[bi][ly], i, bi, 0, ly, len(ops), ident, ops[::-1]


def seq(row):
    """A row without its trailing zeros, as a list."""
    row = [int(t) for t in row]
    while row and row[-1] == 0:
        row.pop()
    return row


def fragments(rng, a, n, width, low=1, lens=None, least=0):
    """n rows of width `width`: a third random parents of random lengths, the rest fragments cut from earlier rows (some
    with one symbol changed), so that a row is contained in another, and short rows meet long ones both ways round; no
    parent is shorter than `least`."""
    T = np.zeros((n, width), dtype=np.int64)
    for r in range(n):
        if r < 3 or r % 3 == 0:
            l = int(rng.integers(least, width + 1)) if lens is None else int(lens[r])
            T[r, :l] = rng.integers(low, a, l)
        else:
            p = seq(T[int(rng.integers(0, r))])
            if len(p) < 2:
                T[r, :1] = rng.integers(max(low, 1), a, 1)
                continue
            a0 = int(rng.integers(0, len(p) - 1))
            a1 = int(rng.integers(a0 + 1, len(p) + 1))
            f = p[a0:a1]
            if r % 2 and len(f) > 2:
                f[len(f) // 2] = int(rng.integers(low, a))
            T[r, :len(f)] = f
        l = len(seq(T[r])) if T[r].any() else 0
        if l and T[r, l - 1] == 0:
            T[r, l - 1] = a - 1
    return T
