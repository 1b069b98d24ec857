"""
The yardstick of the alignment traceback tests (tests/test_alignment_trace_cpu.py, tests/test_alignment_trace_gpu.py).

`definition` is the canonical alignment of DESIGN.md §4.20 as plain Python loops over single cells: the three tables of the
operator modules as they state them (`alignment` minimising over its cost table, the two scores maximising), the end cell,
and the walk back comparing table entries - no direction bits, no negated table, no running maxima.  `rescore` prices a
list of ops again from the table and the gap penalties alone.  `brute_force` is the worded definition of each operator's
value: every alignment path of every admissible pair of substrings.  Nothing under prograph_amd/ imports this file.
"""
import numpy as np

GLOBAL, LOCAL, SEMIGLOBAL = 0, 1, 2
INF = 1 << 40
FIELDS = ("score", "x_begin", "x_end", "y_begin", "y_end", "n_ops", "identities")


def sequence(row):
    """A row without its trailing zeros, as a list of ints."""
    row = [int(v) for v in row]
    while row and row[-1] == 0:
        row.pop()
    return row


def definition(mode, T, gap, gap_open, x, y):
    """{score, x_begin, x_end, y_begin, y_end, n_ops, identities, ops (list, forward order)} of the token lists x, y."""
    x, y = sequence(x), sequence(y)
    lx, ly, e, o = len(x), len(y), int(gap), int(gap_open)
    if mode == GLOBAL:
        better, open_term, ext_term, none = min, (lambda h: h + o + e), (lambda g: g + e), INF
    else:
        better, open_term, ext_term, none = max, (lambda h: h - o - e), (lambda g: g - e), -INF
    H = [[0] * (ly + 1) for _ in range(lx + 1)]
    E = [[none] * (ly + 1) for _ in range(lx + 1)]
    F = [[none] * (ly + 1) for _ in range(lx + 1)]
    if mode == GLOBAL:
        for j in range(1, ly + 1):
            H[0][j] = o + j * e
        for i in range(1, lx + 1):
            H[i][0] = o + i * e
    for i in range(1, lx + 1):
        for j in range(1, ly + 1):
            E[i][j] = better(ext_term(E[i - 1][j]), open_term(H[i - 1][j]))
            F[i][j] = better(ext_term(F[i][j - 1]), open_term(H[i][j - 1]))
            h = better(H[i - 1][j - 1] + int(T[x[i - 1]][y[j - 1]]), E[i][j], F[i][j])
            H[i][j] = max(0, h) if mode == LOCAL else h
    # the end cell
    if mode == GLOBAL:
        bi, bj = lx, ly
    elif mode == LOCAL:
        bi = bj = 0
        for i in range(lx + 1):
            for j in range(ly + 1):
                if H[i][j] > H[bi][bj]:
                    bi, bj = i, j
    else:
        cells = sorted({(i, ly) for i in range(lx + 1)} | {(lx, j) for j in range(ly + 1)})       # by i, then j
        bi, bj = cells[0]
        for i, j in cells:
            if H[i][j] > H[bi][bj]:
                bi, bj = i, j
    # the walk
    i, j, state, ops, ident = bi, bj, "H", [], 0
    while True:
        if state == "H":
            if mode == LOCAL and H[i][j] == 0:
                break
            if mode == SEMIGLOBAL and (i == 0 or j == 0):
                break
            if mode == GLOBAL and (i == 0 or j == 0):
                ops += [3] * j if i == 0 else [2] * i
                i = j = 0
                break
            if H[i][j] == H[i - 1][j - 1] + int(T[x[i - 1]][y[j - 1]]):
                ops.append(1)
                ident += x[i - 1] == y[j - 1]
                i, j = i - 1, j - 1
            elif H[i][j] == E[i][j]:
                state = "E"
            else:
                assert H[i][j] == F[i][j]
                state = "F"
        elif state == "E":
            ops.append(2)
            if E[i][j] == open_term(H[i - 1][j]):
                state = "H"
            i -= 1
        else:
            ops.append(3)
            if F[i][j] == open_term(H[i][j - 1]):
                state = "H"
            j -= 1
    return dict(score=H[bi][bj], x_begin=i, x_end=bi, y_begin=j, y_end=bj, n_ops=len(ops), identities=int(ident),
                ops=ops[::-1])


def rescore(mode, T, gap, gap_open, x, y, x_begin, y_begin, ops):
    """(value, x_end, y_end) of the ops from (x_begin, y_begin) on: the table entry of every pair, `gap` per unaligned
    symbol and `gap_open` per maximal run of one kind; a cost for GLOBAL, a score otherwise."""
    x, y = sequence(x), sequence(y)
    i, j, pairs, gaps, last = int(x_begin), int(y_begin), 0, 0, 0
    for op in ops:
        op = int(op)
        assert op in (1, 2, 3)
        if op == 1:
            pairs += int(T[x[i]][y[j]])
        else:
            gaps += int(gap) + (0 if last == op else int(gap_open))
        i += op != 3
        j += op != 2
        last = op
    return (pairs + gaps if mode == GLOBAL else pairs - gaps), i, j


def _paths(S, gap, gap_open, a, b, i, j, last):
    """The best score (maximising over S) of aligning a[i:] with b[j:] globally, the column before of kind `last`."""
    if i == len(a) and j == len(b):
        return 0
    best = -INF
    if i < len(a) and j < len(b):
        best = max(best, int(S[a[i]][b[j]]) + _paths(S, gap, gap_open, a, b, i + 1, j + 1, 1))
    if i < len(a):
        best = max(best, -gap - (0 if last == 2 else gap_open) + _paths(S, gap, gap_open, a, b, i + 1, j, 2))
    if j < len(b):
        best = max(best, -gap - (0 if last == 3 else gap_open) + _paths(S, gap, gap_open, a, b, i, j + 1, 3))
    return best


def brute_force(mode, T, gap, gap_open, x, y):
    """The operator's value by exhaustion (sequences of a handful of symbols)."""
    x, y = sequence(x), sequence(y)
    if mode == GLOBAL:
        return -_paths(-np.asarray(T, dtype=np.int64), gap, gap_open, x, y, 0, 0, 0)
    best = 0
    for a0 in range(len(x) + 1):
        for b0 in range(len(y) + 1):
            for a1 in range(a0, len(x) + 1):
                for b1 in range(b0, len(y) + 1):
                    if mode == SEMIGLOBAL and ((a0 and b0) or (a1 < len(x) and b1 < len(y))):
                        continue                                  # a free prefix of at most one, a free suffix of at most one
                    best = max(best, _paths(T, gap, gap_open, x[a0:a1], y[b0:b1], 0, 0, 0))
    return best
