"""
Constructed inputs for the group logs of the symmetric kNN sweep - numpy only, no GPU.  Delivered keys
travel to the log of the receiver's GROUP of sixteen consecutive rows: a batch of candidates is gathered by group, one
atomic and one contiguous run of entries per group, and the merge bins a group's log by the receiver's place.  The inputs
here sit on what that adds to tests/knn_sym_testdata.py: the group, block and super-tile seams, a log exactly full and one
entry over, a batch that lands in 64 groups and one that lands in a single group.  tests/test_knn_sym_group_cpu.py pins the
counts from the definition (knn_sym_testdata.delivered); tests/test_knn_sym_group_gpu.py runs them.
"""
import numpy as np

import knn_sym_testdata as D

GROUP = 16
CAP = D.CAPS[64]

# ---- members of clusters on both sides of the group (16), block (64) and super-tile (128) seams
SEAM_ROWS = (15, 16, 17, 31, 32, 63, 64, 65, 127, 128)
SEAM_NS = (129, 1000, 1001)                                  # a last group of 1, 8 and 9 rows
SEAM_KS = (1, 4, 19)


def seam_case(n, l=64):
    """n unrelated rows; two clusters of identical rows alternate over SEAM_ROWS (every seam has a member of each side in
    either cluster's reach), and a third one sits on the last rows of the graph: n - 1, n - 2 and n - 17 (the last group,
    which has fewer than sixteen rows, and the one before it) -> (tokens, [rows of A, rows of B, rows of C])"""
    tok = D.filler(n, l, 6100 + n)
    a, b = np.array(SEAM_ROWS[0::2]), np.array(SEAM_ROWS[1::2])
    c = np.array([n - 17, n - 2, n - 1]) if n - 17 > max(SEAM_ROWS) else np.array([], dtype=np.int64)
    for i, rows in enumerate((a, b, c)):
        if len(rows):
            tok[rows] = D.filler(1, l, 6200 + i)[0]
    return tok, [a, b, c]


# ---- a log exactly full and one entry over (PG_KNN_SYM_CAPL=8: sixteen rows x 8 = 128 entries)
FULL_CAPL = 8
FULL_N = 193
FULL_RECEIVERS = np.arange(128, 144)                         # one group
FULL_KS = (1, 8)                                             # k = 8: a receiver needs every one of its eight delivered keys


def full_case(over, l=64):
    """sixteen clusters: cluster c = eight identical senders at rows 8 c .. 8 c + 7 and the receiver 128 + c; clusters are
    unrelated.  The receivers' group gets 16 x 8 = 128 entries, every row 8: log and bins exactly full, all kept.
    over: row 129 joins cluster 0 - it has NINE senders (eight and row 128), the group gets 129 entries, all sixteen rows
    are evicted and recomputed."""
    tok = D.filler(FULL_N, l, 6300)
    base = D.filler(16, l, 6301)
    for c in range(16):
        tok[8 * c:8 * c + 8] = base[c]
        tok[128 + c] = base[c]
    if over:
        tok[129] = base[0]
    return tok


# ---- a batch that lands in 64 groups: the senders are the 64 rows of pass 0, their mates 17 rows and more apart
SPREAD_N = 2200
SPREAD_KS = (1, 2)


def spread_case(l=64):
    """row i < 64 and row 128 + 32 i + i % 16 are identical, nothing else is near: every delivered key of the batch has a
    group of its own (and every place 0 .. 15 occurs) -> (tokens, receivers)"""
    tok = D.filler(SPREAD_N, l, 6400)
    recv = 128 + 32 * np.arange(64) + np.arange(64) % 16
    tok[recv] = tok[:64]
    return tok, recv


# ---- a batch that lands in ONE group: sixteen receivers of one group, each near all rows of two passes
DENSE_N = 400
DENSE_RECEIVERS = np.arange(256, 272)
DENSE_KS = (1, 16, 19)


def dense_case(l=64):
    """rows 0 .. 127 (two passes) and the group 256 .. 271: one base sequence with up to two substitutions in positions
    that depend on the row (pairwise distance <= 4, below either cap); runs of 64 entries into one log, pass after pass"""
    tok = D.filler(DENSE_N, l, 6500)
    base = D.filler(1, l, 6501)[0]
    for r in list(range(128)) + list(DENSE_RECEIVERS):
        t = base.copy()
        for p in ((r * 7) % l, (r * 13 + 5) % l)[:r % 3]:
            t[p] = t[p] % 20 + 1
        tok[r] = t
    return tok


# ---- the direct form: every pair is below the cap, delivery runs from the epilogue
DIRECT_N, DIRECT_L = 300, 5
DIRECT_KS = (1, 6, 19)

# ---- the codec with 7 distance bits (PG_KNN_GUESS=65) on the device: ladders of every distance 1 .. 64
WIDE_N = 1000
WIDE_GUESS = "65"
WIDE_KS = (1, 19)


def wide_case(order, l=64):
    bases = D.filler(2, l, 6600)
    return D.place([D.ladder(bases[0], 65), D.ladder(bases[1], 40)], WIDE_N, order, seed=66)


def group_entries(tok, cap):
    """per group of sixteen rows: the entries the sweep appends to its log (the rows' delivered keys)"""
    per_row = D.delivered(tok, cap)
    pad = (-len(per_row)) % GROUP
    return np.concatenate([per_row, np.zeros(pad, dtype=per_row.dtype)]).reshape(-1, GROUP).sum(axis=1)
