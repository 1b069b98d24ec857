"""
Constructed inputs for the seams of the symmetric kNN sweep - numpy only, no GPU.  The sweep is exact for a
row whose (k+1)-th key lies below the optimistic cap and whose slot of delivered keys did not overflow; everything else is
evicted.  Random clusters sit far from both conditions (mates at distance <= 6, unrelated rows at ~0.95 L), so the inputs
here are built to sit ON them:

  ladder      members at pairwise distance |i - j| exactly: a row's rank-k distance is a formula (rank_k_distance), and k picks
              which rows sit one below the cap, at it, above it
  duplicates  identical rows at ascending indices: member j receives exactly j delivered keys, all at distance 0, and with
              k >= j + 1 it needs every one of them

and the shapes, ks and knobs of tests/test_knn_sym_edges_gpu.py, which tests/test_knn_sym_edges_cpu.py pins with the oracle
and the host plan.
"""
import numpy as np

# the optimistic cap of the MFMA engine's kNN (knn_launch): 10 where the signature has 54 bits (L > 32), 7 for one group
CAPS = {64: 10, 32: 7}
MAX_K = 19                                                   # k + 1 <= PG_MM_KL = 20: the short-list instance the sweep runs on
OUT_OF_REACH = "100000000"                                   # PG_KNN_SYM_EVICT_LIMIT no launch reaches


def filler(n, l, seed):
    """unrelated rows: uniform tokens in 1..20"""
    return np.random.RandomState(seed).randint(1, 21, size=(n, l)).astype(np.uint8)


def ladder(base, m):
    """m rows: member j is `base` with its first j positions replaced by base[p] % 20 + 1 (another token of 1..20), so
    members i and j differ in exactly the positions min(i, j) .. max(i, j) - 1: d(i, j) = |i - j|"""
    base = np.asarray(base, dtype=np.uint8)
    assert base.ndim == 1 and 1 <= m <= len(base) + 1 and base.min() >= 1 and base.max() <= 20
    out = np.repeat(base[None, :], m, axis=0)
    for j in range(m):
        out[j, :j] = base[:j] % 20 + 1
    return out


def rank_k_distance(m, j, k):
    """the distance of member j's k-th neighbour inside a ladder of m members (None: the ladder has fewer than k others)"""
    d = sorted(abs(i - j) for i in range(m) if i != j)
    return d[k - 1] if k <= len(d) else None


ORDERS = ("ascending", "descending", "interleaved", "straddling")
LADDER_N = 193                                               # three row blocks and one row, two super-tiles
LADDER_M = (24, 21)                                          # members of the two ladders (>= 2 cap + 2 and >= 2 cap - 1 at cap 10)


def place(ladders, n, order, seed=0):
    """the ladders' members in an n-row matrix of unrelated rows -> (tokens, [rows of ladder 0's members, rows of ladder 1's])
      ascending    ladder after ladder from row 3 on, member j at the j-th of its rows: member 0 has every neighbour in its
                   own lists (columns above the row), the last member gets every one by delivery
      descending   the same rows, member j at the j-th from the end
      interleaved  two ladders alternate rows from row 3 on
      straddling   ladder 0 from row 56 (across the block seam at 64), ladder 1 from row 120 (across the super-tile seam at 128)"""
    l = ladders[0].shape[1]
    tok = filler(n, l, 7700 + seed)
    rows = []
    if order in ("ascending", "descending"):
        at = 3
        for lad in ladders:
            r = np.arange(at, at + len(lad))
            rows.append(r if order == "ascending" else r[::-1].copy())
            at += len(lad) + 2
    elif order == "interleaved":
        assert len(ladders) == 2
        rows = [3 + i + 2 * np.arange(len(lad)) for i, lad in enumerate(ladders)]
    elif order == "straddling":
        assert len(ladders) == 2 and len(ladders[0]) == 24 and len(ladders[1]) == 21
        rows = [56 + np.arange(24), 120 + np.arange(21)]     # rows 56..79 and 120..140
    else:
        raise ValueError(order)
    for lad, r in zip(ladders, rows):
        assert r.max() < n
        tok[r] = lad
    assert len(np.unique(np.concatenate(rows))) == sum(len(r) for r in rows)
    return tok, rows


def ladder_case(l, order):
    """two ladders of LADDER_M members on random bases of length l in LADDER_N rows"""
    bases = filler(2, l, 5100 + l)
    return place([ladder(bases[i], LADDER_M[i]) for i in range(2)], LADDER_N, order, seed=l)


def cap_ks(c):
    """the four ks that put ladder rows one below the cap c, at it and above it (see test_knn_sym_edges_cpu.py)"""
    return tuple(k for k in (c - 1, c, 2 * c - 2, 2 * c - 1) if 1 <= k <= MAX_K)


def duplicates(n, size, stride, l=64, start=50, seed=0, lag=8):
    """n unrelated rows of length l with a cluster of `size` identical rows at start, start + stride, ...; stride = 2: a second
    cluster of `size` identical rows on the odd rows, `lag` members behind the first - B's member i sits on the row after A's
    member i + lag -> (tokens, rows of cluster A, rows of B or None).  Member j of a cluster has j identical rows below it:
    j delivered keys, all at distance 0.  With slots of `lag` keys the rows after A's overflowing members lag + 1 .. are B's
    members 1 ..: rows that keep their slot and read it from its first entry on."""
    assert stride in (1, 2)
    tok = filler(n, l, 8800 + seed)
    a = start + stride * np.arange(size)
    b = start + 2 * (lag + np.arange(size)) + 1 if stride == 2 else None
    assert (a if b is None else b).max() < n
    tok[a] = filler(1, l, 8801 + seed)[0]
    if b is not None:
        tok[b] = filler(1, l, 8802 + seed)[0]
    return tok, a, b


def delivered(tok, cap):
    """per row, from the definition: the pairs with a lower index and d < cap - what the sweep sends to the row's slot"""
    t = tok.astype(np.int16)
    d = (t[:, None, :] != t[None, :, :]).sum(axis=2)
    return np.tril(d < cap, -1).sum(axis=1)


# slots of 8 keys (PG_KNN_SYM_CAPL=8): (cluster size, stride); members 7, 8 and 9 are one below, at and one above the slot
SLOT8_N = 193
SLOT8_CLUSTERS = ((12, 1), (12, 2), (24, 1), (24, 2))
SLOT8_KS = (9, 12, 19)
# the production slot (256 keys): 300 identical rows from row 100 on - members 255, 256 and 257 at rows 355, 356, 357
SLOT256_N, SLOT256_SIZE, SLOT256_START = 1000, 300, 100
SLOT256_KS = (1, 19)

# PG_SYM_MAX_PIECES = 16 lists a row.  A block of `len` super-tiles in pieces of P gets min(ceil(len / P), len // 3, 16), P >= 3:
# sixteen pieces need 48 super-tiles - 6017 rows is the smallest graph whose block 0 has them (pieces of 3), and 6401 rows
# (51 super-tiles) the smallest that asks for 17 and is clamped
PIECES_16 = (6017, "3")                                      # (rows, PG_KNN_SYM_PIECE)
PIECES_17 = (6401, "3")
PIECES_KS = (1, 19)


def pieces_asked(n, piece):
    """what block 0 of an n-row sweep asks for before the clamp at 16 (sym_block_pieces with a fixed piece length)"""
    length = (n + 127) // 128
    p = min(max(int(piece), 3), max(length, 3))
    return max(1, min((length + p - 1) // p, length // 3))


WIDTHS = (1, 5, 31, 32, 33, 40, 63, 64)
WIDTH_NS = (129, 1000)
WIDTH_KS = (1, 6, 19)


def width_case(n, l):
    """clustered rows of length l with a ladder across the block seam at 64 (rows 56 .., as many members as l allows, 24 at
    most) and two interleaved clusters of 24 duplicates from row 80 on"""
    from prograph_amd import synth
    tok = np.ascontiguousarray(synth.clustered_tokens(n, l, seed=2600 + n + l, members=64))
    m = min(l + 1, 24)
    tok[56:56 + m] = ladder(filler(1, l, 2601 + l)[0], m)
    a = 80 + 2 * np.arange(24)
    tok[a] = filler(1, l, 2602 + l)[0]
    tok[a + 1] = filler(1, l, 2603 + l)[0]
    return tok


TINY_NS = (1, 2, 20, 63, 64)
TINY_LS = (32, 64)
TINY_KS = (1, 19)


def tiny_case(n, l):
    """n rows: a ladder of up to 8 members from row 0, the rest unrelated, the last row a copy of row 0"""
    tok = filler(n, l, 3300 + n + l)
    m = min(n, 8)
    tok[:m] = ladder(filler(1, l, 3301 + l)[0], m)
    tok[n - 1] = tok[0]
    return tok
