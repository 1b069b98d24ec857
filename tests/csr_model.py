"""
An independent model of the CSR support layer (TEST-ONLY): what `pg_csr_row_stats` reduces, and what the graph analytics
make of it, written from the definitions in pure Python and NumPy.  It shares no code with prograph_amd/graph.py or
tests/fake_native.py: both are held against it (tests/test_csr_kernels_gpu.py, tests/test_graph_analytics_kinds_gpu.py,
tests/test_graph_containers_cpu.py).

Sums are `math.fsum` - the correctly rounded sum of the float64 terms - so a caller can state how far a float64 or
float32 accumulation in any order may be from them.  An entry whose column is negative is no edge and enters nothing.
"""
import math

import numpy as np

KEYS = ("deg", "sum_f", "sum_wf", "self_w", "col_sum")


def _edges(indptr, indices, w):
    """[(row, column, weight)] as Python numbers, entries with a negative column left out; no weights: 1.0 each."""
    indptr = [int(v) for v in indptr]
    out = []
    for r in range(len(indptr) - 1):
        for e in range(indptr[r], indptr[r + 1]):
            c = int(indices[e])
            if c >= 0:
                out.append((r, c, 1.0 if w is None else float(w[e])))
    return out


def row_stats(indptr, indices, w, f, row0, ncols):
    """The five reductions of `pg_csr_row_stats` as float64 arrays: per row deg = sum w, sum_f = sum f[col],
    sum_wf = sum w f[col] (each product rounded once to float64), self_w = sum of the weights of the entries whose
    column is row0 + row; per column col_sum = sum w.  `f` None: sum_f and sum_wf are left out.
    With them, under `abs_<key>` the same sums over the terms' magnitudes, and under `n_rows` / `n_cols` the number of
    edges of every row / column: what an error bound of a reordered sum is made of."""
    nrows = len(indptr) - 1
    per_row = {k: [[] for _ in range(nrows)] for k in KEYS[:4]}
    per_col = [[] for _ in range(int(ncols))]
    for r, c, wt in _edges(indptr, indices, w):
        per_row["deg"][r].append(wt)
        if f is not None:
            per_row["sum_f"][r].append(float(f[c]))
            per_row["sum_wf"][r].append(wt * float(f[c]))
        if c == row0 + r:
            per_row["self_w"][r].append(wt)
        per_col[c].append(wt)
    out = {}
    for k, lists in list(per_row.items()) + [("col_sum", per_col)]:
        if f is None and k in ("sum_f", "sum_wf"):
            continue
        out[k] = np.array([math.fsum(t) for t in lists], dtype=np.float64)
        out["abs_" + k] = np.array([math.fsum(abs(v) for v in t) for t in lists], dtype=np.float64)
    out["n_rows"] = np.array([len(t) for t in per_row["deg"]], dtype=np.int64)
    out["n_cols"] = np.array([len(t) for t in per_col], dtype=np.int64)
    return out


def analytics(indptr, indices, w, f, n):
    """The reference's analytics of a square graph over n nodes (row0 = 0), from its dense float64 matrix: A from the
    coordinates with duplicates summed, L = -A, diagonal overwritten by D, D kept in float32 as `degree()` returns it
    (out-degree: row sums; in-degree: column sums).  `w` None: boolean weights.  Returns
      degree            float32 [n]  row sums rounded once
      degree_exact      float64 [n]  the row sums themselves; degree_abs: of the magnitudes; counts int64 [n]
      indegree, indegree_exact, indegree_abs, col_counts   the same by column
      adjacency         float64 [n, n]
      laplacian         {"outdegree" | "indegree": float64 [n, n]}
      dirichlet         {mode: f^T L f, an fsum of the n^2 + n products}; dirichlet_abs: of their magnitudes
      local_variance    float64 [n]  f_r - mean of f over the row's edges, NaN for a row without edges
    (`f` None: no dirichlet, no local_variance)."""
    edges = _edges(indptr, indices, w)
    rows = [[] for _ in range(n)]
    cols = [[] for _ in range(n)]
    for r, c, wt in edges:
        rows[r].append((c, wt))
        cols[c].append(wt)
    out = {}
    for name, lists, pick in (("degree", rows, lambda e: e[1]), ("indegree", cols, lambda e: e)):
        exact = np.array([math.fsum(pick(e) for e in t) for t in lists], dtype=np.float64)
        out[name + "_exact"] = exact
        out[name + "_abs"] = np.array([math.fsum(abs(pick(e)) for e in t) for t in lists], dtype=np.float64)
        out[name] = exact.astype(np.float32)
    out["counts"] = np.array([len(t) for t in rows], dtype=np.int64)
    out["col_counts"] = np.array([len(t) for t in cols], dtype=np.int64)
    A = np.zeros((n, n), dtype=np.float64)
    for r in range(n):
        named = {}
        for c, wt in rows[r]:
            named.setdefault(c, []).append(wt)
        for c, t in named.items():
            A[r, c] = math.fsum(t)
    out["adjacency"] = A
    out["laplacian"] = {}
    for mode, D in (("outdegree", out["degree"]), ("indegree", out["indegree"])):
        L = -A
        L[np.arange(n), np.arange(n)] = D.astype(np.float64)
        out["laplacian"][mode] = L
    if f is None:
        return out
    fv = [float(v) for v in np.asarray(f, dtype=np.float64).reshape(-1)]
    out["dirichlet"], out["dirichlet_abs"] = {}, {}
    for mode, L in out["laplacian"].items():
        terms = [fv[r] * (float(L[r, c]) * fv[c]) for r in range(n) for c in np.nonzero(L[r])[0]]
        out["dirichlet"][mode] = math.fsum(terms)
        out["dirichlet_abs"][mode] = math.fsum(abs(t) for t in terms)
    lv = np.full(n, np.nan, dtype=np.float64)
    for r in range(n):
        if rows[r]:
            lv[r] = fv[r] - math.fsum(fv[c] for c, _ in rows[r]) / len(rows[r])
    out["local_variance"] = lv
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The edge lists the kernel tests and the stand-in's test share: every row length at which the wave loop of the kernel
# changes (one wave takes 64 entries a turn), workgroups of four rows filled and part filled, columns named by several
# lanes of a wave and by several rows, the row's own node absent, once and twice.
# ---------------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 600)
NROWS = (1, 3, 4, 5, 19)
NCOLS = 300
ROW0 = (0, 37)
HOT = 7                                     # the column every row names from several lanes: atomics meet on one word
SEED = {1: 8, 3: 1, 4: 4, 5: 7, 19: 0}      # nrows -> where in LENGTHS its first row starts: (600), (1, 63, 64),
#                                             (65, 127, 128, 129), (129, 600, 0, 1, 63), all of them twice


def edge_lists(nrows, row0, seed=0, ncols=NCOLS):
    """(indptr int64, indices int32): row r has LENGTHS[(r + seed) % 9] entries (nrows = 19: every length at least twice,
    in every position of a workgroup).  In a row of at least 3 entries HOT stands at entries 0, 1 and at every 5th;
    its own node row0 + r stands nowhere (r % 3 == 0), once (1) or twice (2) - in rows long enough -, the rest is random,
    so columns repeat within a row (600 entries over 300 columns) and between rows."""
    rng = np.random.default_rng(1000 * nrows + 10 * row0 + seed)
    lens = [LENGTHS[(r + seed) % len(LENGTHS)] for r in range(nrows)]
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    parts = []
    for r, n in enumerate(lens):
        own = row0 + r
        c = rng.integers(0, ncols, n)
        c[c == own] = (own + 1) % ncols
        if n >= 3:
            c[0] = c[1] = HOT
            c[::5] = HOT
            for at in ((), (n - 1,), (2, n - 1))[r % 3]:
                c[at] = own
        parts.append(c)
    return indptr, np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, np.int32)


def with_negative_columns(indptr, indices):
    """The same lists with -1 at entries 0, 63 and 64 of every row that has them, and, where there is more than one row,
    one row (the longest) all -1."""
    out = indices.copy()
    lens = np.diff(indptr)
    for r in range(len(lens)):
        for at in (0, 63, 64):
            if at < lens[r]:
                out[indptr[r] + at] = -1
    if len(lens) > 1:
        r = int(np.argmax(lens))
        out[indptr[r]:indptr[r + 1]] = -1
    return out


def exact_weights(kind, n, seed=0):
    """None | uint8 with 0 and 255 present | float32 multiples of 2^-10 in (-8, 8), negative ones among them."""
    rng = np.random.default_rng(77 + seed)
    if kind == "none":
        return None
    if kind == "u8":
        w = rng.integers(0, 256, n).astype(np.uint8)
        w[:2] = (0, 255)[:len(w[:2])]
        return w
    return (rng.integers(-8192, 8192, n) / 1024.0).astype(np.float32)


def exact_values(ncols, seed=0):
    """float64 multiples of 2^-20 in [0, 1): with the weights above every product and partial sum is exact in float64
    (magnitudes below 2^18, granularity 2^-30: 48 bits), so the sums do not depend on their order."""
    return np.random.default_rng(5 + seed).integers(0, 1 << 20, ncols) / float(1 << 20)
