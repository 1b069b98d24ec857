"""
An independent model of the graph operations (TEST-ONLY): `sorted`, `transpose` and `symmetrize` of a CSR as DESIGN.md §4.30
defines them, in pure Python lists and dicts.  It shares no code with prograph_amd/, with tests/fake_graph_native.py or with
tests/capi_graph: all are held against it (tests/test_graph_ops_cpu.py, tests/test_graph_ops_gpu.py).

A weight is carried as (bit pattern, value): the bits as a Python int of the dtype's unsigned view, the value as a Python int or
float (float16 and float32 are exact in a Python float).  What comes out is rebuilt from the bits, so "bit for bit" includes the
payload of a NaN and the sign of a zero.  An entry whose column is outside 0..ncols-1 is no edge.
"""
import numpy as np

import csr_model

_UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _weights(w):
    w = np.ascontiguousarray(w)
    bits = w.view(_UNSIGNED[w.dtype.itemsize]).tolist()
    return list(zip(bits, w.tolist()))


def _arrays(rows, dtype):
    """[[(column, (bits, value))]] per row -> (indptr int64, indices int32, weights dtype)."""
    indptr, indices, bits = [0], [], []
    for row in rows:
        for c, w in row:
            indices.append(c)
            bits.append(w[0])
        indptr.append(len(indices))
    dtype = np.dtype(dtype)
    return (np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32),
            np.array(bits, dtype=_UNSIGNED[dtype.itemsize]).view(dtype))


def edges(indptr, indices, weights, ncols):
    """[(row, column, weight)] in storage order, no-edge entries left out."""
    w = _weights(weights)
    out = []
    for r in range(len(indptr) - 1):
        for e in range(int(indptr[r]), int(indptr[r + 1])):
            c = int(indices[e])
            if 0 <= c < ncols:
                out.append((r, c, w[e]))
    return out


def sorted_rows(indptr, indices, weights, ncols):
    rows = [[] for _ in range(len(indptr) - 1)]
    for r, c, w in edges(indptr, indices, weights, ncols):
        rows[r].append((c, w))
    for row in rows:
        row.sort(key=lambda cw: cw[0])                      # list.sort is stable: equal columns stay in storage order
    return _arrays(rows, weights.dtype)


def transpose(indptr, indices, weights, ncols, row0=0):
    rows = [[] for _ in range(ncols)]
    for r, c, w in edges(indptr, indices, weights, ncols):
        rows[c].append((row0 + r, w))                       # storage order: ascending rows, duplicates in order
    return _arrays(rows, weights.dtype)


def pick(a, b, combine):
    """The winner of two weights (bits, value): a NaN loses to a number, of two NaNs and of two equal values (-0, +0) the smaller
    bit pattern wins; else the smaller (min) or larger (max) value."""
    nan_a, nan_b = a[1] != a[1], b[1] != b[1]
    if nan_a or nan_b:
        if nan_a and nan_b:
            return a if a[0] <= b[0] else b
        return b if nan_a else a
    if a[1] == b[1]:
        return a if a[0] <= b[0] else b
    low, high = (a, b) if a[1] < b[1] else (b, a)
    return low if combine == "min" else high


def symmetrize(indptr, indices, weights, mode="union", combine="min"):
    """Of a square graph over n = len(indptr) - 1 nodes."""
    n = len(indptr) - 1
    forward, found = set(), {}
    for r, c, w in edges(indptr, indices, weights, n):
        forward.add((r, c))
        for key in {(r, c), (c, r)}:                        # a self-loop is its own reverse: it enters once
            found.setdefault(key, []).append(w)
    rows = [[] for _ in range(n)]
    for (r, c) in sorted(found):
        if mode == "mutual" and not ((r, c) in forward and (c, r) in forward):
            continue
        ws = found[(r, c)]
        best = ws[0]
        for w in ws[1:]:
            best = pick(best, w, combine)
        rows[r].append((c, best))
    return _arrays(rows, weights.dtype)


def same(got, want):
    """Three arrays against three arrays, bit for bit (dtypes included)."""
    for g, w, name in zip(got, want, ("indptr", "indices", "weights")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, np.flatnonzero(g.view(np.uint8).reshape(-1) != w.view(np.uint8).reshape(-1))[:8])


# ---------------------------------------------------------------------------------------------------------------------
# The inputs the CPU and the GPU tests share.
# ---------------------------------------------------------------------------------------------------------------------
DTYPES = (np.uint8, np.int16, np.int32, np.float16, np.float32)


def weights_of(dtype, n, seed=0):
    """n weights of `dtype` from a small set, so that equal values meet: integers with the dtype's extremes and negative
    ones among them; floats with negative values, infinities, NaNs of both signs and two payloads, -0 and +0."""
    rng = np.random.default_rng(seed + 11)
    dtype = np.dtype(dtype)
    if dtype.kind in "ui":
        info = np.iinfo(dtype)
        pool = np.array([info.min, info.max, 0, 1, 2, 3, 5, 100] + ([-1, -2, -100] if dtype.kind == "i" else [7, 8, 200]), dtype=dtype)
    else:
        u = {2: np.uint16, 4: np.uint32}[dtype.itemsize]
        nans = np.array({2: [0x7E00, 0xFE00, 0x7E01], 4: [0x7FC00000, 0xFFC00000, 0x7FC00001]}[dtype.itemsize], dtype=u).view(dtype)
        pool = np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.5, -2.5, 3.0, np.inf, -np.inf, 6e-8], dtype=dtype), nans])
    return pool[rng.integers(0, len(pool), n)]


def square_lists(nrows, negative=False):
    """The edge lists of csr_model over nrows nodes made square: columns folded into 0..nrows-1 (a graph of 19 nodes with
    rows of up to 600 entries: every column many times, self-loops absent, once and many times)."""
    indptr, indices = csr_model.edge_lists(nrows, 0, csr_model.SEED[nrows])
    folded = (indices % nrows).astype(np.int32)
    if negative:
        folded = np.where(csr_model.with_negative_columns(indptr, indices) < 0, -1, folded).astype(np.int32)
    return indptr, folded
