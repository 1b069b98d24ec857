"""
The yardstick of the `Prograph.rescore` tests (tests/test_rescore_cpu.py, tests/test_alignment_list_gpu.py): a candidate graph
as host CSR arrays, and the selection over its values in plain NumPy, row by row - a stable sort by column, then a stable
sort by value.  Nothing under prograph_amd/ imports this file.
"""
import numpy as np


def random_csr(rng, nrows, ncols, most, own_row=True):
    """A seeded candidate graph: per row 0..most distinct columns in random order (the row itself among them now and then),
    rows 0 and 1 forced to the extremes (no edge, `most` edges)."""
    lens = rng.integers(0, most + 1, nrows)
    lens[0], lens[1 % nrows] = 0, min(most, ncols)
    cols = []
    for r in range(nrows):
        c = rng.permutation(ncols)[:lens[r]]
        if own_row and len(c) and r % 3 == 0:
            c[0] = r if r not in c else c[0]
        cols.append(c.astype(np.int64))
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    return indptr, (np.concatenate(cols) if indptr[-1] else np.zeros(0, dtype=np.int64))


def row_lists(indptr, cols, values):
    """[(columns, values)] per row, in the graph's order."""
    return [(cols[indptr[r]:indptr[r + 1]], values[indptr[r]:indptr[r + 1]]) for r in range(len(indptr) - 1)]


def knn(indptr, cols, values, k, descending):
    """(idx, w) (nrows, k): per row the first k candidates of the stable (value, column) order, -1 / 0 beyond them."""
    n = len(indptr) - 1
    idx, w = np.full((n, k), -1, dtype=np.int64), np.zeros((n, k), dtype=np.int64)
    for r, (c, v) in enumerate(row_lists(indptr, cols, values)):
        by_col = np.argsort(c, kind="stable")
        c, v = c[by_col], v[by_col]
        order = np.argsort(-v if descending else v, kind="stable")[:k]
        idx[r, :len(order)], w[r, :len(order)] = c[order], v[order]
    return idx, w


def eps(indptr, cols, values, keep):
    """(indptr, columns ascending, values) of the candidates with keep(values)."""
    out, cs, vs = [0], [], []
    for c, v in row_lists(indptr, cols, values):
        by_col = np.argsort(c, kind="stable")
        c, v = c[by_col], v[by_col]
        m = keep(v)
        cs.append(c[m])
        vs.append(v[m])
        out.append(out[-1] + int(m.sum()))
    return (np.asarray(out, dtype=np.int64), np.concatenate(cs) if cs else np.zeros(0, dtype=np.int64),
            np.concatenate(vs) if vs else np.zeros(0, dtype=np.int64))


def knn_equals(g, want, first):
    idx, w = want
    assert g.idx.dtype.is_signed and g.dist.shape == g.idx.shape == idx.shape and g.first == first
    assert np.array_equal(g.idx.cpu().numpy(), idx) and np.array_equal(g.dist.cpu().numpy(), w)


def csr_equals(g, want):
    indptr, cols, vals = want
    assert np.array_equal(g.indptr.cpu().numpy(), indptr)
    assert np.array_equal(g.indices.cpu().numpy(), cols) and np.array_equal(g.weights.cpu().numpy(), vals)
