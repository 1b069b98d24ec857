"""
TEST-ONLY stand-in for the three graph operations of prograph_amd._native (`csr_sort_rows`, `csr_transpose`, `csr_symmetrize`),
in the manner of tests/fake_native.py: NumPy on CPU tensors, so that the containers and `Prograph.symmetrize` can be exercised on
a box without a GPU.  Vectorised sorts and group reductions - no code shared with tests/graph_ops_model.py, which it is held
against (tests/test_graph_ops_cpu.py).  Nothing under prograph_amd/ imports this file; the product has no CPU path.
"""
import numpy as np
import torch

from prograph_amd import _native

_UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _np(indptr, indices, weights):
    return indptr.numpy().astype(np.int64), indices.numpy().astype(np.int64), np.ascontiguousarray(weights.numpy())


def _out(rows, nrows, cols, w):
    indptr = np.zeros(nrows + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=nrows))
    return torch.from_numpy(indptr), torch.from_numpy(cols.astype(np.int32)), torch.from_numpy(np.ascontiguousarray(w))


def _coo(indptr, indices, ncols):
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    real = (indices >= 0) & (indices < ncols)
    return rows[real], indices[real], np.flatnonzero(real)


def csr_sort_rows(indptr, indices, weights, ncols, trim=True):
    ip, ix, w = _np(indptr, indices, weights)
    rows, cols, at = _coo(ip, ix, int(ncols))
    order = np.argsort(rows * max(int(ncols), 1) + cols, kind="stable")
    return _out(rows[order], len(ip) - 1, cols[order], w[at[order]])


def csr_transpose(indptr, indices, weights, ncols, row0=0, trim=True):
    ip, ix, w = _np(indptr, indices, weights)
    rows, cols, at = _coo(ip, ix, int(ncols))
    order = np.argsort(cols, kind="stable")
    return _out(cols[order], int(ncols), rows[order] + int(row0), w[at[order]])


def csr_symmetrize(indptr, indices, weights, mode="union", combine="min"):
    if mode not in _native.SYM_MODES or combine not in _native.SYM_COMBINES:
        raise ValueError("mode is 'union' or 'mutual', combine is 'min' or 'max'")
    ip, ix, w = _np(indptr, indices, weights)
    n = len(ip) - 1
    rows, cols, at = _coo(ip, ix, n)
    w = w[at]
    bits = w.view(_UNSIGNED[w.dtype.itemsize]).astype(np.int64)
    off = rows != cols                                                  # a self-loop is its own reverse: it enters once
    key = np.concatenate([rows * n + cols, (cols * n + rows)[off]])
    bits = np.concatenate([bits, bits[off]])
    value = np.concatenate([w, w[off]]).astype(np.float64)              # exact for every dtype the containers carry
    side = np.concatenate([np.ones(len(rows), np.int64), np.full(int(off.sum()), 2, np.int64)])
    side[:len(rows)][~off] = 3
    nan = np.isnan(value)
    rank = np.where(nan, 0.0, value if combine == "min" else -value)    # ascending: the winner first
    order = np.lexsort((bits, rank, nan, key))
    key, bits, side = key[order], bits[order], side[order]
    head = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, np.int64)
    sides = np.bitwise_or.reduceat(side, head) if len(head) else side[:0]
    keep = np.ones(len(head), bool) if mode == "union" else sides == 3
    key, bits = key[head][keep], bits[head][keep]
    wout = bits.astype(_UNSIGNED[w.dtype.itemsize]).view(w.dtype)
    return _out(key // max(n, 1), n, key % max(n, 1), wout)


def install(monkeypatch):
    monkeypatch.setattr(_native, "csr_sort_rows", csr_sort_rows)
    monkeypatch.setattr(_native, "csr_transpose", csr_transpose)
    monkeypatch.setattr(_native, "csr_symmetrize", csr_symmetrize)
