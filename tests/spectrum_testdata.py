"""
The k-mer spectrum's definition for the tests, written with `collections.Counter` and Python integers
only - no torch, no package code: window i of a row counts iff none of its k tokens is 0; its code is the window read in
base `symbols`; the bucket is the code (exact) or (((code + 1) * 2654435761) mod 2^32) >> (32 - log2 dims) (hashed).
"""
import operator
from collections import Counter

import numpy as np

HASH_MUL = 2654435761


def width_of(k, symbols, dims):
    return dims if dims else symbols ** k


def bucket_of(code, dims):
    if not dims:
        return code
    return (((code + 1) * HASH_MUL) % (1 << 32)) >> (32 - (dims.bit_length() - 1))


def profile(row, k, symbols, dims=0):
    """int64 [D] counts of one token row (any integer sequence): the buckets of the counting windows, counted by a
    Counter.  Short rows go window by window in Python integers; long ones form the same codes with int64 numpy
    arithmetic first ((code + 1) * 2654435761 < 2^63), so that the tests' reference stays quick."""
    row = [int(t) for t in row]
    c = Counter()
    if len(row) <= 80:
        for i in range(len(row) - k + 1):
            w = row[i:i + k]
            if all(w):
                code = 0
                for t in w:
                    code = code * symbols + (t - 1)
                c[bucket_of(code, dims)] += 1
    else:
        w = np.lib.stride_tricks.sliding_window_view(np.array(row, dtype=np.int64), k)
        code = ((w - 1) * np.array([symbols ** (k - 1 - j) for j in range(k)], dtype=np.int64)).sum(1)[(w != 0).all(1)]
        if dims:
            code = (((code + 1) * HASH_MUL) % (1 << 32)) >> (32 - (dims.bit_length() - 1))
        c.update(code.tolist())
    out = np.zeros(width_of(k, symbols, dims), dtype=np.int64)
    for b, v in c.items():
        out[b] = v
    return out


def profiles(T, k, symbols, dims=0):
    """int64 (N, D) counts of the rows of a token matrix; equal rows are counted once."""
    seen = {}
    out = np.zeros((len(T), width_of(k, symbols, dims)), dtype=np.int64)
    for r, row in enumerate(np.asarray(T)):
        key = row.tobytes()
        if key not in seen:
            seen[key] = profile(row, k, symbols, dims)
        out[r] = seen[key]
    return out


def d2_of(px, py):
    """int64 (M, N) exact squared Euclidean distances of the rows of py against the rows of px."""
    px, py = px.astype(np.int64), py.astype(np.int64)
    nx, ny = (px * px).sum(1), (py * py).sum(1)
    return nx[None, :] + ny[:, None] - 2 * (py @ px.T)


def euclid_of(d2):
    """float32(sqrt(d2)), correctly rounded: d2 < 2^24 is exact in float32 and IEEE's square root rounds correctly."""
    assert d2.min() >= 0 and d2.max() < 1 << 24
    return np.sqrt(d2.astype(np.float32))


def sim_of(d):
    """1 / (1 + d) in float32, each step correctly rounded (numpy's float32 arithmetic is IEEE)."""
    return (np.float32(1) / (np.float32(1) + d.astype(np.float32))).astype(np.float32)


def knn_oracle(d2, k, first, similarity=False):
    """Ranks first..first+k-1 of every row in the stable order of (d2, column) - for similarities of (-s, column), s =
    1/(1+d) - : columns int32 (M, k) and the float32 weights (d or s); ranks beyond the row are -1 / 0."""
    m, n = d2.shape
    idx = np.full((m, k), -1, dtype=np.int32)
    w = np.zeros((m, k), dtype=np.float32)
    vals = sim_of(euclid_of(d2)) if similarity else euclid_of(d2)
    order = np.argsort(-vals if similarity else d2, axis=1, kind="stable")[:, first:first + k]
    idx[:, :order.shape[1]] = order
    w[:, :order.shape[1]] = np.take_along_axis(vals, order, 1)
    return idx, w


def eps_oracle(d, comp, eps, keep_zero, similarity=False):
    """CSR (indptr, indices, weights) of where(comp(d, eps) & (d > 0)) over a float32 (M, N) block, `eps` rounded to
    float32 first; similarities: where(comp(1/(1+eps), s) & (s < 1)) with s = 1/(1+d)."""
    if similarity:
        s = sim_of(d)
        hit = comp(np.float32(1 / (1 + eps)), s)
        if not keep_zero:
            hit &= s < 1
        vals = s
    else:
        hit = comp(d, np.float32(eps))
        if not keep_zero:
            hit &= d > 0
        vals = d
    rows, cols = np.nonzero(hit)
    indptr = np.zeros(d.shape[0] + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(hit.sum(1))
    return indptr, cols.astype(np.int32), vals[rows, cols]


COMPS = [operator.le, operator.lt, operator.eq, operator.ge, operator.gt]
