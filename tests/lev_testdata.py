"""
Inputs and oracle-side references shared by the Levenshtein tests (CPU and GPU).

Set A: 1000 clustered variable-length rows (lengths 96..128, clusters of 50) plus 60 unrelated rows (uniform tokens
1..20, lengths 40..128), permuted.  Properties the tests rely on - and assert from the oracle's results, so that a
changed generator cannot make them vacuous: for k = 16 most rows have their 16th neighbour within 8 edits and the
unrelated ones do not; duplicates occur; no row has 63 neighbours within 8 edits.
"""
import operator

import numpy as np

from oracle import c_oracle as C
from prograph_amd import synth


def set_a():
    tok, _ = synth.clustered_varlen_tokens(1000, Lmax=128, Lmin=96, members=50)
    rng = np.random.default_rng(7)
    extra = np.zeros((60, 128), dtype=np.uint8)
    for i in range(60):
        l = int(rng.integers(40, 129))
        extra[i, :l] = rng.integers(1, 21, l)
    T = np.concatenate([tok, extra])
    return np.ascontiguousarray(T[rng.permutation(len(T))])


def pair_matrix(X, Y):
    """(M, N) unbanded distances from the C oracle, pair by pair."""
    return np.array([[C.lev_pair(y, x, 128) for x in X] for y in Y], dtype=np.int64)


def csr_from_banded(T, comp, eps):
    """The epsilon graph (0 < d, comp(d, eps)), eps <= 8, from the oracle's banded kNN lists: complete because no row has
    a 63rd rank within the band (asserted)."""
    idx, d = C.lev_knn(T, 63, band=8)
    assert (d[:, 62] > 8).all(), "a row has 63 in-band neighbours: the lists are not the whole neighbourhood"
    indptr, cols, wts = [0], [], []
    for i in range(len(T)):
        keep = (d[i] <= 8) & (d[i] > 0) & comp(d[i].astype(np.int64), eps)
        o = np.argsort(idx[i][keep], kind="stable")
        cols.append(idx[i][keep][o]); wts.append(d[i][keep][o])
        indptr.append(indptr[-1] + int(keep.sum()))
    return np.array(indptr, dtype=np.int64), np.concatenate(cols).astype(np.int32), np.concatenate(wts).astype(np.uint8)


def csr_from_matrix(D, comp, eps, keep_zero=False):
    keep = comp(D, eps) & ((D >= 0) if keep_zero else (D > 0))
    r, c = np.nonzero(keep)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    return indptr, c.astype(np.int32), D[r, c].astype(np.uint8)


def knn_from_matrix(D, k, first):
    order = np.argsort(D, axis=1, kind="stable")[:, first:first + k]
    return order.astype(np.int32), np.take_along_axis(D, order, 1).astype(np.uint8)


OPS = {"le": operator.le, "lt": operator.lt, "eq": operator.eq, "ge": operator.ge, "gt": operator.gt}
