"""ctypes wrapper of oracle/_build/liboracle.so — TEST INFRASTRUCTURE (see oracle/oracle.c)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "liboracle.so")
_SRC = os.path.join(_HERE, "oracle.c")
_lib = None


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


def lib():
    global _lib
    if _lib is None:
        # a library older than its source would lack what the source has gained since: make knows the dependency
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(_SRC):
            build()
        # a bounded team: the GPU boxes show hundreds of CPUs but grant a share of them
        os.environ.setdefault("OMP_NUM_THREADS", str(min(32, os.cpu_count() or 1)))
        _lib = ctypes.CDLL(_SO)
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def hamming(X, Y):
    X = np.ascontiguousarray(X, dtype=np.uint8); Y = np.ascontiguousarray(Y, dtype=np.uint8)
    out = np.empty((Y.shape[0], X.shape[0]), dtype=np.int64)
    lib().orc_hamming(_p(X), ctypes.c_int64(X.shape[0]), _p(Y), ctypes.c_int64(Y.shape[0]), ctypes.c_int(X.shape[1]), _p(out))
    return out


def eps_csr(T, cmp, eps, row0=0, nrows=None, fast=False):
    """`fast`: the vectorised leg (orc_eps_fast, pinned to the scalar one by tests/test_oracle.py) for full-size checks."""
    T = np.ascontiguousarray(T, dtype=np.uint8)
    n, l = T.shape
    nrows = n - row0 if nrows is None else nrows
    counts = np.zeros(nrows, dtype=np.int64)
    args = (_p(T), ctypes.c_int64(n), ctypes.c_int(l), ctypes.c_int64(row0), ctypes.c_int64(nrows), ctypes.c_int(cmp),
            ctypes.c_double(eps))
    f = lib().orc_eps_fast if fast else lib().orc_eps
    f(*args, _p(counts), None, None, None)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = np.empty(max(int(indptr[-1]), 1), dtype=np.int32); w = np.empty(max(int(indptr[-1]), 1), dtype=np.uint8)
    f(*args, _p(counts), _p(indptr), _p(idx), _p(w))
    return indptr, idx[:indptr[-1]], w[:indptr[-1]]


def knn(T, k, row0=0, nrows=None, fast=False):
    T = np.ascontiguousarray(T, dtype=np.uint8)
    n, l = T.shape
    nrows = n - row0 if nrows is None else nrows
    idx = np.empty((nrows, k), dtype=np.int32); d = np.empty((nrows, k), dtype=np.uint8)
    f = lib().orc_knn_fast if fast else lib().orc_knn
    f(_p(T), ctypes.c_int64(n), ctypes.c_int(l), ctypes.c_int64(row0), ctypes.c_int64(nrows), ctypes.c_int(k), _p(idx), _p(d))
    return idx, d


def synth(n, l, seed, members=256):
    out = np.empty((n, l), dtype=np.uint8)
    lib().orc_synth(ctypes.c_int64(n), ctypes.c_int(l), ctypes.c_uint64(seed), ctypes.c_int64(members), _p(out))
    return out


def lev_pair(a, b, band):
    a = np.ascontiguousarray(a, dtype=np.uint8); b = np.ascontiguousarray(b, dtype=np.uint8)
    la = int(np.argmin(np.append(a, 0) != 0)); lb = int(np.argmin(np.append(b, 0) != 0))
    f = lib().orc_lev_pair
    f.restype = ctypes.c_int
    return int(f(_p(a), ctypes.c_int(la), _p(b), ctypes.c_int(lb), ctypes.c_int(band)))


def lev_knn(T, k, band=8, row0=0, nrows=None):
    T = np.ascontiguousarray(T, dtype=np.uint8)
    n, l = T.shape
    nrows = n - row0 if nrows is None else nrows
    idx = np.empty((nrows, k), dtype=np.int32); d = np.empty((nrows, k), dtype=np.uint8)
    lib().orc_lev_knn(_p(T), ctypes.c_int64(n), ctypes.c_int(l), ctypes.c_int64(row0), ctypes.c_int64(nrows),
                      ctypes.c_int(band), ctypes.c_int(k), _p(idx), _p(d))
    return idx, d


def lev_matrix(X, Y, dtype=np.int64):
    """(M, N) unbanded edit distances of the non-zero prefixes of the rows of Y against those of the rows of X
    (orc_lev_matrix): zero-right-padded uint8 rows, the two operands at their own widths of up to 2048; int32 or int64."""
    X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.uint8); Y = np.ascontiguousarray(np.atleast_2d(Y), dtype=np.uint8)
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise TypeError("lev_matrix: int32 or int64")
    if X.shape[1] > 2048 or Y.shape[1] > 2048:
        raise ValueError("lev_matrix: at most 2048 positions per operand")
    out = np.empty((Y.shape[0], X.shape[0]), dtype=dtype)
    lib().orc_lev_matrix(_p(X), ctypes.c_int64(X.shape[0]), ctypes.c_int(X.shape[1]), _p(Y), ctypes.c_int64(Y.shape[0]),
                         ctypes.c_int(Y.shape[1]), _p(out), ctypes.c_int(dtype.itemsize))
    return out


TRACE_MAX_CELLS = 1 << 19            # oracle.c's ORC_TRACE_MAX_CELLS: (len x + 1) * (len y + 1) of one pair
_TRACE_ERRORS = {1: "a pair's row number is outside its operand", 2: "a symbol outside the table",
                 3: f"a pair of more than {TRACE_MAX_CELLS} cells", 4: "ldo is below len x + len y of a pair", 5: "a bad argument",
                 6: "no memory"}


def align_trace(X, Y, xi, yi, table, gap, gap_open, mode, ldo=None):
    """(head int32 (P, 8), ops uint8 (P, ldo)) of the canonical alignments (orc_align_trace) of the pairs
    (X[xi[p]], Y[yi[p]]): zero-right-padded uint8 operands at their own widths, `table` (A, A) integers read as
    table[x symbol][y symbol], `mode` 0 global distance, 1 local, 2 semi-global, 3 fit; `ldo` defaults to the two widths
    together.  The layout is the device's: head = score, x_begin, x_end, y_begin, y_end, n_ops, identities, 0, and ops is
    zero from n_ops on.  A pair of more than TRACE_MAX_CELLS cells is refused (ValueError)."""
    X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.uint8); Y = np.ascontiguousarray(np.atleast_2d(Y), dtype=np.uint8)
    xi = np.ascontiguousarray(xi, dtype=np.int32).reshape(-1); yi = np.ascontiguousarray(yi, dtype=np.int32).reshape(-1)
    T = np.ascontiguousarray(table, dtype=np.int64)
    if T.ndim != 2 or T.shape[0] != T.shape[1] or len(xi) != len(yi):
        raise ValueError("align_trace: a square table and two lists of one length")
    ldo = X.shape[1] + Y.shape[1] if ldo is None else int(ldo)
    head = np.empty((len(xi), 8), dtype=np.int32); ops = np.empty((len(xi), ldo), dtype=np.uint8)
    f = lib().orc_align_trace
    f.restype = ctypes.c_int
    rc = f(_p(X), ctypes.c_int64(X.shape[0]), ctypes.c_int(X.shape[1]), _p(Y), ctypes.c_int64(Y.shape[0]), ctypes.c_int(Y.shape[1]),
           _p(xi), _p(yi), ctypes.c_int64(len(xi)), _p(T), ctypes.c_int(T.shape[0]), ctypes.c_int(int(gap)), ctypes.c_int(int(gap_open)),
           ctypes.c_int(int(mode)), _p(head), _p(ops), ctypes.c_int64(ldo))
    if rc:
        raise ValueError(f"align_trace: {_TRACE_ERRORS.get(rc, rc)}")
    return head, ops
