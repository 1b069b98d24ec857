"""
Levenshtein (edit) distance over tokenised, zero right-padded sequences — NOT in the reference
(acmater/prograph ships only hamming / minkowski); defined by this build.

`levenshtein(X (N,D1), Y (M,D2), similarity=False) -> (M,N)` follows the operator protocol of `hamming`: row m is
Y[m] against every row of X, `torch.int64`, on the device of the inputs; `ValueError` on an empty operand;
`similarity=True` returns 1/(1+d).

    * a row's sequence is the row with its trailing zeros removed (an all-zero row is the empty sequence), so the zero
      padding `clean_input` adds to the narrower operand changes nothing;
    * the remaining values are symbols compared by equality (an interior zero is an ordinary symbol); substitution,
      insertion and deletion cost 1; there is no band and no cap: d(empty, b) = len(b);
    * values must be integers in 0..255 (any dtype): anything else raises `ValueError`.

Device operands with tokens up to 31 and zeros only as trailing padding run on the HIP kernels: up to 128 positions
`pg_levenshtein_dense` (prograph_amd/csrc/pg_lev.hip), from 129 to 2048 positions `pg_levenshtein_long_dense`
(prograph_amd/csrc/pg_lev_long.hip).  Everything else - larger tokens, interior zeros, more than 2048 positions, CPU
tensors - is evaluated by the torch expression below, on the device the operands live on: the Wagner-Fischer table row
by row over the whole (M, N) batch, the
dependency inside a row resolved by v[j] = j + cummin(c[k] - k).  It is the slow path; it is exact.

`levenshtein_knn` is the banded (capped) kNN of BASELINE.json configs[4]: d = min(edit distance, band+1), canonical
(d, index) order, rank 0 dropped.

There is no `align` here: the edit script of a pair is `alignment(1 - I, 1).align(X, Y)`, I the identity over the alphabet
(prograph_amd/alignments.py).
"""
import torch

from .. import _native
from .hamming import _as_byte_tokens
from .utils import clean_input

_DP_ELEMS = 1 << 24            # table entries (pairs x columns) alive per block of the torch expression


def levenshtein_knn(tokens, k, band=8, **kw):
    return _native.levenshtein_knn(tokens, k, band=band, **kw)


def _lengths(T):
    """(R,) int64: index of the last non-zero + 1."""
    pos = torch.arange(1, T.shape[1] + 1, device=T.device, dtype=torch.int32)
    return ((T != 0) * pos).amax(dim=1).to(torch.int64)


def _dp_block(x, lx, y, ly):
    """(m, n) int64 edit distances of y rows (lengths ly) against x rows (lengths lx); x, y already cut to the longest
    sequence among their rows."""
    m, n, dx = y.shape[0], x.shape[0], x.shape[1]
    j = torch.arange(dx + 1, device=x.device, dtype=torch.int32)
    v = j.expand(m, n, dx + 1).contiguous()                              # row 0 of every table: D[0][j] = j
    at = lx.view(1, n, 1).expand(m, n, 1)
    res = v.gather(2, at).squeeze(2)                                     # empty y: d = len(x)
    for i in range(1, y.shape[1] + 1):
        ne = (y[:, i - 1].view(m, 1, 1) != x.view(1, n, dx)).to(torch.int32)
        c = torch.empty_like(v)
        c[..., 0] = i
        c[..., 1:] = torch.minimum(v[..., 1:] + 1, v[..., :-1] + ne)     # deletion | substitution or match
        v = torch.cummin(c - j, dim=2).values + j                        # insertions: min over k <= j of c[k] + (j - k)
        res = torch.where((ly == i).view(m, 1), v.gather(2, at).squeeze(2), res)
    return res.to(torch.int64)


def _torch_levenshtein(X, Y):
    """The definition as a torch expression: X (N, D), Y (M, D) uint8 on one device -> (M, N) int64."""
    lx, ly = _lengths(X), _lengths(Y)
    X, Y = X[:, :int(lx.max())], Y[:, :int(ly.max())]
    n, m = X.shape[0], Y.shape[0]
    cols = max(1, min(n, _DP_ELEMS // (X.shape[1] + 1)))
    rows = max(1, min(m, _DP_ELEMS // (cols * (X.shape[1] + 1))))
    out = torch.empty((m, n), dtype=torch.int64, device=X.device)
    for r0 in range(0, m, rows):
        for c0 in range(0, n, cols):
            out[r0:r0 + rows, c0:c0 + cols] = _dp_block(X[c0:c0 + cols], lx[c0:c0 + cols], Y[r0:r0 + rows], ly[r0:r0 + rows])
    return out


def _on_device(T):
    """Do the tokens live where the kernels run?  (One place to ask, which the host-logic tests patch.)"""
    return T.is_cuda


def levenshtein(X, Y, similarity=False):
    """(M, N) edit distances (or similarities 1/(1+d)) of the M rows of Y against the N rows of X, int64."""
    X, Y = clean_input(X, Y)
    Y = Y.to(X.device)
    xb = _as_byte_tokens(X)
    yb = xb if Y is X else _as_byte_tokens(Y)
    if xb is None or yb is None:
        raise ValueError("levenshtein: the symbols must be integers in 0..255")
    d = None
    if _on_device(xb) and xb.shape[1] <= 128:
        xo = _native.lev_operand(xb)
        yo = xo if yb is xb else _native.lev_operand(yb)
        if xo.valid() and yo.valid():                                    # tokens <= 31, zeros trailing only
            d = _native.levenshtein_dense(xo, yo, out_bytes=8)
    elif _on_device(xb) and xb.shape[1] <= _native.LEV_LONG_MAX_L and _native.lev_long_ready():
        xo = _native.lev_long_operand(xb)
        yo = xo if yb is xb else _native.lev_long_operand(yb)
        if xo.valid() and yo.valid():
            d = _native.levenshtein_long_dense(xo, yo, out_bytes=8)
    if d is None:
        d = _torch_levenshtein(xb, yb)
    return 1 / (1 + d) if similarity else d
