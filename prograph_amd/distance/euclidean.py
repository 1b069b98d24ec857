"""
Euclidean (L2) distance operator for embeddings, in fp32 on the matrix cores, with the reference's similarity line
s = 1/(1+d).  `minkowski` reproduces the reference's fp16 tensor expression - every step rounded to fp16, a sum of
squares above 65 504 is inf -; this is a metric of its own with a contract of its own.

Non-empty 2-D fp16 device tensors with finite elements - what `build_graph(representation="Embedded",
distance=euclidean)` stages - run on the matrix-core kernels (`pg_cosine_prep` + `pg_euclidean_dense`,
prograph_amd/csrc/pg_cos.hip): p = x.y, nx = ||x||^2, ny = ||y||^2 are fp32 sums of exact fp16 products, and

    d = 0                                   if p == nx == ny bitwise (identical vectors, two zero vectors)
      = sqrt(max((nx + ny) - (p + p), 0))   otherwise: every step rounded to fp32, the root correctly rounded
    s = 1 / (1 + d)

Everything else is evaluated by the torch expression below, in fp32 on the device the operands live on, with the same
rules.  A zero vector is an ordinary point, d(0, y) = sqrt(ny), and no finite fp16 input overflows.

Stated tolerance.  The form cancels, so the error is absolute in the norms: against the exact d^2 of the fp16 values

    |d_hat^2 - d^2| <= B(D) (nx + ny) + 2^-22 d^2,      B(D) = 2 D 2^-24 + 2^-21.

A non-identical pair whose true d^2 lies below B(D) (nx + ny) - a near-duplicate - may therefore come out as 0 or with
a large relative error; typical neighbours are far above that level.
"""
import torch

from .. import _native
from .utils import clean_input


def _torch_euclidean(X, Y, similarity):
    Xf, Yf = X.to(torch.float32), Y.to(torch.float32)
    p = Yf @ Xf.T
    nx, ny = (Xf * Xf).sum(1), (Yf * Yf).sum(1)
    d = torch.sqrt(torch.clamp((nx[None, :] + ny[:, None]) - (p + p), min=0))
    d = torch.where((p == nx[None, :]) & (p == ny[:, None]), torch.zeros_like(d), d)
    return 1 / (1 + d) if similarity else d


def _native_ok(X, Y):
    return all(t.dtype == torch.float16 and t.dim() == 2 and t.is_cuda and t.shape[0] > 0 and t.shape[1] > 0 for t in (X, Y))


def euclidean(X, Y, similarity=False):
    """(M, N) Euclidean distances (or similarities 1/(1+d)) of the M rows of Y against the N rows of X, float32."""
    X, Y = clean_input(X, Y)
    if _native_ok(X, Y):
        xc = _native.cosine_prep(X)
        yc = xc if Y is X else _native.cosine_prep(Y)
        if not (xc.nonfinite() or yc.nonfinite()):
            return _native.euclidean_dense(xc, yc, similarity=similarity)
    return _torch_euclidean(X, Y, similarity)
