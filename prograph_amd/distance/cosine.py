"""
Cosine distance operator.  The reference exports `cosine` (prograph/distance/__init__.py) but its module only
prints "Add method."; this is the operator its README's to-do list asks for, with the reference's similarity
line, s = 1/(1+d).

Non-empty 2-D fp16 device tensors with finite elements - what `build_graph(representation="Embedded",
distance=cosine)` stages (prograph/prograph.py:726 of the reference) - run on the matrix-core kernels
(`pg_cosine_prep` + `pg_cosine_dense`, prograph_amd/csrc/pg_cos.hip).  Everything else is evaluated by the torch
expression below, in fp32 on the device the operands live on, with the same three rules:

    d = 1                           if ||x||^2 == 0 or ||y||^2 == 0
      = 0                           if x.y == ||x||^2 == ||y||^2 bitwise (identical vectors)
      = clamp(1 - (x.y / ||y||) / ||x||, 0, 2)   with the reciprocal roots rounded once per vector
"""
import torch

from .. import _native
from .utils import clean_input


def _torch_cosine(X, Y, similarity):
    Xf, Yf = X.to(torch.float32), Y.to(torch.float32)
    p = Yf @ Xf.T
    nx, ny = (Xf * Xf).sum(1), (Yf * Yf).sum(1)
    rx, ry = 1 / torch.sqrt(nx), 1 / torch.sqrt(ny)
    d = torch.clamp(1 - (p * ry[:, None]) * rx[None, :], 0, 2)
    d = torch.where((p == nx[None, :]) & (p == ny[:, None]), torch.zeros_like(d), d)
    d = torch.where((nx[None, :] == 0) | (ny[:, None] == 0), torch.ones_like(d), d)
    return 1 / (1 + d) if similarity else d


def _native_ok(X, Y):
    return all(t.dtype == torch.float16 and t.dim() == 2 and t.is_cuda and t.shape[0] > 0 and t.shape[1] > 0 for t in (X, Y))


def cosine(X, Y, similarity=False):
    """(M, N) cosine distances (or similarities 1/(1+d)) of the M rows of Y against the N rows of X, float32."""
    X, Y = clean_input(X, Y)
    if _native_ok(X, Y):
        xc = _native.cosine_prep(X)
        yc = xc if Y is X else _native.cosine_prep(Y)
        if not (xc.nonfinite() or yc.nonfinite()):
            return _native.cosine_dense(xc, yc, similarity=similarity)
    return _torch_cosine(X, Y, similarity)
