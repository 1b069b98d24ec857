"""
TEST-ONLY stand-in for the alignment entry points of prograph_amd._native (on top of tests/fake_native.py): answers them
from the recurrence in numpy on CPU tensors, so that the host logic of `build_graph(distance=alignment(C, gap))` and
`search` - route choice, block sizes, selection arguments, containers, dtypes - runs without a GPU.  Nothing under
prograph_amd/ imports it.  `calls` records which entry points ran and with what.

`recurrence` below is the same double loop as `definition` in tests/test_alignment_cpu.py, so the two share any mistake:
what the tests prove through this stand-in is the host logic around the kernel, not the recurrence.  The recurrence itself
is checked where the fake is not involved: the torch expression against `definition` and against `levenshtein` /
`substitution` on the CPU, and the kernel against `definition` on the GPU.
"""
import numpy as np
import torch

import fake_native
import fake_sub_native
from prograph_amd import _native

calls = []


class FakeAlnOperand:
    def __init__(self, tokens, a):
        self.tokens = tokens if isinstance(tokens, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tokens))
        assert self.tokens.dtype == torch.uint8 and self.tokens.dim() == 2 and self.tokens.shape[1] <= _native.ALN_MAX_L
        self.n, self.l = self.tokens.shape
        self.a, self.npad, self.buf = int(a), _native.npad(self.n), torch.zeros(1, dtype=torch.int32)
        calls.append(("operand", self.n, self.l, self.a))

    def valid(self):
        return bool(self.tokens.max() < self.a)


def _lengths(T):
    return np.where(T != 0, np.arange(1, T.shape[1] + 1), 0).max(axis=1, initial=0)


def recurrence(C, gap, X, Y):
    """(M, N) int64 alignment distances of the rows of Y against the rows of X (trailing zeros are padding)."""
    lx, ly = _lengths(X), _lengths(Y)
    M, N, LX = len(Y), len(X), X.shape[1]
    H = np.empty((LX + 1, M, N), dtype=np.int64)
    H[:] = (np.arange(LX + 1) * gap)[:, None, None]
    at = np.broadcast_to(lx[None, None, :], (1, M, N))
    out = np.take_along_axis(H, at, 0)[0].copy()
    for i in range(1, int(ly.max(initial=0)) + 1):
        cy = C[Y[:, i - 1]]
        diag = H[0].copy()
        H[0] = i * gap
        for j in range(1, LX + 1):
            up = H[j].copy()
            H[j] = np.minimum(diag + cy[:, X[:, j - 1]], np.minimum(up, H[j - 1]) + gap)
            diag = up
        done = ly == i
        out[done] = np.take_along_axis(H, at, 0)[0][done]
    return out


def _dense(xo, yo, cost, gap, out_bytes=8, rows=None):
    r0, r1 = (0, yo.n) if rows is None else rows
    calls.append(("dense", r1 - r0, out_bytes, int(gap)))
    d = recurrence(cost.numpy(), int(gap), xo.tokens.numpy().astype(np.intp), yo.tokens.numpy()[r0:r1].astype(np.intp))
    return torch.from_numpy(d).to({2: torch.float16, 8: torch.int64}[out_bytes])


def _f16_knn(block, k, first=1, descending=False):
    calls.append(("f16_knn", k, first, descending))
    return fake_native._f16_knn(block, k, first=first, descending=descending)


def _f16_eps(block, cmp, eps, similarity=False, keep_zero=False):
    calls.append(("f16_eps", cmp, float(eps), similarity, keep_zero))
    d = block.to(torch.float32)
    keep = fake_native._OPS[cmp](d, float(np.float16(eps))) & ((d >= 0) if keep_zero else (d > 0))
    rows, cols = torch.where(keep)
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(keep.sum(dim=1), 0)])
    return indptr, cols.to(torch.int32), block[rows, cols]


def install(monkeypatch):
    fake_native.install(monkeypatch)
    del calls[:]
    monkeypatch.setattr(_native, "aln_operand", FakeAlnOperand)
    monkeypatch.setattr(_native, "sub_cost", fake_sub_native._cost)
    monkeypatch.setattr(_native, "alignment_dense", _dense)
    monkeypatch.setattr(_native, "f16_knn", _f16_knn)
    monkeypatch.setattr(_native, "f16_eps", _f16_eps)
