"""
TEST-ONLY stand-in for the substitution entry points of prograph_amd._native (on top of tests/fake_native.py): answers
them from the definition in numpy on CPU tensors, so that the host logic of `build_graph(distance=substitution(C))` and
`search` - route choice, block sizes, selection arguments, containers, dtypes - runs without a GPU.  Nothing under
prograph_amd/ imports it.  `calls` records which entry points ran and with what.
"""
import numpy as np
import torch

import fake_native
from prograph_amd import _native

calls = []


class FakeSubOperand:
    def __init__(self, tokens, a):
        self.tokens = tokens if isinstance(tokens, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tokens))
        assert self.tokens.dtype == torch.uint8 and self.tokens.dim() == 2 and self.tokens.shape[1] <= _native.SUB_MAX_L
        self.n, self.l = self.tokens.shape
        self.a, self.npad, self.buf = int(a), _native.npad(self.n), torch.zeros(1, dtype=torch.int32)
        calls.append(("operand", self.n, self.l, self.a))

    def valid(self):
        return bool(self.tokens.max() < self.a)


def _cost(table):
    t = np.zeros((32, 32), dtype=np.int64)
    t[:len(table), :len(table)] = np.asarray(table)
    return torch.from_numpy(t)


def _dense(xo, yo, cost, out_bytes=8, rows=None, out=None, cols=None):
    assert xo.l == yo.l and out is None and cols is None
    r0, r1 = (0, yo.n) if rows is None else rows
    calls.append(("dense", r1 - r0, out_bytes))
    C, X, Y = cost.numpy(), xo.tokens.numpy().astype(np.intp), yo.tokens.numpy()[r0:r1].astype(np.intp)
    d = C[Y[:, None, :], X[None, :, :]].sum(-1)
    return torch.from_numpy(d).to({2: torch.float16, 4: torch.int32, 8: torch.int64}[out_bytes])


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
    monkeypatch.setattr(_native, "sub_operand", FakeSubOperand)
    monkeypatch.setattr(_native, "sub_cost", _cost)
    monkeypatch.setattr(_native, "substitution_dense", _dense)
    monkeypatch.setattr(_native, "f16_knn", _f16_knn)
    monkeypatch.setattr(_native, "f16_eps", _f16_eps)
