"""
TEST-ONLY stand-in for the Levenshtein entry points of prograph_amd._native (on top of tests/fake_native.py): answers
them from the C oracle on CPU tensors, so that the host logic of `build_graph(distance=levenshtein)` and `search` -
route choice, the hybrid kNN merge, containers, dtypes - runs without a GPU.  Nothing under prograph_amd/ imports it.
`calls` records which entry points ran and over how many rows.
"""
import numpy as np
import torch

import fake_native
from oracle import c_oracle as C
from prograph_amd import _native

calls = []


class FakeLevOperand:
    def __init__(self, tokens):
        self.tokens = tokens if isinstance(tokens, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tokens))
        assert self.tokens.dtype == torch.uint8 and self.tokens.dim() == 2 and self.tokens.shape[1] <= 128
        self.n, self.l = self.tokens.shape

    def valid(self):
        t = self.tokens.numpy()
        lens = (t != 0).sum(1)
        return bool(t.max() <= 31) and all((r[:l] != 0).all() for r, l in zip(t, lens))


def _matrix(xo, yo, rows):
    X, Y = xo.tokens.numpy(), yo.tokens.numpy()[rows[0]:rows[1]]
    return np.array([[C.lev_pair(y, x, 128) for x in X] for y in Y], dtype=np.int64)


def _dense(xo, yo, out_bytes=8, rows=None):
    rows = (0, yo.n) if rows is None else rows
    calls.append(("dense", rows[1] - rows[0]))
    return torch.from_numpy(_matrix(xo, yo, rows)).to({2: torch.float16, 8: torch.int64}[out_bytes])


def _eps(op, cmp, thr, cap=512, keep_zero=False):
    calls.append(("eps", op.n))
    assert cmp in (_native.CMP_LE, _native.CMP_LT, _native.CMP_EQ) and 0 <= thr <= 8
    d = _matrix(op, op, (0, op.n))
    np.fill_diagonal(d, -1)                                             # the row itself is no candidate
    keep = fake_native._OPS[cmp](d, thr) & (d >= (0 if keep_zero else 1))
    r, c = np.nonzero(keep)
    indptr = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64)
    return torch.from_numpy(indptr), torch.from_numpy(c.astype(np.int32)), torch.from_numpy(d[r, c].astype(np.uint8))


def _knn(tokens, k, band=8, **kw):
    calls.append(("banded_knn", int(tokens.shape[0])))
    idx, d = C.lev_knn(tokens.numpy(), k, band=band)
    return torch.from_numpy(idx), torch.from_numpy(d)


def _f16_eps(block, cmp, eps, similarity=False, keep_zero=False):
    d = block.to(torch.float32)
    keep = fake_native._OPS[cmp](d, float(np.float16(eps))) & ((d >= 0) if keep_zero else (d > 0))
    rows, cols = torch.where(keep)
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(keep.sum(dim=1), 0)])
    return indptr, cols.to(torch.int32), block[rows, cols]


def install(monkeypatch):
    fake_native.install(monkeypatch)
    del calls[:]
    monkeypatch.setattr(_native, "lev_operand", FakeLevOperand)
    monkeypatch.setattr(_native, "levenshtein_dense", _dense)
    monkeypatch.setattr(_native, "levenshtein_eps", _eps)
    monkeypatch.setattr(_native, "levenshtein_knn", _knn)
    monkeypatch.setattr(_native, "f16_eps", _f16_eps)
