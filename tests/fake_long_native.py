"""
TEST-ONLY stand-in for the entry points of the alignment kernels beyond 128 positions (`_native.aln_long_operand`,
`alignment_long_dense`, `alignment_local_long_dense`, `i32_knn`, `i32_eps`), layered on tests/fake_affine_native.py and
tests/fake_local_native.py: the same `calls` list, the answers from their `recurrence` functions on CPU tensors, and
`aln_long_ready` patched to True, so that the host logic of the long routes - route choice, block sizes, selection
arguments, containers, dtypes - runs without a GPU.  Nothing under prograph_amd/ imports it.
"""
import numpy as np
import torch

import fake_affine_native
import fake_local_native
import fake_native
from fake_aln_native import calls
from prograph_amd import _native


class FakeLongOperand:
    def __init__(self, tokens, a):
        self.tokens = tokens if isinstance(tokens, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tokens))
        assert self.tokens.dtype == torch.uint8 and self.tokens.dim() == 2 and self.tokens.shape[1] <= _native.ALN_LONG_MAX_L
        self.n, self.l = self.tokens.shape
        self.a, self.npad, self.buf = int(a), _native.npad(self.n), torch.zeros(1, dtype=torch.int32)
        self.flags = torch.zeros(1, dtype=torch.int32) + int(self.tokens.max() >= self.a)
        calls.append(("long_operand", self.n, self.l, self.a))


def _block(name, recurrence, xo, yo, table, gap, gap_open, out_bytes, rows):
    assert isinstance(xo, FakeLongOperand) and isinstance(yo, FakeLongOperand) and out_bytes in (4, 8)
    r0, r1 = (0, yo.n) if rows is None else rows
    calls.append((name, r1 - r0, out_bytes, int(gap), int(gap_open)))
    d = recurrence(table.numpy(), int(gap), int(gap_open), xo.tokens.numpy().astype(np.intp),
                   yo.tokens.numpy()[r0:r1].astype(np.intp))
    return torch.from_numpy(d).to({4: torch.int32, 8: torch.int64}[out_bytes])


def _long_dense(xo, yo, cost, gap, gap_open, out_bytes=8, rows=None):
    return _block("long_dense", fake_affine_native.recurrence, xo, yo, cost, gap, gap_open, out_bytes, rows)


def _local_long_dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None):
    return _block("local_long_dense", fake_local_native.recurrence, xo, yo, score, gap, gap_open, out_bytes, rows)


def _i32_knn(block, k, first=1, descending=False):
    assert block.dtype == torch.int32
    calls.append(("i32_knn", k, first, descending))
    s = torch.sort(block.to(torch.int64), dim=1, descending=bool(descending), stable=True)
    return s[1][:, first:first + k].to(torch.int32), s[0][:, first:first + k].to(torch.int32)


def _i32_eps(block, cmp, thr, keep_zero=False):
    assert block.dtype == torch.int32 and isinstance(thr, int)
    calls.append(("i32_eps", cmp, thr, keep_zero))
    keep = fake_native._OPS[cmp](block.to(torch.int64), thr) & ((block >= 0) if keep_zero else (block > 0))
    rows, cols = torch.where(keep)
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(keep.sum(dim=1), 0)])
    return indptr, cols.to(torch.int32), block[rows, cols]


def install(monkeypatch, ready=True):
    fake_affine_native.install(monkeypatch)
    fake_local_native.install(monkeypatch)                     # both sit on fake_aln_native: one `calls` list
    monkeypatch.setattr(_native, "aln_long_ready", lambda: ready)
    monkeypatch.setattr(_native, "aln_long_operand", FakeLongOperand)
    monkeypatch.setattr(_native, "alignment_long_dense", _long_dense)
    monkeypatch.setattr(_native, "alignment_local_long_dense", _local_long_dense)
    monkeypatch.setattr(_native, "i32_knn", _i32_knn)
    monkeypatch.setattr(_native, "i32_eps", _i32_eps)
