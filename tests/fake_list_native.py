"""
TEST-ONLY stand-in for the edge-list kernel (`_native.alignment_list_scores`, `_native.aln_list_ready`), layered on
tests/fake_stats_native.py (and through it on every alignment stand-in, `i32_knn` and `i32_eps` included): the same `calls`
list, the values from the definitions that file uses, on CPU tensors, so that the host logic of `Prograph.rescore` and of
`candidates=` / `pool=` - routes, blocks, padding, the gather back to columns, containers - runs without a GPU.  Nothing
under prograph_amd/ imports it.
"""
import numpy as np
import torch

import fake_stats_native
import fake_trace_native
from fake_aln_native import calls
from fake_stats_native import FIT, head_of
from prograph_amd import _native

INT32_MIN = -(1 << 31)


def value_of(mode, T, gap, gap_open, row, col):
    """The operator's value of an edge: `row` (the Y side: whole, under fit) against `col`."""
    if int(mode) == FIT:                                                  # the tracer's x has the free ends: the column
        return head_of(mode, T, gap, gap_open, col, row)[0]
    return head_of(mode, T, gap, gap_open, row, col)[0]


def _list_scores(xo, yo, indptr, indices, mode, table, gap, gap_open):
    assert isinstance(xo, fake_trace_native.FakeTraceOperand) and isinstance(yo, fake_trace_native.FakeTraceOperand)
    indptr, indices = torch.as_tensor(indptr).to(torch.int64), torch.as_tensor(indices)
    assert indices.dtype == torch.int32 and indptr.numel() == yo.n + 1 and int(indptr[0]) == 0
    assert int(indptr[-1]) == indices.numel() and bool((indptr[1:] >= indptr[:-1]).all())
    calls.append(("list_scores", int(mode), yo.n, indices.numel(), int(gap), int(gap_open)))
    T = table.numpy().astype(np.int64)
    out = torch.empty(indices.numel(), dtype=torch.int32)
    for r in range(yo.n):
        for e in range(int(indptr[r]), int(indptr[r + 1])):
            c = int(indices[e])
            out[e] = value_of(mode, T, gap, gap_open, yo.tokens[r].numpy(), xo.tokens[c].numpy()) if 0 <= c < xo.n else INT32_MIN
    return out


def install(monkeypatch, ready=True, list_ready=True, long_ready=True):
    fake_stats_native.install(monkeypatch, ready=ready, long_ready=long_ready)
    monkeypatch.setattr(_native, "aln_list_ready", lambda: list_ready)
    monkeypatch.setattr(_native, "alignment_list_scores", _list_scores)
