"""
TEST-ONLY stand-in for the long edge-list kernel (`_native.alignment_list_long_scores`, `_native.aln_list_long_ready`),
layered on tests/fake_list_native.py (and through it on every alignment stand-in, `i32_knn` and `i32_eps` included): the
same `calls` list, the values from `fake_list_native.value_of`, on CPU tensors, so that the route of `Prograph.rescore` and
of `candidates=` / `pool=` at 129..2048 positions runs without a GPU.  Nothing under prograph_amd/ imports it.
"""
import numpy as np
import torch

import fake_list_native
from fake_aln_native import calls
from fake_list_native import INT32_MIN, value_of
from fake_long_native import FakeLongOperand
from prograph_amd import _native


def _list_long_scores(xo, yo, indptr, indices, mode, table, gap, gap_open):
    assert isinstance(xo, FakeLongOperand) and isinstance(yo, FakeLongOperand)
    assert _native.ALN_MAX_L < max(xo.l, yo.l) <= _native.ALN_LONG_MAX_L
    indptr, indices = torch.as_tensor(indptr).to(torch.int64), torch.as_tensor(indices)
    assert indices.dtype == torch.int32 and indptr.numel() == yo.n + 1 and int(indptr[0]) == 0
    assert int(indptr[-1]) == indices.numel() and bool((indptr[1:] >= indptr[:-1]).all())
    calls.append(("list_long_scores", int(mode), yo.n, indices.numel(), int(gap), int(gap_open)))
    T = table.numpy().astype(np.int64)
    out = torch.empty(indices.numel(), dtype=torch.int32)
    for r in range(yo.n):
        for e in range(int(indptr[r]), int(indptr[r + 1])):
            c = int(indices[e])
            out[e] = value_of(mode, T, gap, gap_open, yo.tokens[r].numpy(), xo.tokens[c].numpy()) if 0 <= c < xo.n else INT32_MIN
    return out


def install(monkeypatch, ready=True, list_ready=True, long_ready=True, list_long_ready=True):
    fake_list_native.install(monkeypatch, ready=ready, list_ready=list_ready, long_ready=long_ready)
    monkeypatch.setattr(_native, "aln_list_long_ready", lambda: list_long_ready)
    monkeypatch.setattr(_native, "alignment_list_long_scores", _list_long_scores)
