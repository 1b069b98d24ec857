"""
TEST-ONLY stand-in for the launch behind `_native.alignment_stats` (`_native._stats_launch`), layered on
tests/fake_trace_long_native.py (and through it on every alignment stand-in) and tests/fake_fit_native.py: the same `calls`
list, the heads from `definition` of tests/trace_testdata.py (fit: `canonical` of tests/fit_testdata.py) on CPU tensors, so
that the host logic of `ops=False` and of the percent-identity cuts of `build_graph` / `search` - routes, the index check,
the slices of the long route, masks and `indptr` - runs without a GPU.  The long launch is wrapped to record the size of
the `ops` buffer it is handed.  Nothing under prograph_amd/ imports it.
"""
import numpy as np
import torch

import fake_fit_native
import fake_trace_long_native
import fake_trace_native
from fake_aln_native import calls
from fake_long_native import FakeLongOperand
from fit_testdata import canonical, seq
from prograph_amd import _native
from trace_testdata import FIELDS, definition

FIT = 3


def head_of(mode, T, gap, gap_open, x, y):
    """The seven fields of one pair from the definitions."""
    if int(mode) == FIT:
        return list(canonical(T, int(gap), int(gap_open), seq(x), seq(y))[:7])
    d = definition(int(mode), T, int(gap), int(gap_open), x, y)
    return [d[f] for f in FIELDS]


def _launch(xo, yo, xi, yi, mode, table, gap, gap_open, head):
    assert isinstance(xo, fake_trace_native.FakeTraceOperand) and isinstance(yo, fake_trace_native.FakeTraceOperand)
    assert xi.dtype == torch.int32 and yi.dtype == torch.int32 and xi.numel() == yi.numel() == head.shape[0]
    assert head.shape[1] == 8 and head.dtype == torch.int32 and head.is_contiguous()
    calls.append(("stats", int(mode), xi.numel(), int(gap), int(gap_open)))
    T = table.numpy().astype(np.int64)
    for p in range(xi.numel()):
        head[p] = torch.tensor(head_of(mode, T, gap, gap_open, xo.tokens[int(xi[p])].numpy(), yo.tokens[int(yi[p])].numpy()) + [0],
                               dtype=torch.int32)


def _long_launch(xo, yo, xi, yi, p0, p1, mode, table, gap, gap_open, head, ops, ws):
    assert xi.numel() == yi.numel() == head.shape[0] and ops.shape[0] >= head.shape[0] and p1 <= head.shape[0]
    calls.append(("ops_buffer", ops.numel(), ops.shape[0]))
    fake_trace_long_native._launch(xo, yo, xi, yi, p0, p1, mode, table, gap, gap_open, head, ops, ws)


def install(monkeypatch, ready=True, long_ready=True):
    fake_fit_native.install(monkeypatch, ready=ready)
    fake_trace_long_native.install(monkeypatch, ready=ready, long_ready=long_ready)
    monkeypatch.setattr(_native, "aln_long_operand", FakeLongOperand)
    monkeypatch.setattr(_native, "_stats_launch", _launch)
    monkeypatch.setattr(_native, "_trace_long_launch", _long_launch)
