"""
TEST-ONLY stand-in for the launch behind `_native.alignment_trace_long` (`_native._trace_long_launch`), layered on
tests/fake_trace_native.py: the same `calls` list, the answers from `definition` of tests/trace_testdata.py on CPU tensors,
and `aln_trace_long_ready` patched to `ready`, so that the long route of `alignments.trace` and `Prograph.align` - route
choice, the default workspace, the split into launches - runs without a GPU.  The operands are the `FakeLongOperand`s of
tests/fake_long_native.py; `aln_trace_long_wave_bytes` stays the library's own (a host function).  Nothing under
prograph_amd/ imports it.
"""
import numpy as np
import torch

import fake_trace_native
from fake_aln_native import calls
from fake_long_native import FakeLongOperand
from prograph_amd import _native
from trace_testdata import FIELDS, definition


def _launch(xo, yo, xi, yi, p0, p1, mode, table, gap, gap_open, head, ops, ws):
    assert isinstance(xo, FakeLongOperand) and isinstance(yo, FakeLongOperand)
    assert xi.dtype == torch.int32 and yi.dtype == torch.int32 and head.shape[1] == 8 and ops.shape[1] >= xo.l + yo.l
    one = _native.aln_trace_long_wave_bytes(xo.l, yo.l)
    assert ws.numel() >= one and (p1 - p0 + 63) // 64 <= ws.numel() // one       # every wave of the launch has its share
    calls.append(("trace_long", int(mode), p0, p1, int(gap), int(gap_open), ws.numel()))
    T = table.numpy().astype(np.int64)
    for p in range(p0, p1):
        d = definition(int(mode), T, int(gap), int(gap_open), xo.tokens[int(xi[p])].numpy(), yo.tokens[int(yi[p])].numpy())
        head[p] = torch.tensor([d[f] for f in FIELDS] + [0], dtype=torch.int32)
        ops[p] = 0
        ops[p, :d["n_ops"]] = torch.tensor(d["ops"], dtype=torch.uint8)


def install(monkeypatch, ready=True, long_ready=True):
    fake_trace_native.install(monkeypatch, ready=ready)
    monkeypatch.setattr(_native, "aln_trace_long_ready", lambda: long_ready)
    monkeypatch.setattr(_native, "_trace_long_launch", _launch)
