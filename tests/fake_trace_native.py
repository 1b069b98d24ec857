"""
TEST-ONLY stand-in for the launch behind `_native.alignment_trace` (`_native._trace_launch`), layered on
tests/fake_semiglobal_native.py (and through it on every alignment stand-in): the same `calls` list, the answers from
`definition` of tests/trace_testdata.py on CPU tensors, so that the host logic of `Prograph.align` and
`_native.alignment_trace` - edge lists, `idxs`, queries, the index check, the split into launches that fit
`workspace_bytes` - runs without a GPU.  `aln_trace_wave_bytes` stays the library's own (a host function).  Nothing under
prograph_amd/ imports it.
"""
import numpy as np
import torch

import fake_semiglobal_native
from fake_aln_native import calls
from prograph_amd import _native
from trace_testdata import FIELDS, definition


class FakeTraceOperand:
    def __init__(self, tokens, a):
        self.tokens = tokens if isinstance(tokens, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tokens))
        assert self.tokens.dtype == torch.uint8 and self.tokens.dim() == 2 and self.tokens.shape[1] <= _native.ALN_MAX_L
        self.n, self.l = self.tokens.shape
        self.a, self.npad, self.buf = int(a), _native.npad(self.n), torch.zeros(1, dtype=torch.int32)
        self.flags = torch.zeros(1, dtype=torch.int32) + int(self.tokens.max() >= self.a)
        calls.append(("operand", self.n, self.l, self.a))

    def valid(self):
        return int(self.flags.item()) == 0


def _launch(xo, yo, xi, yi, p0, p1, mode, table, gap, gap_open, head, ops, ws):
    assert isinstance(xo, FakeTraceOperand) and isinstance(yo, FakeTraceOperand)
    assert xi.dtype == torch.int32 and yi.dtype == torch.int32 and head.shape[1] == 8 and ops.shape[1] >= xo.l + yo.l
    one = _native.aln_trace_wave_bytes(xo.l, yo.l)
    assert ws.numel() >= one and (p1 - p0 + 63) // 64 <= ws.numel() // one       # every wave of the launch has its share
    calls.append(("trace", int(mode), p0, p1, int(gap), int(gap_open)))
    T = table.numpy().astype(np.int64)
    for p in range(p0, p1):
        d = definition(int(mode), T, int(gap), int(gap_open), xo.tokens[int(xi[p])].numpy(), yo.tokens[int(yi[p])].numpy())
        head[p] = torch.tensor([d[f] for f in FIELDS] + [0], dtype=torch.int32)
        ops[p] = 0
        ops[p, :d["n_ops"]] = torch.tensor(d["ops"], dtype=torch.uint8)


def install(monkeypatch, ready=True):
    fake_semiglobal_native.install(monkeypatch, ready=ready)
    monkeypatch.setattr(_native, "aln_operand", FakeTraceOperand)
    monkeypatch.setattr(_native, "_trace_launch", _launch)
