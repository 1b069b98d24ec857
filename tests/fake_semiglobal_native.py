"""
TEST-ONLY stand-in for `_native.alignment_semiglobal_dense` / `_native.alignment_semiglobal_long_dense`, layered on
tests/fake_long_native.py (and through it on the local and global alignment stand-ins): the same operands, the same `calls`
list, the answers from `definition` of tests/semiglobal_testdata.py on CPU tensors, so that the host logic of
`build_graph` / `search` under `semiglobal_alignment(S, gap, gap_open)` - route choice, block sizes, selection arguments,
the mirrored comparator, the removal of the diagonal - runs without a GPU.  The local stand-ins stay installed: a call
that reached them would show in `calls`.  Nothing under prograph_amd/ imports it.
"""
import numpy as np
import torch

import fake_long_native
from fake_aln_native import calls
from semiglobal_testdata import definition


def _answer(name, dtypes, xo, yo, score, gap, gap_open, out_bytes, rows):
    r0, r1 = (0, yo.n) if rows is None else rows
    calls.append((name, r1 - r0, out_bytes, int(gap), int(gap_open)))
    s = definition(score.numpy(), int(gap), int(gap_open), xo.tokens.numpy().astype(np.intp),
                   yo.tokens.numpy()[r0:r1].astype(np.intp))
    return torch.from_numpy(s).to(dtypes[out_bytes])


def _dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None):
    return _answer("semiglobal_dense", {2: torch.float16, 8: torch.int64}, xo, yo, score, gap, gap_open, out_bytes, rows)


def _long_dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None):
    assert isinstance(xo, fake_long_native.FakeLongOperand) and isinstance(yo, fake_long_native.FakeLongOperand)
    return _answer("semiglobal_long_dense", {4: torch.int32, 8: torch.int64}, xo, yo, score, gap, gap_open, out_bytes, rows)


def install(monkeypatch, ready=True):
    from prograph_amd import _native
    fake_long_native.install(monkeypatch, ready=ready)
    monkeypatch.setattr(_native, "alignment_semiglobal_dense", _dense)
    monkeypatch.setattr(_native, "alignment_semiglobal_long_dense", _long_dense)
