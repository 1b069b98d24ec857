"""
TEST-ONLY stand-in for `_native.alignment_fit_dense` / `_native.alignment_fit_long_dense`, layered on
tests/fake_long_native.py (and through it on the local and global alignment stand-ins): the same operands, the same `calls`
list, the answers `definition` of tests/fit_testdata.py PLUS the bias on CPU tensors, so that the host logic of
`build_graph` / `search` under `fit_alignment(S, gap, gap_open)` - route choice, block sizes, the shift and its removal,
the shifted threshold, the `s > 0` filter, the removal of the diagonal - runs without a GPU.  A block with a negative entry
is an error here: the selection kernels sort non-negative values.  Nothing under prograph_amd/ imports it.
"""
import numpy as np
import torch

import fake_long_native
from fake_aln_native import calls
from fit_testdata import definition


def _answer(name, dtypes, xo, yo, score, gap, gap_open, out_bytes, rows, bias):
    r0, r1 = (0, yo.n) if rows is None else rows
    calls.append((name, r1 - r0, out_bytes, int(gap), int(gap_open), int(bias)))
    s = definition(score.numpy(), int(gap), int(gap_open), xo.tokens.numpy().astype(np.intp),
                   yo.tokens.numpy()[r0:r1].astype(np.intp)) + int(bias)
    assert out_bytes == 8 or s.min() >= 0, "a block for the selection layers must not be negative"
    assert out_bytes != 2 or s.max() <= 2048, "an fp16 block holds integers up to 2048"
    return torch.from_numpy(s).to(dtypes[out_bytes])


def _dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None, bias=0):
    return _answer("fit_dense", {2: torch.float16, 8: torch.int64}, xo, yo, score, gap, gap_open, out_bytes, rows, bias)


def _long_dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None, bias=0):
    assert isinstance(xo, fake_long_native.FakeLongOperand) and isinstance(yo, fake_long_native.FakeLongOperand)
    return _answer("fit_long_dense", {4: torch.int32, 8: torch.int64}, xo, yo, score, gap, gap_open, out_bytes, rows, bias)


def install(monkeypatch, ready=True):
    from prograph_amd import _native
    fake_long_native.install(monkeypatch, ready=ready)
    monkeypatch.setattr(_native, "alignment_fit_dense", _dense)
    monkeypatch.setattr(_native, "alignment_fit_long_dense", _long_dense)
