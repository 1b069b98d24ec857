"""
TEST-ONLY stand-in for the entry points of the Levenshtein kernel beyond 128 positions (`_native.lev_long_operand`,
`levenshtein_long_dense`, `lev_long_ready`), on top of tests/fake_lev_native.py and in the style of
tests/fake_long_native.py: the same `calls` list, the answers from `lev_long_testdata.wagner_fischer_rows` on CPU tensors,
and the fp16 selection recorded with its arguments, so that the host logic of the long routes - route choice, block
format, selection arguments, containers, dtypes - runs without a GPU.  Nothing under prograph_amd/ imports it.
"""
import numpy as np
import torch

import fake_lev_native
import fake_native
import lev_long_testdata as LL
from fake_lev_native import calls
from prograph_amd import _native

_memo = {}


class FakeLevLongOperand:
    def __init__(self, tokens):
        self.tokens = tokens if isinstance(tokens, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tokens))
        assert self.tokens.dtype == torch.uint8 and self.tokens.dim() == 2 and 1 <= self.tokens.shape[1] <= _native.LEV_LONG_MAX_L
        self.n, self.l = self.tokens.shape
        calls.append(("long_operand", self.n, self.l))

    def valid(self):
        t = self.tokens.numpy()
        lens = (t != 0).sum(1)
        return bool(t.max() <= 31) and all((r[:l] != 0).all() for r, l in zip(t, lens))


def _long_dense(xo, yo, out_bytes=8, rows=None):
    assert isinstance(xo, FakeLevLongOperand) and isinstance(yo, FakeLevLongOperand) and out_bytes in (2, 8)
    r0, r1 = (0, yo.n) if rows is None else rows
    calls.append(("long_dense", r1 - r0, out_bytes))
    X, Y = xo.tokens.numpy(), yo.tokens.numpy()[r0:r1]
    key = (X.shape, Y.shape, X.tobytes(), Y.tobytes())
    if key not in _memo:
        _memo[key] = LL.wagner_fischer_rows(X, Y)
    return torch.from_numpy(_memo[key]).to({2: torch.float16, 8: torch.int64}[out_bytes])


def _f16_knn(block, k, first=1, descending=False):
    assert block.dtype == torch.float16
    calls.append(("f16_knn", k, first, descending))
    return fake_native._f16_knn(block, k, first=first, descending=descending)


def _f16_eps(block, cmp, eps, similarity=False, keep_zero=False):
    assert block.dtype == torch.float16
    calls.append(("f16_eps", cmp, float(eps), keep_zero))
    return fake_lev_native._f16_eps(block, cmp, eps, similarity=similarity, keep_zero=keep_zero)


def install(monkeypatch, ready=True):
    fake_lev_native.install(monkeypatch)
    monkeypatch.setattr(_native, "lev_long_ready", lambda: ready)
    monkeypatch.setattr(_native, "lev_long_operand", FakeLevLongOperand)
    monkeypatch.setattr(_native, "levenshtein_long_dense", _long_dense)
    monkeypatch.setattr(_native, "f16_knn", _f16_knn)
    monkeypatch.setattr(_native, "f16_eps", _f16_eps)
