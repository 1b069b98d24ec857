"""
TEST-ONLY stand-in for `_native.alignment_local_dense` / `_native.aln_local_score`, layered on tests/fake_aln_native.py:
the same operands, the same `calls` list, the local alignment recurrence in numpy on CPU tensors, so that the host logic
of `build_graph` / `search` under `local_alignment(S, gap, gap_open)` - route choice, block sizes, selection arguments,
the mirrored comparator, the removal of the diagonal - runs without a GPU.  Nothing under prograph_amd/ imports it.

`recurrence` keeps one rolling row of H and E over all (M, N) pairs at once, the outer loop over the rows of Y; it is
written apart from `definition` in tests/local_testdata.py (outer loop over X, checked there against a brute force over
substrings and alignment paths), and the tests compare its answers with that definition: what they prove through this
stand-in is the host logic around the kernel.
"""
import numpy as np
import torch

import fake_aln_native
from fake_aln_native import calls

NEG = -(1 << 40)


def recurrence(S, gap, gap_open, X, Y):
    """(M, N) int64 local alignment scores of the rows of Y against the rows of X (trailing zeros are padding)."""
    lx, ly = fake_aln_native._lengths(X), fake_aln_native._lengths(Y)
    M, N, LX = len(Y), len(X), X.shape[1]
    H = np.zeros((LX + 1, M, N), dtype=np.int64)
    E = np.full((LX + 1, M, N), NEG, dtype=np.int64)
    best = np.zeros((M, N), dtype=np.int64)
    real = (np.arange(1, LX + 1)[:, None] <= lx[None, :])[:, None, :]          # (LX, 1, N): position j of x exists
    for i in range(1, int(ly.max(initial=0)) + 1):
        sy = S[Y[:, i - 1]]
        E = np.maximum(E - gap, H - gap_open - gap)
        diag = H[0].copy()
        F = np.full((M, N), NEG, dtype=np.int64)
        for j in range(1, LX + 1):
            up = H[j].copy()
            F = np.maximum(F - gap, H[j - 1] - gap_open - gap)
            H[j] = np.maximum(np.maximum(0, diag + sy[:, X[:, j - 1]]), np.maximum(E[j], F))
            diag = up
        row = np.where(real, H[1:], 0).max(axis=0, initial=0)
        best = np.where((ly >= i)[:, None], np.maximum(best, row), best)
    return best


def _score(table):
    t = np.zeros((32, 32), dtype=np.int64)
    t[:len(table), :len(table)] = np.asarray(table)
    calls.append(("score", len(table)))
    return torch.from_numpy(t)


def _local_dense(xo, yo, score, gap, gap_open, out_bytes=8, rows=None):
    r0, r1 = (0, yo.n) if rows is None else rows
    calls.append(("local_dense", r1 - r0, out_bytes, int(gap), int(gap_open)))
    s = recurrence(score.numpy(), int(gap), int(gap_open), xo.tokens.numpy().astype(np.intp),
                   yo.tokens.numpy()[r0:r1].astype(np.intp))
    return torch.from_numpy(s).to({2: torch.float16, 8: torch.int64}[out_bytes])


def install(monkeypatch):
    from prograph_amd import _native
    fake_aln_native.install(monkeypatch)
    monkeypatch.setattr(_native, "aln_local_score", _score)
    monkeypatch.setattr(_native, "alignment_local_dense", _local_dense)
