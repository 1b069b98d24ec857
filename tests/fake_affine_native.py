"""
TEST-ONLY stand-in for `_native.alignment_affine_dense`, layered on tests/fake_aln_native.py: the same operands, the same
`calls` list, the affine recurrence in numpy on CPU tensors, so that the host logic of `build_graph` / `search` under
`alignment(C, gap, gap_open=o)` - route choice, block sizes, selection arguments - runs without a GPU.  Nothing under
prograph_amd/ imports it.

`recurrence` keeps one rolling row of H and E over all (M, N) pairs at once; it is written apart from the definition in
tests/test_alignment_affine_cpu.py (full H, E, F tables, checked there against a brute force over alignment paths), and
the tests compare its answers with that definition: what they prove through this stand-in is the host logic around the
kernel.
"""
import numpy as np
import torch

import fake_aln_native
from fake_aln_native import calls

BIG = 1 << 40


def recurrence(C, gap, gap_open, X, Y):
    """(M, N) int64 affine alignment distances of the rows of Y against the rows of X (trailing zeros are padding)."""
    lx, ly = fake_aln_native._lengths(X), fake_aln_native._lengths(Y)
    M, N, LX = len(Y), len(X), X.shape[1]
    H = np.empty((LX + 1, M, N), dtype=np.int64)
    H[:] = (gap_open + np.arange(LX + 1) * gap)[:, None, None]
    H[0] = 0
    E = np.full((LX + 1, M, N), BIG, dtype=np.int64)
    at = np.broadcast_to(lx[None, None, :], (1, M, N))
    out = np.take_along_axis(H, at, 0)[0].copy()
    for i in range(1, int(ly.max(initial=0)) + 1):
        cy = C[Y[:, i - 1]]
        E = np.minimum(E + gap, H + gap_open + gap)
        diag = H[0].copy()
        H[0] = gap_open + i * gap
        F = np.full((M, N), BIG, dtype=np.int64)
        for j in range(1, LX + 1):
            up = H[j].copy()
            F = np.minimum(F + gap, H[j - 1] + gap_open + gap)
            H[j] = np.minimum(diag + cy[:, X[:, j - 1]], np.minimum(E[j], F))
            diag = up
        done = ly == i
        out[done] = np.take_along_axis(H, at, 0)[0][done]
    return out


def _affine_dense(xo, yo, cost, gap, gap_open, out_bytes=8, rows=None):
    r0, r1 = (0, yo.n) if rows is None else rows
    calls.append(("affine_dense", r1 - r0, out_bytes, int(gap), int(gap_open)))
    d = recurrence(cost.numpy(), int(gap), int(gap_open), xo.tokens.numpy().astype(np.intp),
                   yo.tokens.numpy()[r0:r1].astype(np.intp))
    return torch.from_numpy(d).to({2: torch.float16, 8: torch.int64}[out_bytes])


def install(monkeypatch):
    from prograph_amd import _native
    fake_aln_native.install(monkeypatch)
    monkeypatch.setattr(_native, "alignment_affine_dense", _affine_dense)
