"""
Semi-global ("overlap", end-gap-free) alignment score over tokenised, zero right-padded sequences - NOT in the reference
(acmater/prograph ships only hamming / minkowski); defined by this build.

    score = semiglobal_alignment(S, gap)               # S: (A, A) SCORE table indexed by token value: larger is nearer
    score = semiglobal_alignment(S, gap, gap_open=o)   # affine: a run of g unaligned symbols costs o + g * gap
    s = score(X (N,D1), Y (M,D2))                      # (M, N): the best end-gap-free alignment of Y[m] with X[n]

`alignment` is global: every symbol of both sequences is aligned or paid for.  `local_alignment` aligns the best pair of
substrings and may discard everything awkward.  This is the third mode: drop a prefix of at most one of the two
sequences and a suffix of at most one of them at no cost, then align what is left globally; s(x, y) is the best such
score.  A fragment against its parent must align as a whole - an internal mismatch or indel is paid for, only the
parent's overhang is free - and two sequences of which one ends as the other begins score their overlap.  Gotoh's form,
maximising (e = gap, i over x, j over y):

    H[i][0] = H[0][j] = 0,   E[0][j] = F[i][0] = -inf,
    E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
    H[i][j] = max(H[i-1][j-1] + S[x_i, y_j], E[i][j], F[i][j])                                  (no zero floor),
    s = max(max over i of H[i][len y], max over j of H[len x][j])                      (i = 0..len x, j = 0..len y).

s is symmetric, at least 0 (H[0][len y] = 0) and at most min(len x, len y) * max(S); an empty sequence scores 0 against
everything; gap_open = 0 is the linear gap penalty.  It is a SIMILARITY and takes the whole contract of
`local_alignment`: sequences (a row without its trailing zeros, an interior zero is symbol 0, padding never scores), the
table's rules (2..32 symbols, integers in -128..127, symmetric, an entry of at least 1; copied), `gap` in 1..255,
`gap_open` in 0..255, `similarity=False` raises, `build_graph` and `search` rank largest first whatever their
`similarity` argument says (prograph.py: `_build_graph_local`, `_search_local`, by type).

Device byte-token operands of at most 128 positions run on the HIP kernel (`pg_alignment_semiglobal_dense`,
prograph_amd/csrc/pg_aln_semiglobal.hip); those of 129..2048 positions on the strip-mined kernel of the same file
(`pg_alignment_semiglobal_long_dense`) while 2 * min(widths) * max(S) + 255 <= 65 535, the bound of its 16-bit cells,
which hold the score plus min(widths) * max(S).  Everything else is evaluated by the torch expression below on the device
the operands live on, CPU included: the table row by row over the whole (M, N) batch in `local_alignment._dp_block`'s
style without the clamp, F by the cummax over A, and the result picked from column len x of every row i <= len y and from
row len y (the batch tables run over the rows of Y, so X lies along a row).  It is the slow path; it is exact.

`score.align(X, Y)`, inherited, returns the alignments themselves: see prograph_amd/alignments.py.
"""
import torch

from .local_alignment import _score_operator


class semiglobal_alignment(_score_operator):
    """The score of one score table and gap penalty, linear or affine (see the module text)."""
    _DENSE, _LONG_DENSE, _LONG_FITS = "alignment_semiglobal_dense", "alignment_semiglobal_long_dense", "aln_semiglobal_long_fits"
    _WHAT = "a semi-global alignment score"

    def _dp_block(self, St, x, lx, y, ly):
        """(m, n) int64 scores of y rows (lengths ly) against x rows (lengths lx); x, y already cut to the longest
        sequence among their rows.  Row i of every table at once; F is resolved inside the row by the cummax over A."""
        m, n, dx, e, o = y.shape[0], x.shape[0], x.shape[1], self._gap, self._open
        jg = torch.arange(dx + 1, device=x.device, dtype=torch.int32) * e
        v = torch.zeros((m, n, dx + 1), dtype=torch.int32, device=x.device)    # row 0: H[0][j] = 0
        E = torch.full_like(v, -(1 << 28))                                     # E[0][j] = -inf
        inside = (torch.arange(dx + 1, device=x.device).view(1, 1, -1) <= lx.view(1, n, 1))      # j <= len x
        at = lx.long().view(1, n, 1).expand(m, n, 1)                           # column len x of every table
        low = torch.full_like(v, -(1 << 28))
        best = torch.zeros((m, n), dtype=torch.int32, device=x.device)        # H[0][len x] = 0; len y = 0: row 0
        xl = x.long().view(1, n, dx)
        for i in range(1, y.shape[1] + 1):
            score = St[y[:, i - 1].long().view(m, 1, 1), xl]                   # (m, n, dx): S[y_i, x_j]
            E = torch.maximum(E - e, v - (o + e))                              # extend the run | open one from the row above
            A = torch.zeros_like(v)                                            # H[i][0] = 0
            A[..., 1:] = torch.maximum(v[..., :-1] + score, E[..., 1:])        # aligned pair | gap against y_i
            F = low.clone()                                                    # F[i][0] = -inf
            F[..., 1:] = torch.cummax(A + jg, dim=2).values[..., :-1] - jg[1:] - o         # max over k < j of A[k] - o - (j - k) e
            v = torch.maximum(A, F)
            last_col = torch.where((ly >= i).view(m, 1), v.gather(2, at)[..., 0], best)    # H[i][len x], i <= len y
            last_row = torch.where((ly == i).view(m, 1), torch.where(inside, v, low).amax(dim=2), best)   # row len y, j <= len x
            best = torch.maximum(best, torch.maximum(last_col, last_row))
        return best.to(torch.int64)
