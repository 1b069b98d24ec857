"""
Fit ("glocal") alignment score over tokenised, zero right-padded sequences - NOT in the reference (acmater/prograph ships
only hamming / minkowski); defined by this build.

    score = fit_alignment(S, gap)               # S: (A, A) SCORE table indexed by token value: larger is nearer
    score = fit_alignment(S, gap, gap_open=o)   # affine: a run of g unaligned symbols costs o + g * gap
    s = score(X (N,D1), Y (M,D2))               # (M, N): the best alignment of ALL of Y[m] with ANY SUBSTRING of X[n]

`alignment` is global and charges for the whole parent; `local_alignment` cuts away whatever is awkward;
`semiglobal_alignment` lets either sequence drop its own ends.  This is the fourth mode, the one that answers "where in this
protein does my peptide sit, and how well": every symbol of y is aligned or paid for, and only the ends of x are free.
s(x, y) is the maximum, over all substrings x' of x (the empty one included), of the global affine score of y against x'.
Gotoh's form, maximising (e = gap, o = gap_open, i over x, j over y):

    H[i][0] = 0 (i = 0..len x),   H[0][j] = F[0][j] = -(o + j e) (j >= 1),   E[0][j] = E[i][0] = F[i][0] = -inf,
    E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
    H[i][j] = max(H[i-1][j-1] + S[x_i, y_j], E[i][j], F[i][j])                                  (no zero floor),
    s(x, y) = max over i = 0..len x of H[i][len y].

  * NOT SYMMETRIC.  The whole sequence is the Y operand of the operator, everywhere: in `build_graph` the graph's row, in
    `search` the query.  An edge (r, c) or a hit (q, c) reads "row r / query q, whole, placed in column c".
  * Range: -(o + e len y) <= s <= min(len x, len y) * max(0, max S).  An empty y scores 0 against everything, an empty x
    scores -(o + e len y): all of y unaligned.
  * SCORES MAY BE NEGATIVE, as those of no other score operator here.
  * Under a table whose diagonal entries are the largest of their rows, a sequence against itself scores its self score
    sum S[y_j, y_j], and so does a fragment cut from x against x (at least that under any table) - which `alignment`
    never gives, and `semiglobal_alignment` only while dropping an end of the fragment does not pay better.

It is a SIMILARITY and takes the whole contract of `local_alignment`: sequences (a row without its trailing zeros, an
interior zero is symbol 0, padding never scores), the table's rules (2..32 symbols, integers in -128..127, symmetric, an
entry of at least 1; copied), `gap` in 1..255, `gap_open` in 0..255, `similarity=False` raises, `build_graph` and `search`
rank largest first whatever their `similarity` argument says.  Self graphs are directed: row r lists the columns that
CONTAIN r best; rank 0 - the row itself, or a row of lower index that contains it - is dropped as for every distance.

Device byte-token operands of at most 128 positions run on the HIP kernel `pg_alignment_fit_dense`, those of 129..2048
positions on the strip-mined `pg_alignment_fit_long_dense` (both prograph_amd/csrc/pg_aln_fit.hip), while
gap_open + width_y * (gap + 2 max(0, max S)) + 255 <= 65 535 (`_native.aln_fit_fits`): their 16-bit cells hold the score plus
gap_open + width_y * (gap + max S).  The short kernel needs the bound too (128 positions at 255 / 255 / 127 miss it).
Everything else is evaluated by the torch expression below on the device the operands live on, CPU included: the table
row by row over the whole (M, N) batch in `local_alignment._dp_block`'s style without the clamp - the batch tables run over
the rows of Y, so X lies along a row: row 0 is 0 (the free prefix of x), column 0 follows E (y_1..y_i unaligned), and the
result is the maximum of row len y over the columns j <= len x.  It is the slow path; it is exact.

`score.align(X, Y)` returns the alignments themselves - row p of Y, whole, within row p of X: see prograph_amd/alignments.py.
"""
import torch

from .. import _native
from .local_alignment import _score_operator


class fit_alignment(_score_operator):
    """The score of one score table and gap penalty, linear or affine (see the module text)."""
    _DENSE, _LONG_DENSE, _LONG_FITS = "alignment_fit_dense", "alignment_fit_long_dense", "aln_fit_fits"
    _WHAT = "a fit alignment score"

    def _long_fits(self, width_x, width_y):
        return _native.aln_fit_fits(width_x, width_y, self.max_score, self._gap, self._open)

    _short_fits = _long_fits                         # the 128-position kernel's cells are the same 16 bits

    def _select_bias(self, width_y):
        """What `build_graph` and `search` add to every score of a block before the selection layers, which sort
        non-negative values: -(the least score) of a row operand `width_y` wide."""
        return self._open + self._gap * int(width_y)

    def _f16_route(self, width_x, width_y):
        """Shifted scores lie in 0..bias + width_y * max(S): the fp16 blocks hold them exactly up to 2048."""
        return (max(width_x, width_y) <= _native.ALN_MAX_L and self._short_fits(width_x, width_y)
                and self._select_bias(width_y) + width_y * self.max_score <= 2048)

    def _i32_route(self, width_x, width_y):
        """Everything else inside `aln_fit_fits`, narrow operands included: int32 blocks of the strip-mined kernel."""
        return _native.aln_long_ready() and self._long_fits(width_x, width_y)

    def _native_dense(self, xo, yo, out_bytes, rows=None, bias=0):
        return _native.alignment_fit_dense(xo, yo, self.device_score(), self._gap, self._open, out_bytes=out_bytes, rows=rows,
                                           bias=bias)

    def _native_long_dense(self, xo, yo, out_bytes, rows=None, bias=0):
        return _native.alignment_fit_long_dense(xo, yo, self.device_score(), self._gap, self._open, out_bytes=out_bytes,
                                                rows=rows, bias=bias)

    def _dp_block(self, St, x, lx, y, ly):
        """(m, n) int64 scores of y rows (lengths ly) against x rows (lengths lx); x, y already cut to the longest
        sequence among their rows.  Row i of every table at once; F is resolved inside the row by the cummax over A."""
        m, n, dx, e, o = y.shape[0], x.shape[0], x.shape[1], self._gap, self._open
        jg = torch.arange(dx + 1, device=x.device, dtype=torch.int32) * e
        v = torch.zeros((m, n, dx + 1), dtype=torch.int32, device=x.device)    # row 0: 0 - y may start anywhere in x
        E = torch.full_like(v, -(1 << 28))                                     # E of row 0: -inf
        inside = (torch.arange(dx + 1, device=x.device).view(1, 1, -1) <= lx.view(1, n, 1))      # j <= len x
        low = torch.full_like(v, -(1 << 28))
        best = torch.zeros((m, n), dtype=torch.int32, device=x.device)        # len y = 0: row 0
        xl = x.long().view(1, n, dx)
        for i in range(1, y.shape[1] + 1):
            score = St[y[:, i - 1].long().view(m, 1, 1), xl]                   # (m, n, dx): S[y_i, x_j]
            E = torch.maximum(E - e, v - (o + e))                              # extend the run | open one from the row above
            A = E.clone()                                                      # column 0: y_1..y_i unaligned, -(o + i e)
            A[..., 1:] = torch.maximum(v[..., :-1] + score, E[..., 1:])        # aligned pair | y_i unaligned
            F = low.clone()                                                    # no x symbol before column 1
            F[..., 1:] = torch.cummax(A + jg, dim=2).values[..., :-1] - jg[1:] - o         # max over k < j of A[k] - o - (j - k) e
            v = torch.maximum(A, F)
            last_row = torch.where(inside, v, low).amax(dim=2)                 # row i over the columns j <= len x
            best = torch.where((ly == i).view(m, 1), last_row, best)           # row len y alone is read
        return best.to(torch.int64)
