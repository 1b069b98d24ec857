"""
Gapped alignment distance over tokenised, zero right-padded sequences - NOT in the reference (acmater/prograph ships
only hamming / minkowski); defined by this build.

    dist = alignment(C, gap)                  # C: (A, A) cost table indexed by token value, or a `substitution`
    dist = alignment(C, gap, gap_open=o)      # affine: a run of g unaligned symbols costs o + g * gap (see below)
    d = dist(X (N,D1), Y (M,D2))              # (M, N): global alignment of Y[m] with X[n]

Global alignment (Needleman-Wunsch) with a linear gap penalty: d(x, y) is the minimum, over all alignments of the two
sequences, of the sum of C[x_i, y_j] over the aligned pairs plus `gap` per symbol left unaligned,

    H[0][j] = j * gap,   H[i][0] = i * gap,
    H[i][j] = min(H[i-1][j-1] + C[x_i, y_j], H[i-1][j] + gap, H[i][j-1] + gap),       d = H[len x][len y].

`dist` follows the operator protocol of `hamming`: row m is Y[m] against every row of X, `torch.int64`, on the device of
X; `ValueError` on an empty operand; `similarity=True` returns 1/(1+d).

    * a row's sequence is the row with its trailing zeros removed (an all-zero row is the empty sequence), as for
      `levenshtein`, so the zero padding `clean_input` adds to the narrower operand changes nothing;
    * an interior zero - a letter outside the alphabet - is an ordinary symbol: row and column 0 of C;
    * the table takes the rules of `substitution` (square, 2..32 symbols, integers 0..255, symmetric, zero diagonal,
      copied; `ValueError` otherwise) and is checked by that class; a `substitution` instance lends its table, so
      `substitution.from_scores` and `substitution.for_alphabet` serve both distances;
    * `gap` is an integer in 1..255 (`ValueError` for a bool, a fraction, 0 or more than 255);
    * operands must hold integers in 0..A-1 (any dtype); anything else raises `ValueError`.

`alignment(1 - I, 1)` is the Levenshtein distance; on operands of one length L without zeros and with
2 * gap > L * max(C) no gap pays and the distance is `substitution(C)`.

Device byte-token operands of at most 128 positions run on the HIP kernel (`pg_alignment_dense`,
prograph_amd/csrc/pg_aln.hip); those of 129..2048 positions on the strip-mined kernel (`pg_alignment_long_dense`,
prograph_amd/csrc/pg_aln_long.hip, linear and affine alike) while width * max(max C, gap) + 2 gap_open + 2 gap <= 65 535,
the bound of its 16-bit cells.  Everything else is evaluated by the torch expression below on the device the operands
live on, CPU included: the table row by row over the whole (M, N) batch, as in `levenshtein`, the dependency inside a
row resolved by v[j] = j * gap + cummin(c[k] - k * gap).  It is the slow path; it is exact.

Affine gap penalties: `alignment(C, gap, gap_open=o)`, o an integer in 0..255, prices a maximal run of g consecutive
unaligned symbols of one sequence at o + g * gap (a run in x directly followed by a run in y is two runs) - an indel of
several residues is one event, as the open / extend pair that accompanies a score matrix has it.  With e = gap:

    H[0][0] = 0,   H[0][j] = o + j e,   H[i][0] = o + i e,
    E[i][j] = min(E[i-1][j] + e, H[i-1][j] + o + e),   F[i][j] = min(F[i][j-1] + e, H[i][j-1] + o + e),
    H[i][j] = min(H[i-1][j-1] + C[x_i, y_j], E[i][j], F[i][j]),                       d = H[len x][len y],

E[0][j] and F[i][0] infinite.  gap_open = 0 is the linear form above in every respect.  With gap_open > 0 the kernel is
`pg_alignment_affine_dense` (prograph_amd/csrc/pg_aln_affine.hip) and the torch expression carries E between rows:
A[j] = min(v_old[j-1] + cost, E[j]), F[j] = o + j e + cummin_{k<j}(A[k] - k e) - a cell that is itself in a gap never
opens a cheaper one than extending does, so the cummin may run over A instead of H - and v[j] = min(A[j], F[j]).
A distance is at most width * max(max C, gap) + gap_open: align the shorter sequence, gap the rest in one run.

`build_graph` and `search` recognise instances by type (prograph.py: `_build_graph_alignment`, `_search_alignment`);
two instances with equal table, gap and gap_open behave identically.

`dist.align(X, Y)` returns the alignments themselves - row p of X with row p of Y - and `Prograph.align` those of a graph's
edges: see prograph_amd/alignments.py.
"""
import numpy as np
import torch

from .. import _native
from .. import alignments as _alignments
from .hamming import _as_byte_tokens
from .levenshtein import _lengths
from .substitution import substitution
from .utils import clean_input

_DP_ELEMS = 1 << 24            # table entries (pairs x columns) alive per block of the torch expression


def _gap_open(gap_open):
    """An integer in 0..255 as int, or ValueError."""
    if isinstance(gap_open, (bool, np.bool_)) or not isinstance(gap_open, (int, float, np.integer, np.floating)):
        raise ValueError("the gap-open penalty must be an integer in 0..255")
    if not np.isfinite(gap_open) or gap_open != int(gap_open) or not 0 <= int(gap_open) <= _native.ALN_MAX_OPEN:
        raise ValueError("the gap-open penalty must be an integer in 0..255")
    return int(gap_open)


def _gap(gap):
    """An integer in 1..255 as int, or ValueError."""
    if isinstance(gap, (bool, np.bool_)) or not isinstance(gap, (int, float, np.integer, np.floating)):
        raise ValueError("the gap penalty must be an integer in 1..255")
    if not np.isfinite(gap) or gap != int(gap) or not 1 <= int(gap) <= _native.ALN_MAX_GAP:
        raise ValueError("the gap penalty must be an integer in 1..255")
    return int(gap)


class alignment:
    """The distance of one cost table and gap penalty, linear or affine (see the module text)."""

    def __init__(self, C, gap, gap_open=0):
        self._sub = C if isinstance(C, substitution) else substitution(C)      # its constructor validates and copies
        self._gap = _gap(gap)
        self._open = _gap_open(gap_open)

    @property
    def table(self):
        """The (A, A) uint8 cost table (read-only)."""
        return self._sub.table

    @property
    def gap(self):
        return self._gap

    @property
    def gap_open(self):
        """The price of opening a run of unaligned symbols, on top of `gap` per symbol; 0 is the linear penalty."""
        return self._open

    @property
    def symbols(self):
        return self._sub.symbols

    @property
    def max_cost(self):
        """The largest cost of one alignment column: max(max C, gap).  A distance is at most width * max_cost +
        gap_open."""
        return max(self._sub.max_cost, self._gap)

    def __repr__(self):
        opening = f", gap_open={self._open}" if self._open else ""
        return f"alignment(<{self.symbols} x {self.symbols} table, costs up to {self._sub.max_cost}>, gap={self._gap}{opening})"

    def device_cost(self):
        """The kernel's 32 x 32 uint8 table on the current HIP device."""
        return self._sub.device_cost()

    # ------------------------------------------------------------------ the operator
    def _dp_block(self, Ct, x, lx, y, ly):
        """(m, n) int64 distances of y rows (lengths ly) against x rows (lengths lx); x, y already cut to the longest
        sequence among their rows."""
        if self._open:
            return self._dp_block_affine(Ct, x, lx, y, ly)
        m, n, dx, gap = y.shape[0], x.shape[0], x.shape[1], self._gap
        jg = torch.arange(dx + 1, device=x.device, dtype=torch.int32) * gap
        v = jg.expand(m, n, dx + 1).contiguous()                             # row 0 of every table: H[0][j] = j * gap
        at = lx.view(1, n, 1).expand(m, n, 1)
        res = v.gather(2, at).squeeze(2)                                     # empty y: d = len(x) * gap
        xl = x.long().view(1, n, dx)
        for i in range(1, y.shape[1] + 1):
            cost = Ct[y[:, i - 1].long().view(m, 1, 1), xl]                  # (m, n, dx): C[y_i, x_j]
            c = torch.empty_like(v)
            c[..., 0] = i * gap
            c[..., 1:] = torch.minimum(v[..., 1:] + gap, v[..., :-1] + cost)  # gap in x | aligned pair
            v = torch.cummin(c - jg, dim=2).values + jg                      # gaps in y: min over k <= j of c[k] + (j - k) gap
            res = torch.where((ly == i).view(m, 1), v.gather(2, at).squeeze(2), res)
        return res.to(torch.int64)

    def _dp_block_affine(self, Ct, x, lx, y, ly):
        """`_dp_block` under affine penalties: E (a run ending in a gap against y_i) is carried from row to row, F (a run
        along the row) is resolved inside the row by the cummin over A = min(diagonal, E)."""
        m, n, dx, e, o = y.shape[0], x.shape[0], x.shape[1], self._gap, self._open
        jg = torch.arange(dx + 1, device=x.device, dtype=torch.int32) * e
        v = (jg + o).expand(m, n, dx + 1).contiguous()                       # row 0: H[0][j] = o + j e,
        v[..., 0] = 0                                                        # H[0][0] = 0
        E = v + o                                                            # stands for E[0][j] = inf: E + e = H + o + e
        at = lx.view(1, n, 1).expand(m, n, 1)
        res = v.gather(2, at).squeeze(2)                                     # empty y: one run of len(x), or nothing
        xl = x.long().view(1, n, dx)
        for i in range(1, y.shape[1] + 1):
            cost = Ct[y[:, i - 1].long().view(m, 1, 1), xl]                  # (m, n, dx): C[y_i, x_j]
            E = torch.minimum(E + e, v + (o + e))                            # extend the run | open one from the row above
            A = torch.empty_like(v)
            A[..., 0] = o + i * e                                            # H[i][0], which is E[i][0]
            A[..., 1:] = torch.minimum(v[..., :-1] + cost, E[..., 1:])       # aligned pair | gap against y_i
            F = torch.full_like(v, 1 << 30)                                  # F[i][0] = inf
            F[..., 1:] = torch.cummin(A - jg, dim=2).values[..., :-1] + jg[1:] + o      # min over k < j of A[k] + o + (j - k) e
            v = torch.minimum(A, F)
            res = torch.where((ly == i).view(m, 1), v.gather(2, at).squeeze(2), res)
        return res.to(torch.int64)

    def _torch_expression(self, X, Y):
        """The definition as a torch expression: X (N, D), Y (M, D) uint8 on one device -> (M, N) int64."""
        Ct = self._sub._table_on(X.device).to(torch.int32)
        lx, ly = _lengths(X), _lengths(Y)
        X, Y = X[:, :int(lx.max())], Y[:, :int(ly.max())]
        n, m = X.shape[0], Y.shape[0]
        elems = _DP_ELEMS // 2 if self._open else _DP_ELEMS                  # the affine form keeps E beside every row
        cols = max(1, min(n, elems // (X.shape[1] + 1)))
        rows = max(1, min(m, elems // (cols * (X.shape[1] + 1))))
        out = torch.empty((m, n), dtype=torch.int64, device=X.device)
        for r0 in range(0, m, rows):
            for c0 in range(0, n, cols):
                out[r0:r0 + rows, c0:c0 + cols] = self._dp_block(Ct, X[c0:c0 + cols], lx[c0:c0 + cols], Y[r0:r0 + rows],
                                                                 ly[r0:r0 + rows])
        return out

    def __call__(self, X, Y, similarity=False):
        """(M, N) distances (or similarities 1/(1+d)) of the M rows of Y against the N rows of X, int64."""
        X, Y = clean_input(X, Y)
        Y = Y.to(X.device)
        xb = _as_byte_tokens(X)
        yb = xb if Y is X else _as_byte_tokens(Y)
        if xb is None or yb is None:
            raise ValueError("alignment: the tokens must be integers in 0..255")
        native = xb.is_cuda and 1 <= xb.shape[1] <= _native.ALN_MAX_L
        long = (not native and xb.is_cuda and _native.aln_long_ready()
                and _native.aln_long_fits(xb.shape[1], self.max_cost, self._gap, self._open))
        if long:                                                              # 129..2048 positions inside the 16-bit cells
            xo = _native.aln_long_operand(xb, self.symbols)
            yo = xo if yb is xb else _native.aln_long_operand(yb, self.symbols)
            d = _native.alignment_long_dense(xo, yo, self.device_cost(), self._gap, self._open, out_bytes=8)
            native = True
            inside = int((xo.flags | yo.flags).item()) == 0
        elif native:
            xo = _native.aln_operand(xb, self.symbols)
            yo = xo if yb is xb else _native.aln_operand(yb, self.symbols)
            if self._open:
                d = _native.alignment_affine_dense(xo, yo, self.device_cost(), self._gap, self._open, out_bytes=8)
            else:
                d = _native.alignment_dense(xo, yo, self.device_cost(), self._gap, out_bytes=8)
            inside = int((xo.flags | yo.flags).item()) == 0                   # the pack's validity words: the one host sync
        else:
            inside = int(xb.max()) < self.symbols and int(yb.max()) < self.symbols
        if not inside:
            raise ValueError(f"alignment: a token is outside the cost table (0..{self.symbols - 1})")
        if not native:
            d = self._torch_expression(xb, yb)
        return 1 / (1 + d) if similarity else d

    def align(self, X, Y, ops=True):
        """The canonical optimal alignment of row p of X with row p of Y (P rows each, P may be 1) as an `Alignments`
        container on X's device: which symbols pair, which stay unaligned, and the identities (prograph_amd/alignments.py
        defines it).  `score` is this operator's distance.  Device byte tokens of at most 128 positions run on the HIP
        kernel `pg_alignment_trace`, wider ones up to 2048 positions on `pg_alignment_trace_long`; everything else on the
        exact, slow host expression.  `ops=False`: the same fields without the columns (`ops` is None; at most 128
        positions on `pg_alignment_stats`, which stores and walks nothing)."""
        return _alignments.align(self, X, Y, ops=ops)
