"""
Local alignment score (Smith-Waterman) over tokenised, zero right-padded sequences - NOT in the reference
(acmater/prograph ships only hamming / minkowski); defined by this build.

    score = local_alignment(S, gap)               # S: (A, A) SCORE table indexed by token value: larger is nearer
    score = local_alignment(S, gap, gap_open=o)   # affine: a run of g unaligned symbols costs o + g * gap
    s = score(X (N,D1), Y (M,D2))                 # (M, N): the best local alignment of Y[m] with X[n]

`alignment` is global: every symbol of both sequences is aligned or paid for.  This is its local counterpart: s(x, y) is
the best score, over all pairs of a substring of x and a substring of y and all alignments of the two, of the sum of
S[x_i, y_j] over the aligned pairs minus o + g * gap per maximal run of g unaligned symbols - what answers "do the two
share a domain, whatever surrounds it".  Gotoh's form, maximising, with a zero floor (e = gap):

    H[i][0] = H[0][j] = 0,   E[0][j] = F[i][0] = -inf,
    E[i][j] = max(E[i-1][j] - e, H[i-1][j] - o - e),   F[i][j] = max(F[i][j-1] - e, H[i][j-1] - o - e),
    H[i][j] = max(0, H[i-1][j-1] + S[x_i, y_j], E[i][j], F[i][j]),          s = max over all i, j of H[i][j].

s is symmetric, at least 0 (the empty alignment) and at most min(len x, len y) * max(S); gap_open = 0 is the linear gap
penalty.  It is a SIMILARITY, not a distance: there is no triangle inequality, s(x, x) depends on x, and larger is
nearer.  The operator owns that: `score(X, Y)` and `score(X, Y, similarity=True)` return the scores, `similarity=False`
raises `ValueError`; `build_graph` and `search` rank largest first whatever their `similarity` argument says.

    * a row's sequence is the row with its trailing zeros removed (an all-zero row is the empty sequence, which scores 0
      against everything), as for `alignment`; padding never scores, whatever S[a][0] is;
    * an interior zero - a letter outside the alphabet - is an ordinary symbol: row and column 0 of S;
    * the table: 2-D and square with 2..32 symbols, integers in -128..127, symmetric, at least one entry of 1 or more
      (else every score is 0); `ValueError` otherwise.  No rule for the diagonal.  It is copied;
    * `gap` is an integer in 1..255, `gap_open` one in 0..255, validated as `alignment` validates them;
    * operands must hold integers in 0..A-1 (any dtype); anything else raises `ValueError`; so does an empty operand.

Device byte-token operands of at most 128 positions run on the HIP kernel (`pg_alignment_local_dense`,
prograph_amd/csrc/pg_aln_local.hip); those of 129..2048 positions on the strip-mined kernel
(`pg_alignment_local_long_dense`, prograph_amd/csrc/pg_aln_long.hip) while width * max(S) + 255 <= 65 535, the bound of its
16-bit cells.  Everything else is evaluated by the torch expression below on the device the
operands live on, CPU included: the table row by row over the whole (M, N) batch in `alignment._dp_block_affine`'s style,
E carried between rows, A[j] = max(0, v_old[j-1] + S, E[j]), F[j] = cummax_{k<j}(A[k] + k e) - j e - o - a cell that sits
in a gap never opens a better gap than extending does, so the cummax may run over A -, v = max(A, F), and the running
maximum over the cells with j <= len x and i <= len y.  It is the slow path; it is exact.

`build_graph` and `search` recognise instances by type (prograph.py: `_build_graph_local`, `_search_local`); two
instances with equal table, gap and gap_open behave identically.

`score.align(X, Y)` returns the alignments themselves - row p of X with row p of Y - and `Prograph.align` those of a graph's
edges: see prograph_amd/alignments.py.

`_score_operator` below is everything but the recurrence: the table's rules, the routes and the blocking of the torch
expression.  `semiglobal_alignment` (semiglobal_alignment.py) and `fit_alignment` (fit_alignment.py) are its other
subclasses.
"""
import numpy as np
import torch

from .. import _native
from .. import alignments as _alignments
from .alignment import _gap, _gap_open
from .hamming import _as_byte_tokens
from .levenshtein import _lengths
from .substitution import _integer_table
from .utils import clean_input

_DP_ELEMS = 1 << 23            # table entries (pairs x columns) alive per block of the torch expression (E beside every row)


class _score_operator:
    """A similarity under one score table and gap penalty, linear or affine.  A subclass names its `_native` entries
    (looked up at every call) and the bound of the long kernel's cells, and gives `_dp_block`, the torch expression of its
    recurrence over one (m, n) batch."""
    _DENSE = _LONG_DENSE = _LONG_FITS = None
    _WHAT = None                                     # "a ... score", for the similarity=False error

    def __init__(self, S, gap, gap_open=0):
        S = _integer_table(S, "the score table")
        if not 2 <= S.shape[0] <= _native.SUB_MAX_A:
            raise ValueError(f"the score table must have 2..{_native.SUB_MAX_A} symbols")
        if S.min() < _native.ALN_LOCAL_MIN or S.max() > _native.ALN_LOCAL_MAX:
            raise ValueError("the scores must be in -128..127")
        if not np.array_equal(S, S.T):
            raise ValueError("the score table must be symmetric")
        if S.max() < 1:
            raise ValueError("the score table must have an entry of at least 1 (else every score is 0)")
        self._table = S.astype(np.int8)              # a copy of the caller's data
        self._table.setflags(write=False)
        self._gap = _gap(gap)
        self._open = _gap_open(gap_open)
        self._on = {}                                # device -> (A, A) int32 table of the torch expression
        self._score = None                           # the 32 x 32 int8 table of the kernel, on its device

    @property
    def table(self):
        """The (A, A) int8 score table (read-only)."""
        return self._table

    @property
    def gap(self):
        return self._gap

    @property
    def gap_open(self):
        """The price of opening a run of unaligned symbols, on top of `gap` per symbol; 0 is the linear penalty."""
        return self._open

    @property
    def symbols(self):
        return self._table.shape[0]

    @property
    def max_score(self):
        """The largest entry of the table.  A score is at most width * max_score."""
        return int(self._table.max())

    def __repr__(self):
        opening = f", gap_open={self._open}" if self._open else ""
        return (f"{type(self).__name__}(<{self.symbols} x {self.symbols} table, scores {int(self._table.min())}..{self.max_score}>, "
                f"gap={self._gap}{opening})")

    def device_score(self):
        """The kernel's 32 x 32 int8 table on the current HIP device."""
        dev = _native.device()
        if self._score is None or self._score.device != dev:
            self._score = _native.aln_local_score(self._table)
        return self._score

    # ------------------------------------------------------------------ the operator
    def _table_on(self, dev):
        key = str(dev)
        if key not in self._on:
            self._on[key] = torch.from_numpy(self._table.astype(np.int32)).to(dev)
        return self._on[key]

    def _native_dense(self, xo, yo, out_bytes, rows=None, bias=0):
        """The kernel up to 128 positions on two AlnOperands.  `bias`: `_select_bias`'s shift, 0 for every score that
        cannot be negative (only `fit_alignment`'s kernels take one)."""
        assert not bias
        return getattr(_native, self._DENSE)(xo, yo, self.device_score(), self._gap, self._open, out_bytes=out_bytes, rows=rows)

    def _native_long_dense(self, xo, yo, out_bytes, rows=None, bias=0):
        """The strip-mined kernel up to 2048 positions; exact inside `_long_fits`."""
        assert not bias
        return getattr(_native, self._LONG_DENSE)(xo, yo, self.device_score(), self._gap, self._open, out_bytes=out_bytes,
                                                   rows=rows)

    def _long_fits(self, width_x, width_y):
        return getattr(_native, self._LONG_FITS)(width_x, width_y, self.max_score)

    def _short_fits(self, width_x, width_y):
        """Is the kernel up to 128 positions exact at these widths?  Always, but for `fit_alignment`."""
        return True

    # what `Prograph._local_select` asks an instance (prograph.py): the shift that makes a block non-negative, and whether
    # operands of these widths (x: the columns, y: the rows / queries) take the fp16 or the int32 selection
    def _select_bias(self, width_y):
        return 0

    def _f16_route(self, width_x, width_y):
        """At most 128 positions, and every score - at most width * max(S) - an integer that is exact in fp16."""
        width = max(width_x, width_y)
        return width <= _native.ALN_MAX_L and width * self.max_score <= 2048

    def _i32_route(self, width_x, width_y):
        """Beyond 128 positions, with a device, inside the strip-mined kernel's 16-bit cells."""
        return (max(width_x, width_y) > _native.ALN_MAX_L and _native.aln_long_ready()
                and self._long_fits(width_x, width_y))

    def _torch_expression(self, X, Y):
        """The definition as a torch expression: X (N, D), Y (M, D) uint8 on one device -> (M, N) int64."""
        St = self._table_on(X.device)
        lx, ly = _lengths(X), _lengths(Y)
        X, Y = X[:, :int(lx.max())], Y[:, :int(ly.max())]
        n, m = X.shape[0], Y.shape[0]
        cols = max(1, min(n, _DP_ELEMS // (X.shape[1] + 1)))
        rows = max(1, min(m, _DP_ELEMS // (cols * (X.shape[1] + 1))))
        out = torch.empty((m, n), dtype=torch.int64, device=X.device)
        for r0 in range(0, m, rows):
            for c0 in range(0, n, cols):
                out[r0:r0 + rows, c0:c0 + cols] = self._dp_block(St, X[c0:c0 + cols], lx[c0:c0 + cols], Y[r0:r0 + rows],
                                                                 ly[r0:r0 + rows])
        return out

    def __call__(self, X, Y, similarity=True):
        """(M, N) int64 scores of the M rows of Y against the N rows of X.  A score is a similarity: `similarity=False`
        raises."""
        name = type(self).__name__
        if not similarity:
            raise ValueError(f"{name}: {self._WHAT} is a similarity (larger is nearer), not a distance; "
                             "there is no similarity=False form")
        X, Y = clean_input(X, Y)
        Y = Y.to(X.device)
        xb = _as_byte_tokens(X)
        yb = xb if Y is X else _as_byte_tokens(Y)
        if xb is None or yb is None:
            raise ValueError(f"{name}: the tokens must be integers in 0..255")
        native = xb.is_cuda and 1 <= xb.shape[1] <= _native.ALN_MAX_L and self._short_fits(xb.shape[1], yb.shape[1])
        long = (not native and xb.is_cuda and _native.aln_long_ready()
                and self._long_fits(xb.shape[1], yb.shape[1]))
        if long:                                                              # 129..2048 positions inside the 16-bit cells
            xo = _native.aln_long_operand(xb, self.symbols)
            yo = xo if yb is xb else _native.aln_long_operand(yb, self.symbols)
            s = self._native_long_dense(xo, yo, 8)
            native = True
            inside = int((xo.flags | yo.flags).item()) == 0
        elif native:
            xo = _native.aln_operand(xb, self.symbols)
            yo = xo if yb is xb else _native.aln_operand(yb, self.symbols)
            s = self._native_dense(xo, yo, 8)
            inside = int((xo.flags | yo.flags).item()) == 0                   # the packs' validity words: the one host sync
        else:
            inside = int(xb.max()) < self.symbols and int(yb.max()) < self.symbols
        if not inside:
            raise ValueError(f"{name}: a token is outside the score table (0..{self.symbols - 1})")
        if not native:
            s = self._torch_expression(xb, yb)
        return s

    def align(self, X, Y, ops=True):
        """The canonical optimal alignment of row p of X with row p of Y (P rows each, P may be 1) as an `Alignments`
        container on X's device: which symbols pair, which stay unaligned, where the alignment sits in either sequence,
        and the identities (prograph_amd/alignments.py defines it).  `score` is this operator's score.  Device byte tokens
        of at most 128 positions run on the HIP kernel `pg_alignment_trace`, wider ones up to 2048 positions on
        `pg_alignment_trace_long`; everything else on the exact, slow host expression.  `ops=False`: the same fields
        without the columns (`ops` is None; at most 128 positions on `pg_alignment_stats`, which stores and walks
        nothing)."""
        return _alignments.align(self, X, Y, ops=ops)


class local_alignment(_score_operator):
    """The score of one score table and gap penalty, linear or affine (see the module text)."""
    _DENSE, _LONG_DENSE, _LONG_FITS = "alignment_local_dense", "alignment_local_long_dense", "aln_local_long_fits"
    _WHAT = "a local alignment score"

    def _dp_block(self, St, x, lx, y, ly):
        """(m, n) int64 scores of y rows (lengths ly) against x rows (lengths lx); x, y already cut to the longest
        sequence among their rows.  Row i of every table at once; F is resolved inside the row by the cummax over A."""
        m, n, dx, e, o = y.shape[0], x.shape[0], x.shape[1], self._gap, self._open
        jg = torch.arange(dx + 1, device=x.device, dtype=torch.int32) * e
        v = torch.zeros((m, n, dx + 1), dtype=torch.int32, device=x.device)    # row 0: H[0][j] = 0
        E = torch.full_like(v, -(1 << 28))                                     # E[0][j] = -inf
        inside = (torch.arange(dx + 1, device=x.device).view(1, 1, -1) <= lx.view(1, n, 1))      # j <= len x
        best = torch.zeros((m, n), dtype=torch.int32, device=x.device)
        xl = x.long().view(1, n, dx)
        for i in range(1, y.shape[1] + 1):
            score = St[y[:, i - 1].long().view(m, 1, 1), xl]                   # (m, n, dx): S[y_i, x_j]
            E = torch.maximum(E - e, v - (o + e))                              # extend the run | open one from the row above
            A = torch.zeros_like(v)                                            # H[i][0] = 0
            A[..., 1:] = torch.maximum(v[..., :-1] + score, E[..., 1:]).clamp_(min=0)      # floor | aligned pair | gap against y_i
            F = torch.full_like(v, -(1 << 28))                                 # F[i][0] = -inf
            F[..., 1:] = torch.cummax(A + jg, dim=2).values[..., :-1] - jg[1:] - o         # max over k < j of A[k] - o - (j - k) e
            v = torch.maximum(A, F)
            live = inside & (ly >= i).view(m, 1, 1)                            # padding of either sequence never scores
            best = torch.maximum(best, torch.where(live, v, torch.zeros_like(v)).amax(dim=2))
        return best.to(torch.int64)
