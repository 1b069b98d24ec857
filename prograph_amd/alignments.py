"""
Alignment tracebacks: WHICH symbols the four alignment operators pair, not only what the pairing is worth.

    A = alignment(C, 1, gap_open=3).align(X, Y)        # row p of X with row p of Y; also local_ / semiglobal_ / fit_alignment
    A = pg.align(graph, distance=local_alignment(S, 1, 11))                        # one alignment per edge of a graph
    A.score, A.x_begin, A.x_end, A.y_begin, A.y_end, A.n_ops, A.identities, A.ops   # tensors, one row per pair
    A.identity(), A.cigar(p), A.gapped(p, letters), A.host(), len(A)

THE CANONICAL ALIGNMENT (the C ABI states it in include/prograph_hip.h).  The integer tables H, E, F are
the operator's own (i over the positions of x, j over those of y; E comes from row i - 1 and leaves x_i unaligned, F from
column j - 1 and leaves y_j unaligned; `alignment` minimises, its linear form is the affine one with gap_open = 0; the two
scores maximise).  Of all optimal alignments one is canonical:

  * end cell: global (len x, len y); local the cell of maximal H, ties to the smallest i, then the smallest j, and a
    maximum of 0 is the empty alignment (no ops, all four coordinates 0); semi-global the best of H[i][len y] and
    H[len x][j], the same ties; fit (`fit_alignment`: x has the free ends, y is whole) the best of H[i][len y],
    i = 0..len x, ties to the smallest i;
  * walk back from it in state H.  In H at (i, j): local stops where H[i][j] = 0 (tested first), semi-global where i = 0 or
    j = 0, global at (0, 0) - on i = 0 the j remaining symbols of y are left unaligned, on j = 0 the i of x; fit stops at
    j = 0 and on i = 0 leaves the j remaining symbols of y unaligned, so y_begin = 0, y_end = len y always and
    x_begin:x_end is where y sits.  Otherwise a
    pair if H[i][j] = H[i-1][j-1] + T[x_i][y_j], else state E if H[i][j] = E[i][j], else state F, at the same cell.  In E:
    x_i is unaligned; on to (i-1, j), in state H if E[i][j] equals the open term from H[i-1][j] (open wins a tie - with
    gap_open = 0 there always is one), else still in E.  F mirrors E along j.

Per pair: `score` (the operator's own value), the half-open ranges `x_begin:x_end`, `y_begin:y_end` of the positions the
alignment covers, `n_ops`, `ops` (forward order, left-aligned: 1 pair, 2 x symbol unaligned, 3 y symbol unaligned, 0 beyond
n_ops) and `identities`, the pairs with x_i = y_j.  Sequences are the operators': a row without its trailing zeros, an
interior zero is symbol 0, padding is never aligned.

Routes (`trace`).  Device byte tokens of at most 128 positions: the HIP kernel `pg_alignment_trace`
(prograph_amd/csrc/pg_aln_trace.hip).  Wider device tokens, up to 2048 positions: `pg_alignment_trace_long`
(pg_aln_trace.hip), the same tables in strips of 128 columns, the same alignment field for field.
Everything else - CPU tensors, widths beyond 2048, no device - `host_trace` below: one pair at a time, the three tables
row by row in numpy (F by the running maximum over A, as the operators' torch expressions have it), then the walk over
the stored tables.  It is SLOW (milliseconds per pair at 128 positions, and the tables of one pair take 24 bytes per
cell); it is exact.

WITHOUT THE COLUMNS (`ops=False`).  A percent-identity cut wants `identities / n_ops` of every edge and
throws the columns away.  `pg_alignment_stats` (pg_aln_stats.hip) gives the seven fields of the SAME canonical alignment
from the forward pass alone: every cell carries the counts of the predecessor the walk would choose, so nothing is stored
per cell and nothing is walked back - 32 bytes out per pair, no workspace.  `Prograph.build_graph(..., min_identity=)` and
`Prograph.search(..., min_identity=)` filter a graph's edges by it.
"""
import numpy as np
import torch

from . import _native

GLOBAL, LOCAL, SEMIGLOBAL = _native.ALN_TRACE_GLOBAL, _native.ALN_TRACE_LOCAL, _native.ALN_TRACE_SEMIGLOBAL
FIT = _native.ALN_TRACE_FIT
_NEG = -(1 << 40)
_DIGITS = "0123456789abcdefghijklmnopqrstuv"        # a token as one character when no letters are given
_FIELDS = ("score", "x_begin", "x_end", "y_begin", "y_end", "n_ops", "identities")


class Alignments:
    """P canonical alignments.  Tensor fields on one device: score, x_begin, x_end, y_begin, y_end, n_ops, identities
    (int64 (P,)) and ops (uint8 (P, W); None when built with `ops=False`: `cigar` and `gapped` then raise ValueError, every
    field, `identity()`, `host()` and `len` work).  `x`, `y` are the token matrices the pairs index through `xi`, `yi` (row p is
    x[xi[p]] against y[yi[p]]), kept for `gapped`."""

    def __init__(self, score, x_begin, x_end, y_begin, y_end, n_ops, identities, ops, x=None, y=None, xi=None, yi=None,
                 letters=None):
        self.score, self.x_begin, self.x_end, self.y_begin, self.y_end = score, x_begin, x_end, y_begin, y_end
        self.n_ops, self.identities, self.ops = n_ops, identities, ops
        self.x, self.y, self.xi, self.yi, self.letters = x, y, xi, yi, letters

    def __len__(self):
        return int(self.score.shape[0])

    def __repr__(self):
        ops = "no ops" if self.ops is None else f"ops {tuple(self.ops.shape)}"
        return f"Alignments({len(self)} pairs, {ops}, {self.score.device})"

    def identity(self):
        """identities / n_ops per pair as float64, 0 for an empty alignment."""
        n = self.n_ops.to(torch.float64)
        return torch.where(n > 0, self.identities.to(torch.float64) / n.clamp(min=1), torch.zeros_like(n))

    def host(self):
        """The same container with every tensor field on the CPU."""
        c = lambda t: t if t is None or not isinstance(t, torch.Tensor) else t.cpu()
        return Alignments(*(c(getattr(self, f)) for f in _FIELDS), c(self.ops), c(self.x), c(self.y), c(self.xi), c(self.yi),
                          self.letters)

    def _ops_of(self, p):
        if self.ops is None:                                                # trace(..., ops=False): the statistics alone
            raise ValueError("built without ops")
        return self.ops[p, :int(self.n_ops[p])].cpu().numpy()

    def cigar(self, p):
        """Run-length string of pair p over M (pair), X (x symbol unaligned), Y (y symbol unaligned); '' when empty."""
        ops = self._ops_of(p)
        if not len(ops):
            return ""
        cut = np.flatnonzero(np.diff(ops)) + 1
        starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [len(ops)]])
        return "".join(f"{b - a}{' MXY'[ops[a]]}" for a, b in zip(starts.tolist(), ends.tolist()))

    def _row(self, mat, idx, p):
        if mat is None:
            raise ValueError("this container was built without its sequences")
        r = p if idx is None else int(idx[p])
        return np.asarray(mat[r].cpu() if isinstance(mat, torch.Tensor) else mat[r]).astype(np.int64)

    def gapped(self, p, letters=None):
        """The two rows of alignment p as strings of one length, '-' where a symbol of the other row is unaligned;
        `letters[t]` is the character of token t (default: the container's, else 0-9a-v)."""
        letters = letters or self.letters or _DIGITS
        x, y = self._row(self.x, self.xi, p), self._row(self.y, self.yi, p)
        i, j, a, b = int(self.x_begin[p]), int(self.y_begin[p]), [], []
        for op in self._ops_of(p).tolist():
            a.append(letters[x[i]] if op != 3 else "-")
            b.append(letters[y[j]] if op != 2 else "-")
            i += op != 3
            j += op != 2
        return "".join(a), "".join(b)


# ---------------------------------------------------------------------------------------------- the host expression
def _host_pair(mode, T, e, o, x, y):
    """One pair: (score, x_begin, x_end, y_begin, y_end, identities, ops list).  T maximises (the distance hands in -C)."""
    lx, ly, oe = len(x), len(y), o + e
    jg = np.arange(ly + 1, dtype=np.int64) * e
    H = np.zeros((lx + 1, ly + 1), dtype=np.int64)
    E = np.full((lx + 1, ly + 1), _NEG, dtype=np.int64)
    F = np.full((lx + 1, ly + 1), _NEG, dtype=np.int64)
    if mode == GLOBAL:
        H[0, 1:] = -o - jg[1:]
        H[1:, 0] = -o - np.arange(1, lx + 1, dtype=np.int64) * e
    if mode == FIT:
        H[0, 1:] = -o - jg[1:]                                              # all of y is paid for; column 0 stays 0
    for i in range(1, lx + 1):
        E[i, 1:] = np.maximum(E[i - 1, 1:] - e, H[i - 1, 1:] - oe)
        A = np.empty(ly + 1, dtype=np.int64)
        A[0] = H[i, 0]
        A[1:] = np.maximum(H[i - 1, :-1] + T[x[i - 1], y], E[i, 1:])
        if mode == LOCAL:
            np.maximum(A, 0, out=A)
        F[i, 1:] = np.maximum.accumulate(A + jg)[:-1] - jg[1:] - o         # max over k < j of A[k] - o - (j - k) e
        H[i] = np.maximum(A, F[i])
    if mode == GLOBAL:
        bi, bj = lx, ly
    elif mode == LOCAL:
        bi, bj = (int(v) for v in np.unravel_index(np.argmax(H), H.shape))  # the first maximum in row-major order
        if H[bi, bj] == 0:
            bi = bj = 0
    elif mode == FIT:
        bi, bj = int(np.argmax(H[:, ly])), ly                               # the first maximum: the smallest i
    else:
        col, row = H[:, ly], H[lx, :]
        top = max(int(col.max()), int(row.max()))
        ci = int(np.argmax(col))
        bi, bj = (ci, ly) if col[ci] == top and ci < lx else (lx, int(np.argmax(row == top)))
    score = int(H[bi, bj])
    i, j, state, ops, ident = bi, bj, 0, [], 0
    while True:
        if state == 0:
            if mode == LOCAL and H[i, j] == 0:
                break
            if i == 0 or j == 0:
                if mode == GLOBAL:
                    ops += [3] * j if i == 0 else [2] * i
                    i = j = 0
                if mode == FIT:                                             # the rest of y unaligned; x's prefix is free
                    ops += [3] * j
                    j = 0
                break
            if H[i, j] == H[i - 1, j - 1] + T[x[i - 1], y[j - 1]]:
                ops.append(1)
                ident += int(x[i - 1] == y[j - 1])
                i, j = i - 1, j - 1
            else:
                state = 1 if H[i, j] == E[i, j] else 2
        elif state == 1:
            ops.append(2)
            if E[i, j] == H[i - 1, j] - oe:
                state = 0
            i -= 1
        else:
            ops.append(3)
            if F[i, j] == H[i, j - 1] - oe:
                state = 0
            j -= 1
    return (-score if mode == GLOBAL else score), i, bi, j, bj, ident, ops[::-1]


def host_trace(mode, table, gap, gap_open, X, Y, xi=None, yi=None):
    """The canonical alignments of the pairs (X[xi[p]], Y[yi[p]]) (all rows in order when the lists are None) on the host:
    X, Y integer numpy token matrices inside the table.  Returns the numpy fields (score, x_begin, x_end, y_begin, y_end,
    n_ops, identities, ops (P, width X + width Y)).  Slow: see the module text."""
    T = np.asarray(table, dtype=np.int64)
    if mode == GLOBAL:
        T = -T
    X, Y = np.asarray(X), np.asarray(Y)
    xi = np.arange(len(X)) if xi is None else np.asarray(xi, dtype=np.int64)
    yi = np.arange(len(Y)) if yi is None else np.asarray(yi, dtype=np.int64)
    P = len(xi)
    fields = np.zeros((7, P), dtype=np.int64)
    ops = np.zeros((P, X.shape[1] + Y.shape[1]), dtype=np.uint8)
    for p in range(P):
        x, y = X[xi[p]].astype(np.intp), Y[yi[p]].astype(np.intp)
        nx, ny = np.flatnonzero(x), np.flatnonzero(y)
        x, y = x[:nx[-1] + 1 if len(nx) else 0], y[:ny[-1] + 1 if len(ny) else 0]
        s, xb, xe, yb, ye, ident, o = _host_pair(mode, T, int(gap), int(gap_open), x, y)
        fields[:, p] = (s, xb, xe, yb, ye, len(o), ident)
        ops[p, :len(o)] = o
    return (*fields, ops)


# ---------------------------------------------------------------------------------------------- routes
def _mode_of(op):
    from .distance import alignment, fit_alignment, local_alignment, semiglobal_alignment
    for cls, mode in ((alignment, GLOBAL), (local_alignment, LOCAL), (semiglobal_alignment, SEMIGLOBAL), (fit_alignment, FIT)):
        if isinstance(op, cls):
            return mode
    raise TypeError("align: distance must be an alignment, local_alignment or semiglobal_alignment instance, or a "
                    f"fit_alignment one, not {op!r}")


def _device_table(op, mode):
    return op.device_cost() if mode == GLOBAL else op.device_score()


def from_head(head, ops, **kept):
    """Alignments from the (P, 8) head and the ops of pg_alignment_trace / pg_alignment_trace_long (ops None: from the
    head of pg_alignment_stats alone)."""
    h = head.to(torch.int64)
    return Alignments(*(h[:, c].contiguous() for c in range(7)), ops, **kept)


def trace(op, X, Y, xi=None, yi=None, workspace_bytes=None, letters=None, native=None, native_long=None, ops=True):
    """The alignments of the pairs (X[xi[p]], Y[yi[p]]) under operator `op`; X, Y uint8 token tensors on one device,
    xi, yi integer lists (None: every row in order, X and Y of one height).  The 128-position kernel for device tokens of
    at most 128 positions (`native` overrides that choice), the strip kernel for wider ones up to 2048 positions where
    `_native.aln_trace_long_ready()` (`native_long` overrides that one), `host_trace` otherwise; the result lives on X's
    device.  `workspace_bytes` None: 256 MiB for the first kernel, what the list needs up to 2 GiB for the second.
    `ops=False`: the same fields without the columns (the container's `ops` is None) - at most 128 positions on
    `pg_alignment_stats`, which has no workspace; 129..2048 positions on the strip kernel in slices of the pair list that
    share one ops buffer of at most 256 MiB (`_native.alignment_trace_long_heads`); `host_trace` otherwise, its ops dropped.
    `workspace_bytes` is not consulted then."""
    mode = _mode_of(op)
    name = type(op).__name__
    dev = X.device
    width = max(X.shape[1], Y.shape[1])
    if xi is None:
        if X.shape[0] != Y.shape[0]:
            raise ValueError(f"{name}.align: X and Y must have one row per pair ({X.shape[0]} and {Y.shape[0]} rows)")
        xi = yi = torch.arange(X.shape[0], dtype=torch.int32, device=dev)
    xi, yi = torch.as_tensor(xi).reshape(-1), torch.as_tensor(yi).reshape(-1)
    if xi.numel() != yi.numel():
        raise ValueError(f"{name}.align: as many rows as columns make the pairs")
    if xi.numel() == 0:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        none = torch.zeros((0, X.shape[1] + Y.shape[1]), dtype=torch.uint8, device=dev) if ops else None
        return Alignments(z, z, z, z, z, z, z, none, X, Y, xi, yi, letters)
    if native is None:
        native = X.is_cuda and 1 <= width <= _native.ALN_MAX_L
    if native_long is None:
        native_long = (not native and X.is_cuda and _native.ALN_MAX_L < width <= _native.ALN_LONG_MAX_L
                       and _native.aln_trace_long_ready())
    if native or native_long:
        operand, tracer = ((_native.aln_operand, _native.alignment_trace) if native else
                           (_native.aln_long_operand, _native.alignment_trace_long))
        xo = operand(X, op.symbols)
        yo = xo if Y is X else operand(Y, op.symbols)
        if ops:
            head, cols = tracer(xo, yo, xi, yi, mode, _device_table(op, mode), op.gap, op.gap_open,
                                workspace_bytes=256 << 20 if native and workspace_bytes is None else workspace_bytes)
        else:
            heads = _native.alignment_stats if native else _native.alignment_trace_long_heads
            head, cols = heads(xo, yo, xi, yi, mode, _device_table(op, mode), op.gap, op.gap_open), None
        if int((xo.flags | yo.flags).item()):
            raise ValueError(f"{name}: a token is outside the table (0..{op.symbols - 1})")
        return from_head(head, cols, x=X, y=Y, xi=xi, yi=yi, letters=letters)
    if int(X.max()) >= op.symbols or int(Y.max()) >= op.symbols:
        raise ValueError(f"{name}: a token is outside the table (0..{op.symbols - 1})")
    xh, yh = xi.cpu().numpy(), yi.cpu().numpy()
    if xh.min() < 0 or xh.max() >= X.shape[0] or yh.min() < 0 or yh.max() >= Y.shape[0]:
        raise IndexError(f"{name}.align: a pair's row number is outside its operand")
    *fields, cols = host_trace(mode, op.table, op.gap, op.gap_open, X.cpu().numpy(), Y.cpu().numpy(), xh, yh)
    return Alignments(*(torch.from_numpy(f).to(dev) for f in fields), torch.from_numpy(cols).to(dev) if ops else None,
                      X, Y, xi, yi, letters)


def align(op, X, Y, ops=True):
    """`op.align(X, Y)`: row p of X aligned with row p of Y (see the module text; `fit_alignment`: row p of Y, whole,
    within row p of X); the operators' input rules.  `ops=False`: `trace`'s."""
    from .distance.hamming import _as_byte_tokens
    from .distance.utils import clean_input
    name = type(op).__name__
    X, Y = clean_input(X, Y)
    Y = Y.to(X.device)
    xb = _as_byte_tokens(X)
    yb = xb if Y is X else _as_byte_tokens(Y)
    if xb is None or yb is None:
        raise ValueError(f"{name}: the tokens must be integers in 0..255")
    return trace(op, xb, yb, ops=ops)
