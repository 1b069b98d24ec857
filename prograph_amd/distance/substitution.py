"""
Substitution-matrix distance over tokenised, zero right-padded sequences - NOT in the reference (acmater/prograph
ships only hamming / minkowski); defined by this build.

    dist = substitution(C)                    # C: (A, A) cost table indexed by token value
    d = dist(X (N,D1), Y (M,D2))              # (M, N): d[m, n] = sum_j C[Y[m, j], X[n, j]]

`dist` follows the operator protocol of `hamming`: row m is Y[m] against every row of X, `torch.int64`, on the device of
X; `ValueError` on an empty operand; zero right-padding (`clean_input`) when the widths differ; `similarity=True`
returns 1/(1+d).  Token 0 - padding, or a letter outside the alphabet - is an ordinary index of C: row and column 0
of the table are the pad costs.  With C = 1 - I the distance is the Hamming distance.

The table: 2-D and square with 2 <= A <= 32, integer valued with entries in 0..255, symmetric, zero diagonal
(`ValueError` otherwise).  It is copied, so later edits of the caller's array do not reach the distance.  Operands must
hold integers in 0..A-1 (any dtype); anything else raises `ValueError`.

Device byte-token operands of at most 2048 positions run on the HIP kernel (`pg_substitution_dense`,
prograph_amd/csrc/pg_sub.hip).  Everything else is evaluated by the blocked torch expression
`Ct[Y.long()[:, None, :], X.long()[None, :, :]].sum(-1)` on the device the operands live on, CPU included.

`build_graph` and `search` recognise instances by type (prograph.py: `_build_graph_substitution`,
`_search_substitution`); two instances with equal tables behave identically.
"""
import numpy as np
import torch

from .. import _native
from .hamming import _as_byte_tokens
from .utils import clean_input

_GATHER_ELEMS = 1 << 24        # gathered table entries (pairs x positions) alive per block of the torch expression


def _integer_table(T, what):
    """2-D square integer-valued array as int64, or ValueError."""
    T = T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else np.asarray(T)
    if T.ndim != 2 or T.shape[0] != T.shape[1]:
        raise ValueError(f"{what} must be a square 2-D table")
    if T.dtype == bool or not (np.issubdtype(T.dtype, np.integer) or np.issubdtype(T.dtype, np.floating)):
        raise ValueError(f"{what} must hold integers")
    if not np.issubdtype(T.dtype, np.integer):
        if not np.all(np.isfinite(T)) or np.any(T != np.floor(T)):
            raise ValueError(f"{what} must hold integers")
    return T.astype(np.int64)


class substitution:
    """The distance of one cost table (see the module text)."""

    def __init__(self, C):
        C = _integer_table(C, "the cost table")
        if not 2 <= C.shape[0] <= _native.SUB_MAX_A:
            raise ValueError(f"the cost table must have 2..{_native.SUB_MAX_A} symbols")
        if C.min() < 0 or C.max() > 255:
            raise ValueError("the costs must be in 0..255")
        if not np.array_equal(C, C.T):
            raise ValueError("the cost table must be symmetric")
        if np.any(np.diag(C) != 0):
            raise ValueError("the cost table must have a zero diagonal")
        self._table = C.astype(np.uint8)             # a copy of the caller's data
        self._table.setflags(write=False)
        self._on = {}                                # device -> (A, A) int64 table of the torch expression
        self._cost = None                            # the 32 x 32 uint8 table of the kernel, on its device

    @property
    def table(self):
        """The (A, A) uint8 cost table (read-only)."""
        return self._table

    @property
    def symbols(self):
        return self._table.shape[0]

    @property
    def max_cost(self):
        return int(self._table.max())

    def __repr__(self):
        return f"substitution(<{self.symbols} x {self.symbols} table, costs up to {self.max_cost}>)"

    @classmethod
    def from_scores(cls, S):
        """The usual distance of a similarity score table (BLOSUM-like): C[a][b] = S[a][a] + S[b][b] - 2 S[a][b].
        `S` symmetric and integer; `ValueError` when a cost comes out negative or above 255."""
        S = _integer_table(S, "the score table")
        if not np.array_equal(S, S.T):
            raise ValueError("the score table must be symmetric")
        diag = np.diag(S)
        C = diag[:, None] + diag[None, :] - 2 * S
        if C.min() < 0 or C.max() > 255:
            raise ValueError("the scores give costs outside 0..255")
        return cls(C)

    @staticmethod
    def for_alphabet(M, letters, alphabet, pad):
        """Host-only helper: the table `M`, given for the symbols `letters`, in the token order of `alphabet` (letter j of
        `alphabet` is token j + 1, e.g. `pg.amino_acids`).  Row and column 0 - the padding / unknown token - are set to
        `pad`, entry (0, 0) to 0.  Returns the (len(alphabet) + 1)-square int64 array; a letter of `alphabet` that
        `letters` lacks raises `ValueError`."""
        M = np.asarray(M)
        letters = list(letters)
        if M.ndim != 2 or M.shape != (len(letters), len(letters)):
            raise ValueError("the table must have one row and one column per letter")
        at = {ch: i for i, ch in enumerate(letters)}
        missing = [ch for ch in alphabet if ch not in at]
        if missing:
            raise ValueError(f"the table has no entry for {missing}")
        order = np.array([at[ch] for ch in alphabet], dtype=np.int64)
        out = np.full((len(order) + 1, len(order) + 1), pad, dtype=np.int64)
        out[1:, 1:] = M[np.ix_(order, order)]
        out[0, 0] = 0
        return out

    # ------------------------------------------------------------------ the operator
    def _table_on(self, dev):
        key = str(dev)
        if key not in self._on:
            self._on[key] = torch.from_numpy(self._table.astype(np.int64)).to(dev)
        return self._on[key]

    def device_cost(self):
        """The kernel's 32 x 32 uint8 table on the current HIP device."""
        dev = _native.device()
        if self._cost is None or self._cost.device != dev:
            self._cost = _native.sub_cost(self._table)
        return self._cost

    def _torch_expression(self, X, Y):
        """The definition as a torch expression: X (N, D), Y (M, D) uint8 on one device -> (M, N) int64."""
        Ct = self._table_on(X.device)
        n, m, d = X.shape[0], Y.shape[0], X.shape[1]
        cols = max(1, min(n, _GATHER_ELEMS // d))
        rows = max(1, min(m, _GATHER_ELEMS // (cols * d)))
        out = torch.empty((m, n), dtype=torch.int64, device=X.device)
        Xl, Yl = X.long(), Y.long()
        for r0 in range(0, m, rows):
            for c0 in range(0, n, cols):
                out[r0:r0 + rows, c0:c0 + cols] = Ct[Yl[r0:r0 + rows, None, :], Xl[None, c0:c0 + cols, :]].sum(-1)
        return out

    def __call__(self, X, Y, similarity=False):
        """(M, N) distances (or similarities 1/(1+d)) of the M rows of Y against the N rows of X, int64."""
        X, Y = clean_input(X, Y)
        Y = Y.to(X.device)
        xb = _as_byte_tokens(X)
        yb = xb if Y is X else _as_byte_tokens(Y)
        if xb is None or yb is None:
            raise ValueError("substitution: the tokens must be integers in 0..255")
        if int(xb.max()) >= self.symbols or int(yb.max()) >= self.symbols:
            raise ValueError(f"substitution: a token is outside the cost table (0..{self.symbols - 1})")
        if xb.is_cuda and 1 <= xb.shape[1] <= _native.SUB_MAX_L:
            xo = _native.sub_operand(xb, self.symbols)
            yo = xo if yb is xb else _native.sub_operand(yb, self.symbols)
            d = _native.substitution_dense(xo, yo, self.device_cost(), out_bytes=8)
        else:
            d = self._torch_expression(xb, yb)
        return 1 / (1 + d) if similarity else d
