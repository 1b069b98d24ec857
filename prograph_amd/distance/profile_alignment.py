"""
Profile (PSSM) queries: local, semi-global and fit alignment scores of position-specific score matrices against tokenised,
zero right-padded sequences - NOT in the reference (acmater/prograph ships only hamming / minkowski); defined by this build.

    score = profile_alignment("fit", gap)                 # mode: "local", "semiglobal" or "fit"
    score = profile_alignment("local", gap, gap_open=o)   # affine: a run of g unaligned symbols costs o + g * gap
    s = score(X (N,D), profiles)                          # (Q, N) int64: profile q against row n of X

A profile is an integer array P of shape (L, A): position j has its own score P[j][a] for every symbol a - what a family's
alignment gives (`from_aligned`), or a motif with hard and soft positions, and what no single sequence plus one table can
say.  1 <= L <= 2048, 2 <= A <= 32, entries in -128..127, at least one entry of 1 or more (else no score is positive);
`ValueError` otherwise.  No symmetry is asked.  ALL L positions count: a profile has no padding and carries its own
length.  `profiles` is one (L, A) array, a (Q, L, A) array, or a list of (L_q, A) arrays of different lengths (one A).

The scores are those of `local_alignment`, `semiglobal_alignment` and `fit_alignment` with S[x_i, y_j] replaced by
P[j][x_i]; the profile is the Y operand, `gap` (1..255) and `gap_open` (0..255) are theirs:

  * "local": the best stretch of the profile against the best stretch of the row; at least 0.
  * "semiglobal": both end to end, the unaligned ends of either free; at least 0.
  * "fit": ALL of the profile within ANY stretch of the row - "where in this protein does the motif sit, and how well".
    -(o + e L) <= s: scores may be NEGATIVE.

Rows of X are sequences as everywhere: a row without its trailing zeros; an interior 0 - a letter outside the alphabet - is
symbol 0 and scores column 0 of the profile; padding never scores.  Tokens must be integers in 0..A-1.  All three are
SIMILARITIES: `similarity=False` raises.  The defining equivalence, entry for entry: the profile of a sequence y under a
symmetric table S, P[j][a] = S[y_j][a] (`from_sequence`), scores exactly what `local_alignment(S, ...)`,
`semiglobal_alignment(S, ...)` and `fit_alignment(S, ...)` score for y.

Device byte-token rows of at most 128 positions against profiles of at most 128 positions run on the HIP kernel
`pg_alignment_profile_dense`, up to 2048 positions on either side on the strip-mined `pg_alignment_profile_long_dense` (both
prograph_amd/csrc/pg_aln_profile.hip), inside the 16-bit cell bound of the mode's token kernels with max P for max S
(`_native.aln_local_long_fits`, `aln_semiglobal_long_fits`, `aln_fit_fits`).  Everything else is evaluated by an exact torch
expression on the device X lives on, CPU included: the `_dp_block` of the mode's score operator, whose gathered score term
St[y_i, x_j] reads a table with one row per (profile, position) instead of one per symbol.  It is the slow path.

Profiles are QUERIES only: `Prograph.search(profiles, k= | eps=, distance=score)` ranks the dataset against them
(prograph.py: `_search_profile`); `build_graph`, `align` and the identity cuts raise `ValueError`.  Tracebacks against a
profile are not built.
"""
import numpy as np
import torch

from .. import _native
from .alignment import _gap, _gap_open
from .fit_alignment import fit_alignment
from .hamming import _as_byte_tokens
from .levenshtein import _lengths
from .local_alignment import _DP_ELEMS, local_alignment
from .semiglobal_alignment import semiglobal_alignment

_DP_BLOCK = {"local": local_alignment._dp_block, "semiglobal": semiglobal_alignment._dp_block, "fit": fit_alignment._dp_block}


def _integer_array(T, what):
    """An integer-valued array as int64, or ValueError."""
    T = T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else np.asarray(T)
    if T.dtype == bool or not (np.issubdtype(T.dtype, np.integer) or np.issubdtype(T.dtype, np.floating)):
        raise ValueError(f"{what} must hold integers")
    if not np.issubdtype(T.dtype, np.integer) and (not np.all(np.isfinite(T)) or np.any(T != np.floor(T))):
        raise ValueError(f"{what} must hold integers")
    return T.astype(np.int64)


class Profiles:
    """Validated profiles: `list` of read-only (L_q, A) int8 arrays, `lengths`, `symbols` = A, `width` = the longest
    length, `top` = max(0, max P)."""

    def __init__(self, profiles):
        if isinstance(profiles, (list, tuple)):
            items = [_integer_array(p, "a profile") for p in profiles]
        else:
            P = _integer_array(profiles, "a profile")
            if P.ndim not in (2, 3):
                raise ValueError("profiles must be one (L, A) array, a (Q, L, A) array or a list of (L, A) arrays")
            items = [P] if P.ndim == 2 else list(P)
        if not items:
            raise ValueError("profiles must not be empty")
        for p in items:
            if p.ndim != 2 or not 1 <= p.shape[0] <= _native.ALN_LONG_MAX_L:
                raise ValueError(f"a profile must be an (L, A) array of 1..{_native.ALN_LONG_MAX_L} positions")
            if not 2 <= p.shape[1] <= _native.SUB_MAX_A:
                raise ValueError(f"a profile must have 2..{_native.SUB_MAX_A} symbols")
            if p.shape[1] != items[0].shape[1]:
                raise ValueError("the profiles of one call must have one number of symbols")
            if p.min() < _native.ALN_LOCAL_MIN or p.max() > _native.ALN_LOCAL_MAX:
                raise ValueError("the profile scores must be in -128..127")
            if p.max() < 1:
                raise ValueError("a profile must have an entry of at least 1 (else no score is positive)")
        self.list = [p.astype(np.int8) for p in items]           # copies of the caller's data
        for p in self.list:
            p.setflags(write=False)
        self.lengths = np.array([p.shape[0] for p in items], dtype=np.int64)
        self.symbols, self.width = int(items[0].shape[1]), int(self.lengths.max())
        self.top = max(int(p.max()) for p in items)

    def __len__(self):
        return len(self.list)

    def table(self, r0, r1, dev):
        """The profiles r0..r1-1 as the torch expression reads them: ((r1 - r0) * width, A) int32, row q * width + j =
        P_q[j] (zeros past a profile's length), and the (r1 - r0, width) int64 row numbers."""
        St = np.zeros((r1 - r0, self.width, self.symbols), dtype=np.int32)
        for q in range(r0, r1):
            St[q - r0, :self.lengths[q]] = self.list[q]
        ids = torch.arange((r1 - r0) * self.width, device=dev).view(r1 - r0, self.width)
        return torch.from_numpy(St.reshape(-1, self.symbols)).to(dev), ids


class profile_alignment:
    """The scores of one mode and gap penalty, linear or affine (see the module text)."""
    MODES = _native.ALN_PROFILE_MODES

    def __init__(self, mode, gap, gap_open=0):
        if mode not in self.MODES:
            raise ValueError(f"profile_alignment: mode must be one of {', '.join(repr(m) for m in self.MODES)}")
        self._mode = mode
        self._gap = _gap(gap)
        self._open = _gap_open(gap_open)

    @property
    def mode(self):
        return self._mode

    @property
    def gap(self):
        return self._gap

    @property
    def gap_open(self):
        """The price of opening a run of unaligned symbols, on top of `gap` per symbol; 0 is the linear penalty."""
        return self._open

    def __repr__(self):
        opening = f", gap_open={self._open}" if self._open else ""
        return f"profile_alignment({self._mode!r}, gap={self._gap}{opening})"

    # ------------------------------------------------------------------ the two helpers
    @staticmethod
    def from_sequence(tokens, S):
        """The (L, A) int64 profile of ONE sequence under an (A, A) integer table: P[j][a] = S[tokens[j]][a], L the
        sequence's length (trailing zeros are padding and are cut; at least one symbol must remain)."""
        S = _integer_array(S, "the score table")
        t = _integer_array(tokens, "the sequence").reshape(-1)
        if S.ndim != 2 or S.shape[0] != S.shape[1]:
            raise ValueError("the score table must be a square 2-D table")
        nz = np.nonzero(t)[0]
        if not len(nz):
            raise ValueError("from_sequence: an empty sequence has no profile")
        t = t[:nz[-1] + 1]
        if t.min() < 0 or t.max() >= S.shape[0]:
            raise ValueError(f"from_sequence: a token is outside the score table (0..{S.shape[0] - 1})")
        return S[t]

    @staticmethod
    def from_aligned(rows, symbols, background=None, pseudocount=1.0, scale=2.0):
        """A rounded log-odds PSSM, (L, symbols) int64, from R equal-length aligned token rows (R, L); host numpy.
        A 0 in a row - a gap of the alignment, or a letter outside the alphabet - is skipped in its column's counts:
            c[j][a] = the rows with rows[r][j] = a,  n[j] = sum over a of c[j][a]                     (a = 1..symbols-1)
            b[a]    = background[a] / sum of background[1:]   (None: uniform, 1 / (symbols - 1))
            f[j][a] = (c[j][a] + pseudocount * b[a]) / (n[j] + pseudocount)
            P[j][a] = clip(rint(scale * log2(f[j][a] / b[a])), -128, 127)                             (a = 1..symbols-1)
            P[j][0] = min over a >= 1 of P[j][a]        (an unknown letter scores as the position's worst known one)
        `pseudocount` > 0, `scale` > 0, every background[a], a >= 1, positive (background[0] is not read)."""
        rows = _integer_array(rows, "the aligned rows")
        A = int(symbols)
        if rows.ndim != 2 or rows.shape[0] == 0 or not 1 <= rows.shape[1] <= _native.ALN_LONG_MAX_L:
            raise ValueError(f"from_aligned: (R, L) aligned token rows, 1..{_native.ALN_LONG_MAX_L} columns")
        if not 2 <= A <= _native.SUB_MAX_A or rows.min() < 0 or rows.max() >= A:
            raise ValueError(f"from_aligned: 2..{_native.SUB_MAX_A} symbols, tokens in 0..symbols-1")
        if not pseudocount > 0 or not scale > 0:
            raise ValueError("from_aligned: pseudocount and scale must be positive")
        b = np.full(A, 1.0) if background is None else np.asarray(background, dtype=np.float64).reshape(-1).copy()
        if b.shape[0] != A or not np.all(np.isfinite(b[1:])) or not np.all(b[1:] > 0):
            raise ValueError("from_aligned: background must hold one positive frequency per symbol")
        b = b[1:] / b[1:].sum()
        c = np.stack([(rows == a).sum(axis=0) for a in range(1, A)], axis=1).astype(np.float64)      # (L, A - 1)
        f = (c + pseudocount * b) / (c.sum(axis=1, keepdims=True) + pseudocount)
        P = np.zeros((rows.shape[1], A), dtype=np.int64)
        P[:, 1:] = np.clip(np.rint(scale * np.log2(f / b)), -128, 127).astype(np.int64)
        P[:, 0] = P[:, 1:].min(axis=1)
        return P

    # ------------------------------------------------------------------ the routes
    def _fits(self, width_x, width_y, top):
        """Are the 16-bit cells of the mode's kernels exact at these widths (x: the rows, y: the longest profile)?"""
        if self._mode == "local":
            return _native.aln_local_long_fits(width_x, width_y, top)
        if self._mode == "semiglobal":
            return _native.aln_semiglobal_long_fits(width_x, width_y, top)
        return _native.aln_fit_fits(width_x, width_y, top, self._gap, self._open)

    def _select_bias(self, width_y):
        """What `search` adds to every score of a block before the selection layers, which sort non-negative values:
        -(the least fit score) of a profile `width_y` long; the other modes' scores are not negative."""
        return self._open + self._gap * int(width_y) if self._mode == "fit" else 0

    def _f16_route(self, width_x, width_y, top):
        """At most 128 positions, and every shifted score an integer that is exact in fp16 (0..2048)."""
        most = width_y * top if self._mode == "fit" else min(width_x, width_y) * top
        return (max(width_x, width_y) <= _native.ALN_MAX_L and self._fits(width_x, width_y, top)
                and self._select_bias(width_y) + most <= 2048)

    def _i32_route(self, width_x, width_y, top):
        """Everything else inside the cell bound, up to 2048 positions: int32 blocks of the strip-mined kernel."""
        return _native.aln_long_ready() and self._fits(width_x, width_y, top)

    def _native_dense(self, xo, po, out_bytes, rows=None, bias=0):
        return _native.alignment_profile_dense(self._mode, xo, po, self._gap, self._open, out_bytes=out_bytes, rows=rows, bias=bias)

    def _native_long_dense(self, xo, po, out_bytes, rows=None, bias=0):
        return _native.alignment_profile_long_dense(self._mode, xo, po, self._gap, self._open, out_bytes=out_bytes, rows=rows,
                                                    bias=bias)

    def _torch_expression(self, X, prof):
        """The definition as a torch expression: X (N, D) uint8, Profiles -> (Q, N) int64."""
        lx = _lengths(X)
        X = X[:, :max(int(lx.max()), 1)]
        n, q, dp = X.shape[0], len(prof), _DP_BLOCK[self._mode]
        cols = max(1, min(n, _DP_ELEMS // (X.shape[1] + 1)))
        rows = max(1, min(q, _DP_ELEMS // (cols * (X.shape[1] + 1))))
        out = torch.empty((q, n), dtype=torch.int64, device=X.device)
        for q0 in range(0, q, rows):
            q1 = min(q, q0 + rows)
            St, ids = prof.table(q0, q1, X.device)
            ly = torch.from_numpy(prof.lengths[q0:q1]).to(X.device)
            ids = ids[:, :int(ly.max())]
            for c0 in range(0, n, cols):
                out[q0:q1, c0:c0 + cols] = dp(self, St, X[c0:c0 + cols], lx[c0:c0 + cols], ids, ly)
        return out

    def __call__(self, X, profiles, similarity=True):
        """(Q, N) int64 scores of the Q profiles against the N rows of X.  A score is a similarity: `similarity=False`
        raises."""
        if not similarity:
            raise ValueError(f"profile_alignment: a {self._mode} profile score is a similarity (larger is nearer), not a "
                             "distance; there is no similarity=False form")
        prof = Profiles(profiles)
        X = torch.atleast_2d(torch.as_tensor(X))
        if X.dim() != 2 or X.shape[0] == 0 or X.shape[1] == 0:
            raise ValueError("profile_alignment: X must be a non-empty 2-D token array")
        xb = _as_byte_tokens(X)
        if xb is None:
            raise ValueError("profile_alignment: the tokens must be integers in 0..255")
        wx, wy = xb.shape[1], prof.width
        fits = xb.is_cuda and self._fits(wx, wy, prof.top)
        if fits:
            short = max(wx, wy) <= _native.ALN_MAX_L
            xo = (_native.aln_operand if short else _native.aln_long_operand)(xb, prof.symbols)
            po = _native.profile_operand(prof.list)
            s = (self._native_dense if short else self._native_long_dense)(xo, po, 8)
            inside = xo.valid()                                               # the pack's validity word: the one host sync
        else:
            inside = int(xb.max()) < prof.symbols
        if not inside:
            raise ValueError(f"profile_alignment: a token is outside the profiles' symbols (0..{prof.symbols - 1})")
        return s if fits else self._torch_expression(xb, prof)
