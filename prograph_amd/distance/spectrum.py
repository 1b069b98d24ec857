"""
k-mer spectrum distance over tokenised sequences of any lengths - NOT in the reference; defined by this build
(DESIGN.md §4.26).  Two sequences are compared by their k-mer CONTENT, without alignment: each becomes its vector of
k-mer counts (the spectrum kernel of Leslie et al.), and the vectors meet under the cosine or the Euclidean metric.

    dist = spectrum(k=3, symbols=20, dims=None, metric="cosine")
    d = dist(X (N, L1), Y (M, L2))            # (M, N) float32: cosine(dist.embed(X), dist.embed(Y))
    P = dist.embed(T)                         # (N, D) fp16 count profiles on the device T lives on; dist.D = D

The profile.  Tokens are 1..symbols; 0 is padding or a letter outside the alphabet and may stand anywhere.  For a row
t[0..l) window i (0 <= i <= l - k) COUNTS iff none of its k tokens is 0 - one rule for padding, rows shorter than k
(the zero profile) and unknown letters; `clean_input`'s zero padding therefore changes nothing.  Its code is
sum_j (t[i+j] - 1) * symbols^(k-1-j).  Exact mode (`dims=None`): D = symbols^k (at most 32768) and the window increments
bucket `code`.  Hashed mode (`dims` a power of two in 64..32768): D = dims and the bucket is
(((code + 1) * 2654435761) mod 2^32) >> (32 - log2 dims).  `ValueError` for k outside 1..6, symbols outside 2..255,
symbols^k above 2^31 (above 32768 in exact mode), any other `dims`, and a `metric` other than "cosine" / "euclidean".

`embed` takes a 2-D integer-valued token array or tensor (1-D: one row).  A token above `symbols`, a negative token or a
width above 2048 raises `ValueError`: beyond 2048 positions a count may no longer be exact in fp16.  Device tokens run
on the HIP kernel (`pg_spectrum_profile`, prograph_amd/csrc/pg_spectrum.hip); everything else is evaluated by the torch
expression `_torch_profiles` - windows by `unfold`, codes, `scatter_add` - on the device the tokens live on, CPU
included.  That expression is the definition in Python.

`dist` follows the operator protocol of `hamming`: row m is Y[m] against every row of X, on the device of X,
`ValueError` on an empty operand, `similarity=True` returns 1/(1+d); `build_graph` and `search` recognise instances by
type (prograph.py: `_build_graph_spectrum`, `_search_spectrum`).

Exactness.  With widths of at most 2048, p = x.y, nx = ||x||^2 and ny = ||y||^2 are integers of at most
(l-k+1)^2 <= 2^22, and nx + ny <= 2^23 < 2^24: every fp32 partial sum of the cosine tile routine is an integer below
2^24 and therefore exact, in whatever order it is taken.  Hence `metric="euclidean"` returns float32(sqrt(d^2)),
correctly rounded, of the EXACT integer squared distance - the cancellation tolerance of DESIGN.md §4.24 does not apply
here - and the cosine values are §4.9's epilogue on exact sums.

Equal profiles.  Two different sequences with the same k-mer multiset have distance 0.  They are treated like
duplicates: `eps` graphs drop them through (d > 0), and kNN ties go to the lower column.

Empty profiles.  A sequence shorter than k, or with an unknown in every window, has the zero profile.  Cosine then gives
d = 1 to everything (§4.9 rule 1); under Euclidean it is an ordinary point.
"""
import torch

from .. import _native
from .cosine import cosine
from .euclidean import euclidean
from .hamming import _as_byte_tokens
from .utils import clean_input

_METRICS = {"cosine": cosine, "euclidean": euclidean}
_HASH_MUL = 2654435761
_WINDOW_ELEMS = 1 << 24        # window tokens (rows x windows x k) alive per block of the torch expression


def _profile_width(k, symbols, dims):
    """D as pg_spectrum_dims gives it, or ValueError."""
    for name, v in (("k", k), ("symbols", symbols)) + ((("dims", dims),) if dims is not None else ()):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"spectrum: {name} must be an integer")
    if not 1 <= k <= _native.SPECTRUM_MAX_K:
        raise ValueError(f"spectrum: k must be in 1..{_native.SPECTRUM_MAX_K}")
    if not 2 <= symbols <= 255:
        raise ValueError("spectrum: symbols must be in 2..255")
    codes = int(symbols) ** int(k)
    if codes > 1 << 31:
        raise ValueError("spectrum: symbols^k must not exceed 2^31")
    if not dims:
        if dims is not None and dims != 0:
            raise ValueError("spectrum: dims must be None or a power of two in 64..32768")
        if codes > _native.SPECTRUM_MAX_D:
            raise ValueError(f"spectrum: symbols^k = {codes} exceeds {_native.SPECTRUM_MAX_D}; give dims= for hashed profiles")
        return codes
    if not 64 <= dims <= _native.SPECTRUM_MAX_D or dims & (dims - 1):
        raise ValueError("spectrum: dims must be None or a power of two in 64..32768")
    return int(dims)


class spectrum:
    """The k-mer spectrum distance of one (k, symbols, dims, metric) (see the module text)."""

    def __init__(self, k=3, symbols=20, dims=None, metric="cosine"):
        self.D = _profile_width(k, symbols, dims)
        if metric not in _METRICS:
            raise ValueError('spectrum: metric must be "cosine" or "euclidean"')
        self.k, self.symbols, self.dims, self.metric = int(k), int(symbols), int(dims or 0), metric

    def __repr__(self):
        return f"spectrum(k={self.k}, symbols={self.symbols}, dims={self.dims or None}, metric={self.metric!r})"

    @property
    def plain(self):
        """The embedding operator the profiles meet under: `cosine` or `euclidean`."""
        return _METRICS[self.metric]

    def _torch_profiles(self, T):
        """The definition as a torch expression: T (N, L) integer tokens in 0..symbols on one device -> (N, D) fp16."""
        n, l = T.shape
        k, dev = self.k, T.device
        out = torch.zeros((n, self.D), dtype=torch.int32, device=dev)
        if l >= k and n:
            power = torch.tensor([self.symbols ** (k - 1 - j) for j in range(k)], dtype=torch.int64, device=dev)
            shift = 32 - (self.dims.bit_length() - 1) if self.dims else 0
            rows = max(1, _WINDOW_ELEMS // ((l - k + 1) * k))
            for r0 in range(0, n, rows):
                w = T[r0:r0 + rows].to(torch.int64).unfold(1, k, 1)             # (rows, l - k + 1, k)
                counts = (w != 0).all(-1)
                code = ((w - 1) * power).sum(-1)
                bucket = (((code + 1) * _HASH_MUL) & 0xFFFFFFFF) >> shift if self.dims else code
                out[r0:r0 + rows].scatter_add_(1, torch.where(counts, bucket, torch.zeros_like(bucket)), counts.to(torch.int32))
        return out.to(torch.float16)

    def embed(self, T):
        """(N, D) fp16 k-mer count profiles of the token rows of T, on the device T lives on."""
        T = torch.as_tensor(T)
        if T.dim() == 1:
            T = T.reshape(1, -1)
        if T.dim() != 2:
            raise ValueError("spectrum: tokens must be a 1-D or 2-D array")
        if T.shape[1] > _native.SPECTRUM_MAX_L:
            raise ValueError(f"spectrum: at most {_native.SPECTRUM_MAX_L} positions per sequence (counts beyond are not exact in fp16)")
        if T.shape[0] == 0 or T.shape[1] == 0:
            return torch.zeros((T.shape[0], self.D), dtype=torch.float16, device=T.device)
        tb = _as_byte_tokens(T)
        if tb is None:
            raise ValueError(f"spectrum: the tokens must be integers in 0..{self.symbols}")
        if tb.is_cuda:
            prof, flags = _native.spectrum_profile(tb, self.k, self.symbols, self.dims)
            bad = bool(int(flags.item()))
        else:
            bad = int(tb.max()) > self.symbols
            prof = None if bad else self._torch_profiles(tb)
        if bad:
            raise ValueError(f"spectrum: a token is above symbols = {self.symbols}")
        return prof

    def __call__(self, X, Y, similarity=False):
        """(M, N) distances (or similarities 1/(1+d)) of the M rows of Y against the N rows of X, float32."""
        X, Y = clean_input(X, Y)
        ex = self.embed(X)
        ey = ex if Y is X else self.embed(Y.to(X.device))
        if self.metric == "euclidean" and not ex.is_cuda:
            return _euclidean_of_counts(ex, ey, similarity)
        return self.plain(ex, ey, similarity=similarity)


def _euclidean_of_counts(ex, ey, similarity):
    """`euclidean(ex, ey)` for count profiles that are not on the HIP device, with every float32 step formed in float64
    and rounded once more.  The sums are exact integers either way; for +, / and the square root that second rounding
    is innocuous (53 >= 2 * 24 + 2 bits), so each step is the correctly rounded float32 result whatever the host
    library's float32 root does - some builds of torch's CPU `sqrt` are an ulp off, and the contract here is bitwise."""
    a, b = ex.to(torch.float64), ey.to(torch.float64)
    p = b @ a.T
    d2 = ((a * a).sum(1)[None, :] + (b * b).sum(1)[:, None]) - (p + p)
    d = torch.sqrt(torch.clamp(d2, min=0)).to(torch.float32)
    if similarity:
        d = (1 / (1 + d.to(torch.float64)).to(torch.float32).to(torch.float64)).to(torch.float32)
    return d
