"""
An exact model of the cosine / Euclidean contract of prograph_amd/csrc/pg_cos.hip, numpy only.

Input family: v = ints * 2^s with integer entries in [-A, A], one exponent s per vector and D * A^2 < 2^24.  Every element
is exactly an fp16 value (`Operand.values` asserts it), and p = sum x_k y_k, nx = sum x_k^2, ny = sum y_k^2 are integers
below 2^24 times a power of two: exact in fp32 in whatever order they are accumulated.  The model forms them in int64 and
scales them, then takes the epilogues in numpy float32 step for step as `cs_finish` and `eu_finish` write them.  Roots are
taken in float64 and rounded to float32 (53 >= 2 * 24 + 2 bits: the double rounding is innocuous, and
tests/test_exact_sums_model_cpu.py checks the results in integer arithmetic); every other step is one numpy float32
operation, which rounds once.  With exponents >= -24 no fp32 intermediate is subnormal (the smallest non-zero sum is
2^-48, the largest reciprocal root 2^24).

The device results are compared with this model on bit patterns (tests/test_cosine_exact_gpu.py).  The case lists of that
test live here, so that the CPU test can show on the same data that the mutants below differ from the model.
"""
import math

import numpy as np

F32 = np.float32
A_CAP = 2047                              # 11 significant bits: an integer up to 2047 times 2^s is an fp16 value
EXPONENT_SETS = ("zero", "low", "mixed")  # every vector 2^0; every vector 2^-14; -14..4 per vector
DIMS_SMALL = tuple(range(1, 145))         # N = 70, M = 40: every remainder of the unrolled chunk-pair loop, odd chunk counts
DIMS_LARGE = (1279, 1280, 1281)           # N = 300, M = 77
EDGE_N, EDGE_M, EDGE_D = (1, 2, 31, 32, 33, 257), (1, 31, 33, 129), (9, 64)   # the 32 x 32 tile, the 128-row workgroup
SUBNORMAL_DIMS = (1, 7, 8, 9, 16, 17, 64, 100, 144, 1281)


def amplitude(d):
    """The largest A <= 2047 with d * A^2 < 2^24."""
    a = min(A_CAP, math.isqrt((2 ** 24 - 1) // d))
    assert d * a * a < 2 ** 24 and a >= 1
    return a


class Operand:
    """n vectors ints[i] * 2^exps[i]."""

    def __init__(self, ints, exps):
        self.ints, self.exps = np.asarray(ints, dtype=np.int64), np.asarray(exps, dtype=np.int64)
        assert self.ints.ndim == 2 and self.exps.shape == (len(self.ints),)
        assert self.ints.shape[1] * int(np.abs(self.ints).max(initial=0)) ** 2 < 2 ** 24

    @property
    def n(self):
        return len(self.ints)

    def values(self):
        """The (n, D) float16 matrix; every element exact."""
        v = np.ldexp(self.ints.astype(np.float64), self.exps[:, None])
        with np.errstate(over="ignore"):
            h = v.astype(np.float16)
        assert np.isfinite(h).all() and np.array_equal(h.astype(np.float64), v), "an element is not an fp16 value"
        return h

    def has_fp16_subnormals(self):
        v = np.abs(np.ldexp(self.ints.astype(np.float64), self.exps[:, None]))
        return bool(((v > 0) & (v < 2.0 ** -14)).any())


def _exponents(rng, n, kind):
    if kind == "zero":
        return np.zeros(n, dtype=np.int64)
    if kind == "low":
        return np.full(n, -14, dtype=np.int64)
    if kind == "mixed":
        return rng.integers(-14, 5, n)
    if kind == "subnormal":
        return rng.integers(-24, -19, n)
    raise ValueError(kind)


def _copy(dst, i, src, j, sign=1):
    if i < dst.n and j < src.n:
        dst.ints[i], dst.exps[i] = sign * src.ints[j], src.exps[j]


def plant(x, y):
    """Planted rows, each where the operands are large enough: duplicates in X across the lane halves of a tile (rows 2 /
    5), across two tiles (31 / 32) and far apart (10 / last), a zero vector on each side, Y rows equal to X rows (one in
    another tile), and opposite vectors in X and between Y and X."""
    _copy(x, x.n - 1, x, 10)
    _copy(x, 5, x, 2)
    _copy(x, 32, x, 31)
    _copy(x, 41, x, 40, -1)
    _copy(y, 3, x, 33)
    _copy(y, 4, x, 4)
    _copy(y, 12, x, 6, -1)
    if x.n > 20:
        x.ints[20] = 0
    if y.n > 7:
        y.ints[7] = 0
    return x, y


def make_case(d, n, m, kind, planted=True):
    """(X, Y) Operands of the family at dimension d: entries uniform in [-A, A] with A = amplitude(d)."""
    rng = np.random.default_rng([d, n, m, EXPONENT_SETS.index(kind) if kind in EXPONENT_SETS else 7])
    a = amplitude(d)
    x = Operand(rng.integers(-a, a + 1, (n, d)), _exponents(rng, n, kind))
    y = Operand(rng.integers(-a, a + 1, (m, d)), _exponents(rng, m, kind))
    return plant(x, y) if planted else (x, y)


def dimension_cases(dims, n, m):
    return [(d, n, m, kind) for d in dims for kind in EXPONENT_SETS]


def edge_cases():
    return [(d, n, m, "mixed") for d in EDGE_D for n in EDGE_N for m in EDGE_M]


def grid_case(d, n=600, m=77, seed=0):
    """Tie-saturated data: points of the integer grid {0..7}^d, exponents 0 (many equal distances, many duplicates)."""
    rng = np.random.default_rng([d, seed])
    return (Operand(rng.integers(0, 8, (n, d)), np.zeros(n, dtype=np.int64)),
            Operand(rng.integers(0, 8, (m, d)), np.zeros(m, dtype=np.int64)))


# ---------------------------------------------------------------- the sums
def _f32_exact(ints, exps):
    v = np.ldexp(ints.astype(np.float64), exps)
    f = v.astype(F32)
    assert np.array_equal(f.astype(np.float64), v) and (np.abs(ints) < 2 ** 24).all()
    return f


def norms(x):
    """(n = sum v^2, r = 1/sqrt(n)) as float32: n exact, the root rounded once and the quotient rounded once (1/0 = inf)."""
    n = _f32_exact((x.ints * x.ints).sum(1), 2 * x.exps)
    root = np.sqrt(n.astype(np.float64)).astype(F32)
    with np.errstate(divide="ignore"):
        r = F32(1) / root
    return n, r


def products(x, y):
    """(M, N) float32: p of every Y vector against every X vector, exact."""
    return _f32_exact(y.ints @ x.ints.T, y.exps[:, None] + x.exps[None, :])


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _identical(p, nx, ny):
    return (_bits(p) == _bits(nx)[None, :]) & (_bits(p) == _bits(ny)[:, None])


def _similarity(d):
    return F32(1) / (F32(1) + d)


# ---------------------------------------------------------------- the epilogues
def cosine_block(x, y, similarity=False, variant="contract"):
    """cs_finish on every pair.  variant: "contract" (the model), or one of the two mutants the present tolerance lets
    through - "swapped" multiplies (p * rx) * ry, "fused" takes 1 - t * rx with one rounding (t = p * ry rounded), what an
    fma contraction of the subtraction gives."""
    p = products(x, y)
    (nx, rx), (ny, ry) = norms(x), norms(y)
    with np.errstate(invalid="ignore", over="ignore"):
        if variant == "contract":
            c = (p * ry[:, None]) * rx[None, :]
            d = F32(1) - c
        elif variant == "swapped":
            c = (p * rx[None, :]) * ry[:, None]
            d = F32(1) - c
        elif variant == "fused":
            t = p * ry[:, None]
            # t * rx is exact in float64 (24 x 24 bits); the difference is then rounded to float64 and to float32, which
            # differs from the single rounding of an fma only on a float32 tie of the float64 value: good enough for a mutant
            d = (1.0 - t.astype(np.float64) * rx[None, :].astype(np.float64)).astype(F32)
        else:
            raise ValueError(variant)
        d = np.minimum(np.maximum(d, F32(0)), F32(2))
    d = np.where(_identical(p, nx, ny), F32(0), d)
    d = np.where((nx == 0)[None, :] | (ny == 0)[:, None], F32(1), d).astype(F32)
    return _similarity(d) if similarity else d


def euclidean_block(x, y, similarity=False):
    """eu_finish on every pair."""
    p = products(x, y)
    (nx, _), (ny, _) = norms(x), norms(y)
    sq = np.maximum((nx[None, :] + ny[:, None]) - (p + p), F32(0))
    assert sq.dtype == F32
    d = np.sqrt(sq.astype(np.float64)).astype(F32)
    d = np.where(_identical(p, nx, ny), F32(0), d).astype(F32)
    return _similarity(d) if similarity else d


BLOCKS = {"cosine": cosine_block, "euclidean": euclidean_block}


# ---------------------------------------------------------------- selection over a block
def knn(block, k, first, similarity=False):
    """Ranks first..first+k-1 of every row in (value, column) order, descending values for similarities; ranks the row
    does not have: idx -1, weight 0."""
    m, n = block.shape
    order = np.argsort(-block if similarity else block, axis=1, kind="stable")[:, first:first + k]
    idx = np.full((m, k), -1, dtype=np.int32)
    w = np.zeros((m, k), dtype=F32)
    idx[:, :order.shape[1]] = order
    w[:, :order.shape[1]] = np.take_along_axis(block, order, 1)
    return idx, w


_COMPARE = (np.less_equal, np.less, np.equal, np.greater_equal, np.greater)        # CMP_LE .. CMP_GT


def eps_csr(block, cmp, eps, similarity=False, keep_zero=False):
    """CSR of comp(d, eps) & (d > 0), or comp(eps, s) & (s < 1) for similarities; keep_zero: without the second test."""
    e = F32(eps)
    hit = _COMPARE[cmp](e, block) if similarity else _COMPARE[cmp](block, e)
    if not keep_zero:
        hit &= (block < 1) if similarity else (block > 0)
    rows, cols = np.nonzero(hit)
    indptr = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.int64)
    return indptr, cols.astype(np.int32), block[rows, cols]


def thresholds(block, similarity):
    """Two values of the block (so that == has hits) away from the excluded value: the 3 % and the 50 % quantile."""
    v = np.sort(block.reshape(-1))
    v = v[(v < 1) if similarity else (v > 0)]
    return [float(v[int(q * (len(v) - 1))]) for q in (0.03, 0.5)]
