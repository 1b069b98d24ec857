"""
Interval model of the fp16 Minkowski (p = 2) values and the seeded data the Minkowski value tests share
(numpy only: nothing here touches torch, the library or a device).

What the reference's fp16 tensor expression - and pg_minkowski_dense - compute for a pair (x, y) of fp16 vectors:

    diff = y - x, sq = diff * diff    one correctly rounded fp16 operation each
    s    = the squares summed in fp32, in SOME order (torch vectorises it, the kernel goes chunk by chunk)
    d    = f16(sqrt(f32(f16(s))));  similarity: t = f16(1 + d), f16(1 / f32(t))

Only `s` depends on the order, so the model bounds it instead of guessing the order:

    T = sq * 2^24 as int64 (fp16 values are multiples of 2^-24), S = sum(T): the exact sum, < 2^53 for D <= 4096.
    Any sequence of fp32 additions of D non-negative terms is off by at most g * S,
    g = D * 2^-24 / (1 - D * 2^-24) (the usual gamma bound, with one addition to spare).
    The error is ZERO when S == 0 and when S < 2^24 * lowbit(OR of the terms): then every partial sum of every
    order is a multiple of that bit and below 2^24 of them, i.e. an fp32 value - integer data, tiny data.
    lo16 = f16(f32(S (1 - g))), hi16 = f16(f32(S (1 + g))): equal or adjacent fp16 values.

A pair's allowed values are finish(lo16) and finish(hi16); it is DECIDED when the two are equal, and then the
comparison is bit for bit.  A pair with a non-finite square (the difference or its square overflowed) is inf
(similarity 0) whatever the order.  sqrt and the division run in fp32 and round to fp16 once more, which equals
the correctly rounded fp16 result (24 >= 2 * 11 + 2), so `finish` needs no interval of its own.
"""
import functools

import numpy as np

KINDS = ("normal", "tiny", "edge", "lattice")
DUPLICATES = 20            # x[:20] = y[:20] (fewer when an operand is shorter)
_U = 2.0 ** -24


def data(kind, n, m, d, seed=0):
    """x (n, d) and y (m, d) fp16, seeded; the first min(n, m, 20) rows of both are the same vectors.
    `edge` adds one pair whose difference itself overflows: the last x row is 60000, the last y row -60000."""
    rng = np.random.default_rng([KINDS.index(kind), n, m, d, seed])
    if kind == "lattice":
        x, y = (rng.integers(-3, 4, size=(r, d)).astype(np.float16) for r in (n, m))
    else:
        scale = {"normal": 1.0, "tiny": 2e-3, "edge": np.sqrt(65504.0 / (2 * d))}[kind]
        x, y = ((rng.standard_normal((r, d)) * scale).astype(np.float16) for r in (n, m))
    dup = min(n, m, DUPLICATES)
    x[:dup] = y[:dup]
    if kind == "edge" and n > dup and m > dup:
        x[-1], y[-1] = np.float16(60000), np.float16(-60000)
    return x, y


def _lowbit(v):
    return v & -v


def intervals(x, y):
    """lo16, hi16 (m, n) fp16: the bounds of f16(fp32 sum of the fp16 squares) of every pair (y[i], x[j]) over all
    orders of the additions, and `exact` (m, n) bool: the pairs whose fp32 sum is the same in every order."""
    x, y = np.asarray(x), np.asarray(y)
    assert x.dtype == np.float16 and y.dtype == np.float16 and x.shape[1] == y.shape[1] <= 4096
    d = x.shape[1]
    g = d * _U / (1 - d * _U)
    m, n = y.shape[0], x.shape[0]
    lo, hi = np.empty((m, n), np.float16), np.empty((m, n), np.float16)
    exact = np.empty((m, n), bool)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(m):
            diff = y[i][None, :] - x                                   # fp16 - fp16 -> fp16, correctly rounded
            sq = diff * diff
            bad = ~np.isfinite(sq).all(axis=1)
            t = (np.where(np.isfinite(sq), sq, 0).astype(np.float64) * 2.0 ** 24).astype(np.int64)
            s = t.sum(axis=1)
            ex = (s == 0) | (s < (_lowbit(np.bitwise_or.reduce(t, axis=1)) << 24))
            sf = s.astype(np.float64) * _U                             # exact: s < 2^53
            l = np.where(ex, sf, sf * (1 - g)).astype(np.float32).astype(np.float16)
            h = np.where(ex, sf, sf * (1 + g)).astype(np.float32).astype(np.float16)
            l[bad] = h[bad] = np.inf
            lo[i], hi[i], exact[i] = l, h, ex | bad
    return lo, hi, exact


def bits(a):
    return np.asarray(a).view(np.uint16).astype(np.int64)


def finish(s16, similarity):
    """mk_finish / the reference's last steps on the fp16 sum."""
    with np.errstate(over="ignore"):
        d16 = np.sqrt(s16.astype(np.float32)).astype(np.float16)
        if not similarity:
            return d16
        t = (np.float32(1) + d16.astype(np.float32)).astype(np.float16)
        return (np.float32(1) / t.astype(np.float32)).astype(np.float16)


def _models(lo, hi):
    assert (bits(hi) - bits(lo) >= 0).all() and (bits(hi) - bits(lo) <= 1).all()      # equal or adjacent
    out = {}
    for sim in (False, True):
        a, b = finish(lo, sim), finish(hi, sim)
        out[sim] = (a, b, bits(a) == bits(b))
    return out


def allowed(x, y, similarity):
    """(a, b, decided): the two allowed fp16 values of every pair, (m, n) each, and where they are the same."""
    lo, hi, _ = intervals(x, y)
    return _models(lo, hi)[similarity]


def inside(got, a, b):
    """Every entry of `got` is, bit for bit, one of its pair's two allowed values."""
    g = bits(got)
    return (g == bits(a)) | (g == bits(b))


@functools.lru_cache(maxsize=None)
def case(kind, n, m, d, seed=0):
    """data() and both models of it, computed once per process: x, y, {similarity: (a, b, decided)} and the
    (lo16, hi16, exact) of intervals()."""
    x, y = data(kind, n, m, d, seed)
    lo, hi, exact = intervals(x, y)
    out = _models(lo, hi)
    for v in (x, y, lo, hi, exact) + tuple(t for s in out.values() for t in s):
        v.setflags(write=False)
    return x, y, out, (lo, hi, exact)
