"""
The exact cosine / Euclidean model (tests/exact_sums_model.py) checked without a GPU: its roots and reciprocals are the
nearest float32 to the exact value (integer / `fractions` arithmetic), a few hundred pairs are recomputed step by step
with Python integers and `Fraction` under an explicit round-to-nearest-even, the planted rows give the exact values the
contract names, and the two mutants the loose bound of tests/test_cosine_gpu.py lets through - the swapped multiply order
and the fused `1 - c` - differ from the model in every dimension case of tests/test_cosine_exact_gpu.py and in each of its
other case lists, so that test sees them.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_sums_model as em

F32 = np.float32
NEAR_TWO = F32(2 - 3 * 2.0 ** -23)


# ---------------------------------------------------------------- float32 arithmetic on Fractions
def _exponent(v, base):
    """e with base^e <= v < base^(e + 1), v a positive Fraction."""
    e = (v.numerator.bit_length() - v.denominator.bit_length()) // (1 if base == 2 else 2)
    while Fraction(base) ** e > v:
        e -= 1
    while Fraction(base) ** (e + 1) <= v:
        e += 1
    return e


def rnd(v):
    """The float32 nearest to the Fraction v, ties to even, as a Fraction (normal range only)."""
    if v == 0:
        return Fraction(0)
    sign, v = (-1 if v < 0 else 1), abs(v)
    e = _exponent(v, 2)
    assert -126 <= e <= 127, "outside the normal float32 range"
    ulp = Fraction(2) ** (e - 23)
    q = v / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return sign * n * ulp


def rnd_sqrt(v):
    """The float32 nearest to sqrt(v) for a Fraction v >= 0, by integer square roots."""
    if v == 0:
        return Fraction(0)
    e = _exponent(v, 4)                                   # 2^e <= sqrt(v) < 2^(e + 1)
    ulp = Fraction(2) ** (e - 23)
    q = v / (ulp * ulp)
    t = math.isqrt(q.numerator // q.denominator)          # floor(sqrt(v) / ulp)
    assert 2 ** 23 <= t < 2 ** 24
    if Fraction(2 * t + 1) ** 2 < 4 * q:                  # sqrt(v) / ulp above t + 1/2 (a tie cannot occur)
        t += 1
    return t * ulp


def fr(x):
    return Fraction(float(x))


def scalar_pair(xv, yv):
    """(cosine d, Euclidean d) of two vectors of Fractions, every step of cs_finish / eu_finish rounded by rnd."""
    p, nx, ny = sum(a * b for a, b in zip(xv, yv)), sum(a * a for a in xv), sum(b * b for b in yv)
    assert rnd(p) == p and rnd(nx) == nx and rnd(ny) == ny           # the family: exact in fp32
    same = p == nx == ny
    if nx == 0 or ny == 0:
        dc = Fraction(1)
    elif same:
        dc = Fraction(0)
    else:
        rx, ry = rnd(1 / rnd_sqrt(nx)), rnd(1 / rnd_sqrt(ny))
        c = rnd(rnd(p * ry) * rx)
        dc = min(max(rnd(1 - c), Fraction(0)), Fraction(2))
    de = Fraction(0) if same else rnd_sqrt(max(rnd(rnd(nx + ny) - rnd(p + p)), Fraction(0)))
    return dc, de


def test_the_rounding_helpers_on_known_values():
    assert rnd(Fraction(1, 3)) == fr(F32(1) / F32(3)) and rnd(Fraction(2 ** 24 + 1)) == 2 ** 24
    assert rnd(Fraction(2 ** 24 + 3)) == 2 ** 24 + 4 and rnd(Fraction(-5, 2 ** 30)) == Fraction(-5, 2 ** 30)
    assert rnd_sqrt(Fraction(2)) == fr(F32(np.sqrt(2.0))) and rnd_sqrt(Fraction(9, 4)) == Fraction(3, 2)
    assert rnd_sqrt(Fraction(2 ** 24 - 1)) == fr(np.sqrt(np.float64(2 ** 24 - 1)).astype(F32))


SAMPLE = [(d, 70, 40, kind) for d in (1, 2, 3, 7, 8, 9, 17, 64, 100, 144) for kind in em.EXPONENT_SETS + ("subnormal",)]


def test_roots_and_reciprocals_are_the_nearest_float32():
    seen = 0
    for case in SAMPLE + [(1281, 300, 77, "mixed")]:
        for op in em.make_case(*case):
            n, r = em.norms(op)
            exact = (op.ints.astype(object) ** 2).sum(1)
            for i in range(op.n):
                v = Fraction(int(exact[i])) * Fraction(2) ** int(2 * op.exps[i])
                assert fr(n[i]) == v                                  # the norm itself is exact
                if v == 0:
                    assert np.isinf(r[i]) and r[i] > 0
                    continue
                assert fr(r[i]) == rnd(1 / rnd_sqrt(v)), (case, i)
                seen += 1
    assert seen > 4000


def test_pairs_against_fraction_arithmetic():
    rng = np.random.default_rng(3)
    seen = extremes = 0
    for case in SAMPLE:
        x, y = em.make_case(*case)
        blocks = [(em.cosine_block(x, y), em.euclidean_block(x, y), x, y), (em.cosine_block(x, x), em.euclidean_block(x, x), x, x)]
        for cb, eb, a, b in blocks:
            rows = np.concatenate([rng.integers(0, b.n, 4), [3, 4, 7, 12]])      # random pairs and the planted rows
            cols = np.concatenate([rng.integers(0, a.n, 4), [33, 4, 20, 6]])
            for i, j in zip(rows, cols):
                xv = [Fraction(int(t)) * Fraction(2) ** int(a.exps[j]) for t in a.ints[j]]
                yv = [Fraction(int(t)) * Fraction(2) ** int(b.exps[i]) for t in b.ints[i]]
                dc, de = scalar_pair(xv, yv)
                assert fr(cb[i, j]) == dc and fr(eb[i, j]) == de, (case, i, j)
                extremes += dc in (0, 1, 2)
                seen += 1
        sc, se = em.cosine_block(x, y, similarity=True), em.euclidean_block(x, y, similarity=True)
        for i, j in zip(rng.integers(0, y.n, 3), rng.integers(0, x.n, 3)):
            assert fr(sc[i, j]) == rnd(1 / rnd(1 + fr(blocks[0][0][i, j])))
            assert fr(se[i, j]) == rnd(1 / rnd(1 + fr(blocks[0][1][i, j])))
    assert seen >= 300 and extremes >= 40


@pytest.mark.parametrize("kind", em.EXPONENT_SETS)
def test_planted_rows_give_the_values_the_contract_names(kind):
    for d in (1, 9, 64, 144):
        x, y = em.make_case(d, 70, 40, kind)
        c, e = em.cosine_block(x, x), em.euclidean_block(x, x)
        live = np.arange(70) != 20
        assert (np.diag(c)[live] == 0).all() and (np.diag(e) == 0).all()
        for i, j in ((2, 5), (31, 32), (10, 69)):
            assert c[i, j] == 0 and c[j, i] == 0 and e[i, j] == 0
        assert (c[20] == 1).all() and (c[:, 20] == 1).all() and c[20, 20] == 1 and e[20, 20] == 0
        # opposite vectors: c = -(n * r) * r, and r = 1/sqrt(n) carries two roundings, each product one more, so |c| is
        # within 6 * 2^-24 of 1 and d = 1 - c lies in [2 - 3 * 2^-23, 2] (the clamp holds the upper end): 2 up to rounding,
        # not always 2 itself, and the same for both orders
        assert NEAR_TWO <= c[40, 41] <= 2 and c[41, 40] == c[40, 41]
        c, e = em.cosine_block(x, y), em.euclidean_block(x, y)
        assert c[3, 33] == 0 and e[3, 33] == 0 and c[4, 4] == 0 and NEAR_TWO <= c[12, 6] <= 2
        assert (c[7] == 1).all() and (c[:, 20] == 1).all() and e[7, 20] == 0
        n, _ = em.norms(x)
        assert np.array_equal(e[7], np.sqrt(n.astype(np.float64)).astype(F32))   # d(0, x) = sqrt(nx)
        assert c.dtype == F32 and e.dtype == F32 and c.min() >= 0 and c.max() <= 2


def test_the_generator_refuses_what_is_outside_the_family():
    with pytest.raises(AssertionError):
        em.Operand([[4096, 1]], [0])                                         # D * A^2 >= 2^24
    with pytest.raises(AssertionError):
        em.Operand([[2049]], [0]).values()                                   # 12 significant bits
    with pytest.raises(AssertionError):
        em.Operand([[3]], [-25]).values()                                    # below the smallest fp16 subnormal
    with pytest.raises(AssertionError):
        em.Operand([[2047]], [6]).values()                                   # above 65504
    assert em.amplitude(1) == 2047 and em.amplitude(4) == 2047 and em.amplitude(5) == 1831 and em.amplitude(1280) == 114
    for d in em.DIMS_SMALL + em.DIMS_LARGE:
        a = em.amplitude(d)
        assert d * a * a < 2 ** 24 and (a == 2047 or d * (a + 1) ** 2 >= 2 ** 24)
    for d in em.SUBNORMAL_DIMS:
        x, y = em.make_case(d, 70, 40, "subnormal")
        assert x.has_fp16_subnormals() and y.has_fp16_subnormals() and x.exps.min() >= -24
        x.values(), y.values()
    assert not em.make_case(9, 70, 40, "low")[0].has_fp16_subnormals()


def _differs(case, variant, grid=False):
    x, y = em.grid_case(case) if grid else em.make_case(*case)
    return sum(int((em.cosine_block(x, b, variant=variant).view(np.uint32) != em.cosine_block(x, b).view(np.uint32)).sum())
               for b in (x, y))


@pytest.mark.parametrize("variant", ["swapped", "fused"])
def test_the_mutants_differ_in_every_case_of_the_gpu_test(variant):
    """Per case of the dimension lists (the X-X and the Y-X block together), and in the edge-shape and the grid lists."""
    counts = {c: _differs(c, variant) for c in em.dimension_cases(em.DIMS_SMALL, 70, 40) + em.dimension_cases(em.DIMS_LARGE, 300, 77)}
    missed = [c for c, k in counts.items() if k == 0]
    print(variant, "entries changed per case: min", min(counts.values()), "max", max(counts.values()))
    assert not missed, missed
    assert sum(_differs(c, variant) for c in em.edge_cases()) > 0
    assert all(_differs(d, variant, grid=True) > 0 for d in (2, 3))
    assert all(_differs((d, 70, 40, "subnormal"), variant) > 0 for d in em.SUBNORMAL_DIMS)


def test_selection_helpers_on_a_hand_made_block():
    b = np.array([[0.5, 0.0, 0.5, 2.0], [1.0, 1.0, 0.25, 0.25]], dtype=F32)
    idx, w = em.knn(b, 3, 1)
    assert idx.tolist() == [[0, 2, 3], [3, 0, 1]] and w.tolist() == [[0.5, 0.5, 2.0], [0.25, 1.0, 1.0]]
    idx, w = em.knn(b, 3, 2, similarity=True)
    assert idx.tolist() == [[2, 1, -1], [2, 3, -1]] and w.tolist() == [[0.5, 0.0, 0.0], [0.25, 0.25, 0.0]]
    ip, ix, w = em.eps_csr(b, 0, 0.5)
    assert ip.tolist() == [0, 2, 4] and ix.tolist() == [0, 2, 2, 3] and w.tolist() == [0.5, 0.5, 0.25, 0.25]
    ip, ix, w = em.eps_csr(b, 0, 0.5, keep_zero=True)
    assert ip.tolist() == [0, 3, 5] and ix.tolist() == [0, 1, 2, 2, 3]
    ip, ix, w = em.eps_csr(b, 4, 0.5, similarity=True)                        # eps > s and s < 1
    assert ip.tolist() == [0, 1, 3] and ix.tolist() == [1, 2, 3]
    ip, ix, w = em.eps_csr(b, 2, 0.25)
    assert ix.tolist() == [2, 3] and ix.dtype == np.int32 and ip.dtype == np.int64 and w.dtype == F32
