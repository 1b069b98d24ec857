"""
The cosine and Euclidean kernels (prograph_amd/csrc/pg_cos.hip) against the exact model of tests/exact_sums_model.py, bit
for bit: on inputs whose sums p, nx, ny are exact in fp32 in any accumulation order, DESIGN.md §4.9 / §4.24 determine
every output bit - the norms and reciprocal roots of `pg_cosine_prep`, every entry of the dense blocks as distances and
as similarities, and with them the (value, column) order the fused kNN and eps kernels select in.  No comparison here
has a tolerance; tests/test_exact_sums_model_cpu.py shows on the same case lists that a swapped multiply order or a
contracted `1 - c` in the epilogue changes entries compared here.
"""
import numpy as np
import pytest
import torch

import exact_sums_model as em

pytestmark = pytest.mark.gpu

METRICS = ("cosine", "euclidean")
CMPS = ("CMP_LE", "CMP_LT", "CMP_EQ", "CMP_GE", "CMP_GT")


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def _bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t).view(np.uint32)


def _same(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    if len(bad):
        at = tuple(bad[0])
        have = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
        pytest.fail(f"{what}: {len(bad)} of {g.size} entries differ, the first at {list(map(int, at))}: {have[at]!r} for {want[at]!r}")


def _prep(nat, op):
    """The device operand of a model Operand, its norms and reciprocal roots checked against the model first: a
    departure of nx or ny shows here, before any block is compared."""
    c = nat.cosine_prep(torch.from_numpy(op.values()).to(nat.device()))
    assert not c.nonfinite()
    n, r = em.norms(op)
    _same(c.norms[:op.n], n, "norms")
    _same(c.rnorms[:op.n], r, "rnorms")
    zero = ~op.ints.any(1)
    assert (c.norms[:op.n].cpu().numpy()[zero] == 0).all()
    return c


def _check_blocks(nat, case):
    x, y = em.make_case(*case)
    xc, yc = _prep(nat, x), _prep(nat, y)
    for metric in METRICS:
        dense = getattr(nat, metric + "_dense")
        for a, ac, tag in ((x, xc, "X-X"), (y, yc, "Y-X")):
            for sim in (False, True):
                got = dense(xc, ac, similarity=sim)
                assert got.dtype == torch.float32 and got.shape == (a.n, x.n)
                _same(got, em.BLOCKS[metric](x, a, similarity=sim), (case, metric, tag, "similarity" if sim else "distance"))
    return x, y, xc, yc


@pytest.mark.parametrize("kind", em.EXPONENT_SETS)
def test_every_dimension_to_144(nat, kind):
    """D = 1 .. 144 at N = 70, M = 40: every remainder of the unrolled loop over chunk pairs, every odd chunk count."""
    for case in em.dimension_cases(em.DIMS_SMALL, 70, 40):
        if case[3] == kind:
            _check_blocks(nat, case)


@pytest.mark.parametrize("case", em.dimension_cases(em.DIMS_LARGE, 300, 77), ids=lambda c: f"{c[0]}-{c[3]}")
def test_dimensions_around_1280(nat, case):
    _check_blocks(nat, case)


def _check_knn(nat, metric, xc, yc, block, k, first, sim, what):
    idx, w = getattr(nat, metric + "_knn")(xc, yc, k, first=first, similarity=sim)
    wi, ww = em.knn(block, k, first, sim)
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), wi), (what, k, first, sim)
    _same(w, ww, (what, k, first, sim))


@pytest.mark.parametrize("d", em.EDGE_D)
def test_shapes_at_the_tile_and_workgroup_edges(nat, d):
    """N in {1, 2, 31, 32, 33, 257} against M in {1, 31, 33, 129}: the blocks, and kNN lists with first + k up to 64 on
    rows that are shorter than that (missing ranks: idx -1, weight 0)."""
    for case in em.edge_cases():
        if case[0] != d:
            continue
        x, y, xc, yc = _check_blocks(nat, case)
        for metric in METRICS:
            for sim in (False, True):
                block = em.BLOCKS[metric](x, y, similarity=sim)
                for k, first in ((64, 0), (63, 1), (16, 0), (1, 1)):
                    _check_knn(nat, metric, xc, yc, block, k, first, sim, (case, metric))


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("metric", METRICS)
def test_selection_on_tie_saturated_data(nat, metric, d):
    """Points of the grid {0..7}^d, N = 600: most values occur many times and many points coincide, so the lists and
    the CSR rows are decided by the column order.  kNN (k > 63: the round kernel) and eps graphs under every comparator,
    with and without keep_zero, slots of 256, 4 and 1 entries, against a stable sort / nonzero of the MODEL's block."""
    x, y = em.grid_case(d)
    xc, yc = _prep(nat, x), _prep(nat, y)
    eps_fn = getattr(nat, metric + "_eps")
    for a, ac, tag in ((x, xc, "X-X"), (y, yc, "Y-X")):
        for sim in (False, True):
            block = em.BLOCKS[metric](x, a, similarity=sim)
            _same(getattr(nat, metric + "_dense")(xc, ac, similarity=sim), block, (metric, d, tag, sim))
            assert len(np.unique(block)) < block.size // 4                        # ties in every row
            for k in (1, 16, 63, 64, 130):
                for first in (0, 1):
                    _check_knn(nat, metric, xc, ac, block, k, first, sim, (metric, d, tag))
            for eps in em.thresholds(block, sim):
                for c, cmp in enumerate(CMPS):
                    for keep_zero in (False, True):
                        want = em.eps_csr(block, c, eps, sim, keep_zero)
                        assert getattr(nat, cmp) == c and (c != 2 or want[0][-1] > 0)      # == has hits
                        for cap in (256, 4, 1):
                            ip, ix, w = eps_fn(xc, ac, c, eps, similarity=sim, cap=cap, keep_zero=keep_zero)
                            what = (metric, d, tag, sim, cmp, eps, keep_zero, cap)
                            assert np.array_equal(ip.cpu().numpy(), want[0]), what
                            assert ix.dtype == torch.int32 and np.array_equal(ix.cpu().numpy(), want[1]), what
                            _same(w, want[2], what)


def test_fp16_subnormal_elements(nat):
    """The same family with exponents -24 .. -20, where elements are fp16 subnormals: kept apart, because what the
    matrix cores do with subnormal A / B operands is a property of the hardware the contract has to state."""
    for d in em.SUBNORMAL_DIMS:
        case = (d, 70, 40, "subnormal")
        x, y = em.make_case(*case)
        assert x.has_fp16_subnormals() and y.has_fp16_subnormals()
        _check_blocks(nat, case)
