"""
The interval model of tests/minkowski_model.py against what it has to contain, without a device: the real
reference's distances (tests/golden/minkowski_f16.npz) and the project's own torch expression on CPU fp16
tensors - two fp32 accumulation orders that are not the kernel's.  Then the conditions on the seeded data that
tests/test_minkowski_values_gpu.py relies on, asserted so that no choice of data can hide a failure.

Decided shares (pairs whose two allowed values are the same, so the comparison is bit for bit), 33 x 300 pairs:

    goldens d2 / d64 / d1280 (64 x N pairs)      1.000 / 0.9945 / 0.8727      asserted: >= 0.85, inside for all pairs
    lattice, tiny                                1.000 at every D             asserted: all pairs
    normal                                       >= 0.989 for D <= 136, 0.918 at D = 1000, 0.873 at D = 1280
    edge                                         >= 0.990 for D <= 136, 0.938 at D = 1000, 0.931 at D = 1280
                                                                              asserted: >= 0.85 for D <= 1280
    normal / edge at D = 2049                    0.816 / 0.884                (no share asserted beyond 1280)
"""
import numpy as np
import pytest
import torch

import minkowski_model as mm
from conftest import load_golden
from prograph_amd.distance import minkowski

M, N = 33, 300
DIMS = (1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 255, 257, 1000, 1280, 2049)     # the GPU file's


@pytest.mark.parametrize("name,share", [("d2", 1.0), ("d64", 0.99), ("d1280", 0.85)])
def test_model_contains_the_reference(name, share):
    g = load_golden("minkowski_f16")
    e, want = g[f"{name}_emb"], g[f"{name}_dist64"]
    a, b, decided = mm.allowed(e, e[:64], False)
    assert want.dtype == np.float16 and want.shape == a.shape
    ok = mm.inside(want, a, b)
    print(f"{name}: inside {ok.mean():.4f}, decided {decided.mean():.4f}")
    assert ok.all(), (name, int((~ok).sum()))
    assert np.array_equal(mm.bits(want)[decided], mm.bits(a)[decided])
    assert decided.mean() >= share, (name, float(decided.mean()))


@pytest.mark.parametrize("d", [1, 2, 7, 9, 129, 1000, 1280])
@pytest.mark.parametrize("kind", mm.KINDS)
def test_model_contains_the_torch_expression(kind, d):
    """minkowski() on CPU fp16 tensors takes the reference's torch expression: torch's own accumulation order."""
    x, y, models, _ = mm.case(kind, N, M, d)
    for sim in (False, True):
        got = minkowski(torch.from_numpy(x.copy()), torch.from_numpy(y.copy()), similarity=sim)
        assert got.dtype == torch.float16 and tuple(got.shape) == (M, N)
        a, b, decided = models[sim]
        ok = mm.inside(got.numpy(), a, b)
        assert ok.all(), (kind, d, sim, int((~ok).sum()))


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("kind", mm.KINDS)
def test_conditions_on_the_data(kind, d):
    x, y, models, (lo, hi, exact) = mm.case(kind, N, M, d)
    assert ((mm.bits(hi) - mm.bits(lo)) >= 0).all() and ((mm.bits(hi) - mm.bits(lo)) <= 1).all()
    assert np.array_equal(x[:mm.DUPLICATES], y[:mm.DUPLICATES])
    dist, sim = models[False], models[True]
    dup = np.arange(mm.DUPLICATES)
    assert (dist[0][dup, dup] == 0).all() and (dist[1][dup, dup] == 0).all()
    assert (sim[0][dup, dup] == 1).all() and (sim[1][dup, dup] == 1).all()
    shares = (float(dist[2].mean()), float(sim[2].mean()))
    print(f"{kind} D={d}: decided {shares[0]:.4f} (distance) {shares[1]:.4f} (similarity)")
    if kind in ("lattice", "tiny"):
        assert exact.all() and shares == (1.0, 1.0)
    elif d <= 1280:
        assert min(shares) >= 0.85, shares
    over = np.isinf(dist[0]) & np.isinf(dist[1])
    if kind == "edge":
        assert over[-1, -1] and 0.3 <= over.mean() <= 0.7                        # the sums straddle 65504 | inf
        assert (sim[0][over] == 0).all() and (sim[1][over] == 0).all()
        assert x[-1, 0] == 60000 and y[-1, 0] == -60000 and lo[-1, -1] == np.inf     # the difference itself overflows
    else:
        assert not over.any()
    if kind == "tiny":                                                           # squares that are fp16 subnormals
        sq = (y[:, None, :] - x[None, :, :]) ** 2 if d <= 136 else (y[:4, None, :] - x[None, :, :]) ** 2
        assert ((sq > 0) & (sq < np.float16(2.0 ** -14))).mean() >= 0.8 and (sq < np.float16(2.0 ** -14)).mean() >= 0.99
