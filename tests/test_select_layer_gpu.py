"""
GPU check of the row-block path of `_native._slots_eps` (minkowski_eps / cosine_eps): the CSR built from several blocks
of query rows equals the CSR of one block bit for bit.  The default block holds (256 MB) / (cap * bytes per slot) rows,
which no other test reaches; `rows_per_block=64` cuts m = 130 query rows into 64 + 64 + 2: a boundary inside the
Minkowski kernel's 16-row groups' count (4 groups), on the cosine kernel's 32-row waves, and a last block smaller than
either.  cap = 4 sends most rows of every block through the fill_rows sweep.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M, N, D, CAP = 130, 257, 13, 4


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


@pytest.fixture(scope="module")
def data(nat):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, D)).astype(np.float16)
    y = rng.standard_normal((M, D)).astype(np.float16)
    y[-2:] *= np.float16(0.25)                              # the two rows of the last block: near the centre, many matches
    x[:20] = y[5:25]                                        # dataset rows equal to a query: d = 0 / s = 1 pairs
    x, y = torch.from_numpy(x).to(nat.device()), torch.from_numpy(y).to(nat.device())
    return {"minkowski": (nat.pack_f16(x), nat.pack_f16(y)), "cosine": (nat.cosine_prep(x), nat.cosine_prep(y))}


def _bits(t):
    return t.cpu().numpy().view(np.int16 if t.dtype == torch.float16 else np.int32)


def _same(got, want, what):
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int32 and got[2].dtype == want[2].dtype, what
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what
    assert np.array_equal(_bits(got[2]), _bits(want[2])), what


@pytest.mark.parametrize("keep_zero", [False, True])
@pytest.mark.parametrize("sim", [False, True])
@pytest.mark.parametrize("metric", ["minkowski", "cosine"])
def test_row_blocks_equal_one_block(nat, data, metric, sim, keep_zero):
    xo, yo = data[metric]
    dense, eps_fn = ((nat.minkowski_dense, nat.minkowski_eps) if metric == "minkowski" else (nat.cosine_dense, nat.cosine_eps))
    block = dense(xo, yo, similarity=sim)
    # `le` keeps d <= eps, as a similarity eps <= s: the quarter of the pairs nearest to their query
    eps = float(np.quantile(block.float().cpu().numpy(), 0.75 if sim else 0.25))
    one = eps_fn(xo, yo, nat.CMP_LE, eps, similarity=sim, cap=CAP, keep_zero=keep_zero)
    counts = torch.diff(one[0]).cpu().numpy()
    assert one[0].numel() == M + 1 and 0.2 * M * N < counts.sum() < 0.3 * M * N
    assert (counts > CAP).sum() > M // 2 and all((counts[r0:r0 + 64] > CAP).any() for r0 in (0, 64, 128))
    zeros = int(((block == 1) if sim else (block == 0)).sum())
    assert zeros >= 20                                                 # keep_zero decides about these pairs
    if keep_zero:
        without = eps_fn(xo, yo, nat.CMP_LE, eps, similarity=sim, cap=CAP)
        assert int(one[0][-1]) == int(without[0][-1]) + zeros
    _same(eps_fn(xo, yo, nat.CMP_LE, eps, similarity=sim, cap=CAP, keep_zero=keep_zero, rows_per_block=64), one,
          (metric, sim, keep_zero))
    if metric == "minkowski":                                          # and both are the selection over the dense block
        _same(one, nat.f16_eps(block, nat.CMP_LE, eps, similarity=sim, keep_zero=keep_zero), ("staged", sim, keep_zero))
