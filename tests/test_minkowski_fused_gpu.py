"""
GPU checks of the fused Minkowski graph kernels (pg_minkowski_knn, pg_minkowski_eps_*): they share the per-pair
arithmetic of pg_minkowski_dense, so their graphs must equal the staged path (dense block -> pg_f16_knn /
pg_f16_eps_*) BIT FOR BIT at every dimension - D = 1280 included - and through `build_graph(distance=minkowski)`
the reference's goldens as before; device-resident graphs feed the analytics and the CSR side-car.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import load_golden
from prograph_amd import synth

pytestmark = pytest.mark.gpu

CMPS = ["CMP_LE", "CMP_LT", "CMP_EQ", "CMP_GE", "CMP_GT"]


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def _emb(kind, n, d, seed):
    rng = np.random.default_rng(seed)
    if kind == "ties":          # integer values and duplicated rows: equal distances everywhere
        e = rng.integers(-2, 3, size=(n, d)).astype(np.float16)
        e[1::3] = e[0:n - 1:3][: len(e[1::3])]
    elif kind == "huge":        # squares beyond fp16's range: inf distances
        e = rng.uniform(-60000, 60000, size=(n, d)).astype(np.float16)
        e[::7] *= np.float16(0.001)
    else:
        e = rng.standard_normal((n, d)).astype(np.float16)
    return torch.from_numpy(e)


def _bits(t):
    return t.cpu().numpy().view(np.int16)


def _check_knn(nat, xp, k, first, sim, block):
    fi, fw = nat.minkowski_knn(xp, xp, k, first=first, similarity=sim)
    si, sw = nat.f16_knn(block, k, first=first, descending=sim)
    assert torch.equal(fi, si), (k, first, sim)
    assert np.array_equal(_bits(fw), _bits(sw)), (k, first, sim)


def _check_eps(nat, xp, cmp, eps, sim, block, cap=256):
    got = nat.minkowski_eps(xp, xp, cmp, eps, similarity=sim, cap=cap)
    want = nat.f16_eps(block, cmp, eps, similarity=sim)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (cmp, eps, sim, cap)
    assert np.array_equal(_bits(got[2]), _bits(want[2])), (cmp, eps, sim, cap)
    return int(got[0][-1])


def _thresholds(block):
    v = np.sort(block.float().cpu().numpy().reshape(-1))
    v = v[np.isfinite(v) & (v > 0)]
    return [float(v[int(q * (len(v) - 1))]) for q in (0.02, 0.5)] if len(v) else [1.0]


@pytest.mark.parametrize("sim", [False, True])
@pytest.mark.parametrize("n", [1, 5, 257, 1000, 4099])
@pytest.mark.parametrize("d", [2, 8, 13, 64, 1280])
def test_fused_equals_staged(nat, d, n, sim):
    x = _emb("normal", n, d, seed=d * 7919 + n).to(nat.device())
    xp = nat.pack_f16(x)
    block = nat.minkowski_dense(xp, xp, similarity=sim)
    for k in (1, 5, 16, 63):
        for first in (0, 1):
            if first + k <= 64:
                _check_knn(nat, xp, k, first, sim, block)
    for eps in _thresholds(block):
        for c in CMPS:
            _check_eps(nat, xp, getattr(nat, c), eps, sim, block)


@pytest.mark.parametrize("kind", ["ties", "huge"])
@pytest.mark.parametrize("d", [8, 13, 64, 1280])
def test_fused_equals_staged_on_ties_and_overflow(nat, kind, d):
    n = 1000
    x = _emb(kind, n, d, seed=d + (1 if kind == "ties" else 2)).to(nat.device())
    xp = nat.pack_f16(x)
    for sim in (False, True):
        block = nat.minkowski_dense(xp, xp, similarity=sim)
        if kind == "huge":
            assert torch.isinf(nat.minkowski_dense(xp, xp)).any()
        for k, first in ((1, 0), (5, 1), (16, 1), (63, 1), (63, 0)):
            _check_knn(nat, xp, k, first, sim, block)
        vals = block.float().cpu().numpy().reshape(-1)
        for eps in [float(np.median(vals[np.isfinite(vals)]))] + ([float(np.inf)] if kind == "huge" and not sim else []):
            for c in CMPS:
                _check_eps(nat, xp, getattr(nat, c), eps, sim, block)


def test_eps_rows_beyond_the_slot_capacity(nat):
    """A dense cluster with cap = 4: most rows outgrow their slot and take the restricted second sweep."""
    rng = np.random.default_rng(5)
    for d in (13, 64, 1280):
        e = np.concatenate([rng.normal(0, 0.01, (300, d)), rng.normal(5, 1, (700, d))]).astype(np.float16)
        xp = nat.pack_f16(torch.from_numpy(e).to(nat.device()))
        for sim in (False, True):
            block = nat.minkowski_dense(xp, xp, similarity=sim)
            eps = float(np.float16(1 / (1 + 0.5 * np.sqrt(d)))) if sim else float(0.5 * np.sqrt(d))
            counts = torch.diff(nat.f16_eps(block, nat.CMP_LE if not sim else nat.CMP_GE, eps, similarity=sim)[0])
            cmp = nat.CMP_LE if not sim else nat.CMP_GE
            assert int((counts > 4).sum()) >= 250                  # the overflow sweep does run
            for cap in (4, 256, 1):
                _check_eps(nat, xp, cmp, eps, sim, block, cap=cap)


def _prograph(tmp_path, n, name, seed=3):
    from prograph_amd import Prograph
    tok = synth.clustered_tokens(n, 8, seed=seed)
    f = tmp_path / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(seed).uniform(0, 1, n)}).to_csv(f)
    return Prograph(file=str(f))


def test_goldens_through_device_graphs(nat, tmp_path, capsys):
    """tests/golden/minkowski_f16.npz (outputs of the reference) through build_graph(..., output="csr"), with the
    assertions of test_minkowski_f16_against_the_reference."""
    from prograph_amd.distance import minkowski
    from prograph_amd.graph import CSRGraph, KNNGraph
    g = load_golden("minkowski_f16")
    for name in ("d2", "d64", "d1280"):
        emb = g[f"{name}_emb"]
        pg = _prograph(tmp_path, emb.shape[0], name)
        capsys.readouterr()
        pg.graph["Embedded"] = list(emb)
        tol = 1 if name == "d1280" else 0
        for k in (1, 5, 16):
            G = pg.build_graph(representation="Embedded", k=k, distance=minkowski, output="csr")
            assert isinstance(G, KNNGraph) and G.dist.dtype == torch.float16
            idx, w = G.idx.cpu().numpy(), G.dist.cpu().numpy()
            wulp = np.abs(w.view(np.int16).astype(np.int64) - g[f"{name}_knn{k}_w"].view(np.int16).astype(np.int64))
            assert wulp.max() <= tol
            same = (idx == g[f"{name}_knn{k}_idx"]).all(1)
            assert same.mean() >= (0.98 if name == "d1280" else 1.0), (name, k, float(same.mean()))
        G = pg.build_graph(representation="Embedded", k=4, similarity=True, distance=minkowski, output="csr")
        same = (G.idx.cpu().numpy() == g[f"{name}_knn4_sim_idx"]).all(1)
        assert same.mean() >= (0.98 if name == "d1280" else 1.0)
        if name != "d1280":
            assert np.array_equal(G.dist.cpu().numpy(), g[f"{name}_knn4_sim_w"])
        eps = float(g[f"{name}_eps"])
        for sim, key in ((False, "eps"), (True, "eps_sim")):
            E = pg.build_graph(representation="Embedded", eps=eps, similarity=sim, distance=minkowski, output="csr")
            assert isinstance(E, CSRGraph) and E.weights.dtype == torch.float16
            ip, ix, w = E.host()
            if name == "d1280":
                assert abs(int(ip[-1]) - int(g[f"{name}_{key}_indptr"][-1])) <= 0.002 * int(ip[-1]) + 2
            else:
                assert np.array_equal(ip, g[f"{name}_{key}_indptr"]) and np.array_equal(ix, g[f"{name}_{key}_indices"])
                assert np.array_equal(w.astype(np.float64), g[f"{name}_{key}_weights"].astype(np.float64))


def _staged_blocks(nat, xp, x, fn, rows=4096):
    out = []
    for r0 in range(0, x.shape[0], rows):
        out.append(fn(nat.minkowski_dense(xp, nat.pack_f16(x[r0:r0 + rows]))))
    return out


def test_full_size_fused_equals_staged(nat):
    """N = 50 000, D = 64 (the mink64 shape): kNN k = 16 and eps at ~16 neighbours per row, every entry."""
    rng = np.random.default_rng(64)
    n, d = 50_000, 64
    centers = rng.normal(0, 1, (2000, d))
    e = (centers[rng.integers(0, 2000, n)] + rng.normal(0, 0.15, (n, d))).astype(np.float16)
    x = torch.from_numpy(e).to(nat.device())
    xp = nat.pack_f16(x)
    fi, fw = nat.minkowski_knn(xp, xp, 16, first=1)
    parts = _staged_blocks(nat, xp, x, lambda b: nat.f16_knn(b, 16, first=1))
    assert torch.equal(fi, torch.cat([p[0] for p in parts]))
    assert np.array_equal(_bits(fw), _bits(torch.cat([p[1] for p in parts])))
    eps = float(fw[:, 15].float().median())                             # ~16 neighbours per row
    got = nat.minkowski_eps(xp, xp, nat.CMP_LE, eps)
    parts = _staged_blocks(nat, xp, x, lambda b: nat.f16_eps(b, nat.CMP_LE, eps))
    base, ptrs = 0, [torch.zeros(1, dtype=torch.int64, device=x.device)]
    for p in parts:
        ptrs.append(p[0][1:] + base)
        base += int(p[0][-1])
    assert torch.equal(got[0], torch.cat(ptrs))
    assert torch.equal(got[1], torch.cat([p[1] for p in parts]))
    assert np.array_equal(_bits(got[2]), _bits(torch.cat([p[2] for p in parts])))
    assert 8 * n <= base <= 40 * n, base


def _row_bound(pg, graph, boolean):
    """|deg_device - deg_column| per row: float32 summation error of the column path."""
    col = pg.graph[graph]
    nnz = np.array([len(c[0]) for c in col], dtype=np.float64)
    s = np.array([np.abs(np.asarray(c[1], dtype=np.float64)).sum() for c in col])
    return nnz * 2.0 ** -24 * (nnz if boolean else s) + 1e-300


@pytest.mark.parametrize("kind", ["knn", "eps"])
def test_device_analytics_match_the_column_path(nat, tmp_path, capsys, kind):
    from prograph_amd.distance import minkowski
    from prograph_amd.utils import save
    n, d = 2000, 16
    pg = _prograph(tmp_path, n, "an", seed=11)
    capsys.readouterr()
    rng = np.random.default_rng(12)
    centers = rng.normal(0, 1, (100, d))
    pg.graph["Embedded"] = list((centers[rng.integers(0, 100, n)] + rng.normal(0, 0.3, (n, d))).astype(np.float32))
    args = dict(k=10) if kind == "knn" else dict(eps=1.6)
    tuples = pg.build_graph(representation="Embedded", distance=minkowski, store="E", **args)
    assert pg._device_graph("E") is not None and pg.csr_graphs["E"] is not None
    again = pg.build_graph(representation="Embedded", distance=minkowski, **args)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int16), b[1].view(np.int16)) and
               a[1].dtype == b[1].dtype and a[0].dtype == b[0].dtype for a, b in zip(tuples, again))
    if kind == "eps":
        assert min(len(t[0]) for t in tuples) == 0 and max(len(t[0]) for t in tuples) > 0
    pg.graph["T"] = list(tuples)
    assert pg._device_graph("T") is None
    assert np.array_equal(pg.degree("E", boolean_weights=True), pg.degree("T", boolean_weights=True))
    dw, cw = pg.degree("E").astype(np.float64), pg.degree("T").astype(np.float64)
    assert np.all(np.abs(dw - cw) <= _row_bound(pg, "T", False)), float(np.abs(dw - cw).max())
    for b in (False, True):
        for mode in ("outdegree", "indegree"):
            ld, lc = pg.laplacian("E", boolean_weights=b, mode=mode).diagonal(), pg.laplacian("T", boolean_weights=b, mode=mode).diagonal()
            assert np.all(np.abs(ld - lc) <= _row_bound(pg, "T", b) * (50 if mode == "indegree" else 1)), (b, mode)
            de, dc = pg.dirichlet("E", boolean_weights=b, mode=mode), pg.dirichlet("T", boolean_weights=b, mode=mode)
            assert np.allclose(de, dc, rtol=1e-6, atol=0), (b, mode, de, dc)
    ve, vc = pg.local_variance("E"), pg.local_variance("T")
    assert np.array_equal(np.isnan(ve), np.isnan(vc))
    ok = ~np.isnan(vc)
    assert np.allclose(ve[ok], vc[ok], rtol=1e-12, atol=1e-14)
    # persistence: the device graph goes to the side-car and comes back with identical arrays
    from prograph_amd import Prograph
    assert save(pg, name="mk", directory=str(tmp_path) + "/", graphs="csr")
    back = Prograph(file=str(tmp_path / "mk.pkl"))
    capsys.readouterr()
    g0, g1 = pg.csr_graphs["E"], back.csr_graphs["E"]
    assert type(g0) is type(g1) and g0.similarity == g1.similarity and g0.ncols == g1.ncols
    for a in (("idx", "dist") if kind == "knn" else ("indptr", "indices", "weights")):
        t0, t1 = getattr(g0, a), getattr(g1, a)
        assert t0.dtype == t1.dtype and torch.equal(t0.cpu().view(torch.int16) if t0.dtype == torch.float16 else t0.cpu(),
                                                    t1.cpu().view(torch.int16) if t1.dtype == torch.float16 else t1.cpu())
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].dtype == b[1].dtype
               for a, b in zip(back.graph["E"], pg.graph["E"]))
    assert back._device_graph("E") is not None
    assert np.array_equal(back.degree("E"), pg.degree("E"))
