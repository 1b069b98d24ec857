"""
GPU checks of the cosine kernels (pg_cosine_prep / _dense / _knn / _eps_*, prograph_amd/csrc/pg_cos.hip): the fused
graphs equal the selection over the dense block bit for bit (shared tile routine and epilogue), the values are within
the stated bound of fp64, identical vectors are exactly 0 wherever they sit in a tile, non-finite inputs take the
torch expression, and `build_graph(distance=cosine)` feeds the device analytics and the CSR side-car.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from prograph_amd import synth

pytestmark = pytest.mark.gpu

CMPS = ["CMP_LE", "CMP_LT", "CMP_EQ", "CMP_GE", "CMP_GT"]
DIMS = [1, 7, 8, 9, 15, 16, 17, 64, 100, 1280]


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def _emb(n, d, seed, kind="normal"):
    rng = np.random.default_rng(seed)
    if kind == "clustered":
        centers = rng.normal(0, 1, (max(1, n // 40), d))
        e = centers[rng.integers(0, len(centers), n)] + rng.normal(0, 0.2, (n, d))
    else:
        e = rng.standard_normal((n, d))
    return torch.from_numpy(e.astype(np.float16))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _bound(d):
    return d * 2.0 ** -24 + 2.0 ** -21


def _d64(x, y):
    """fp64 cosine distance of the fp16 values (rows of y against rows of x), zero vectors -> 1."""
    a, b = x.double().cpu().numpy(), y.double().cpu().numpy()
    na, nb = np.sqrt((a * a).sum(1)), np.sqrt((b * b).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1 - (b @ a.T) / nb[:, None] / na[None, :]
    d = np.clip(d, 0, 2)
    d[(na[None, :] == 0) | (nb[:, None] == 0)] = 1
    return d


def _sorted_ref(block, k, first, sim):
    v, i = torch.sort(block, dim=1, descending=sim, stable=True)
    i, v = i[:, first:first + k].to(torch.int32), v[:, first:first + k]
    if i.shape[1] < k:                                               # ranks beyond the row: -1, 0
        pad = k - i.shape[1]
        i = torch.cat([i, torch.full((i.shape[0], pad), -1, dtype=torch.int32, device=i.device)], 1)
        v = torch.cat([v, torch.zeros((v.shape[0], pad), dtype=v.dtype, device=v.device)], 1)
    return i, v


def _check_knn(nat, xc, yc, k, first, sim, block):
    fi, fw = nat.cosine_knn(xc, yc, k, first=first, similarity=sim)
    si, sw = _sorted_ref(block, k, first, sim)
    assert torch.equal(fi, si), (k, first, sim)
    assert np.array_equal(_bits(fw), _bits(sw)), (k, first, sim)
    return fi


def _dense_eps(block, cmp, eps, sim):
    e = float(np.float32(eps))
    op = {0: torch.le, 1: torch.lt, 2: torch.eq, 3: torch.ge, 4: torch.gt}[cmp]
    hit = (op(torch.full_like(block, e), block) & (block < 1)) if sim else (op(block, torch.full_like(block, e)) & (block > 0))
    rows, cols = torch.nonzero(hit, as_tuple=True)
    indptr = torch.zeros(block.shape[0] + 1, dtype=torch.int64, device=block.device)
    indptr[1:] = torch.cumsum(hit.sum(1), 0)
    return indptr, cols.to(torch.int32), block[rows, cols]


def _check_eps(nat, xc, yc, cmp, eps, sim, block, cap=256):
    got = nat.cosine_eps(xc, yc, cmp, eps, similarity=sim, cap=cap)
    want = _dense_eps(block, cmp, eps, sim)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (cmp, eps, sim, cap)
    assert np.array_equal(_bits(got[2]), _bits(want[2])), (cmp, eps, sim, cap)
    return got


def _thresholds(block, sim):
    v = np.sort(block.cpu().numpy().reshape(-1))
    v = v[(v < 1) if sim else (v > 0)]
    return [float(v[int(q * (len(v) - 1))]) for q in (0.03, 0.5)] if len(v) else [0.5]


@pytest.mark.parametrize("d", DIMS)
def test_fused_equals_dense(nat, d):
    """X self graphs (N = 300: not a multiple of 32 or 256) and M != N with Y rows that are not in X."""
    dev = nat.device()
    x = _emb(300, d, seed=d).to(dev)
    y = _emb(77, d, seed=d + 1000).to(dev)
    xc, yc = nat.cosine_prep(x), nat.cosine_prep(y)
    assert not xc.nonfinite() and not yc.nonfinite()
    for a, b in ((xc, xc), (xc, yc)):
        dist = nat.cosine_dense(a, b)
        sim = nat.cosine_dense(a, b, similarity=True)
        assert dist.shape == (b.n, a.n) and dist.dtype == torch.float32
        # s is 1/(1+d) of the kernel's own d, correctly rounded (the CPU quotient is IEEE)
        assert np.array_equal(_bits(sim), _bits(1 / (1 + dist.cpu())))
        for s, block in ((False, dist), (True, sim)):
            for k in (1, 16, 63):
                for first in (0, 1):
                    _check_knn(nat, a, b, k, first, s, block)
            for eps in _thresholds(block, s):
                for c in CMPS:
                    _check_eps(nat, a, b, getattr(nat, c), eps, s, block)


@pytest.mark.parametrize("d", [1, 9, 64, 100, 1280])
def test_accuracy_against_fp64(nat, d):
    dev = nat.device()
    x = _emb(260, d, seed=7 * d, kind="clustered").to(dev)
    y = _emb(50, d, seed=7 * d + 1).to(dev)
    y[7] = x[3]
    x[11] = 0
    xc, yc = nat.cosine_prep(x), nat.cosine_prep(y)
    bound = _bound(d)
    for a, b, xa, xb in ((xc, xc, x, x), (xc, yc, x, y)):
        got = nat.cosine_dense(a, b).double().cpu().numpy()
        ref = _d64(xa, xb)
        assert np.abs(got - ref).max() <= bound, float(np.abs(got - ref).max())
        k = 16
        idx, _ = nat.cosine_knn(a, b, k, first=0)
        idx = idx.cpu().numpy().astype(np.int64)
        mine = np.sort(np.take_along_axis(ref, idx, 1), 1)
        best = np.sort(ref, 1)[:, :k]
        assert np.abs(mine - best).max() <= 2 * bound
        for eps in (0.3, 0.9, 1.0):
            ip, ix, _ = (t.cpu().numpy() for t in nat.cosine_eps(a, b, nat.CMP_LE, eps))
            hit = np.zeros(ref.shape, dtype=bool)
            hit[np.repeat(np.arange(ref.shape[0]), np.diff(ip)), ix] = True
            want = (ref <= eps) & (ref > 0)
            clear = (np.abs(ref - eps) > bound) & (ref > bound)
            assert np.array_equal(hit[clear], want[clear]), eps


def test_duplicates_self_pairs_and_zero_vectors(nat):
    """Duplicated rows across 16 / 32 / 256 boundaries, every self pair: d == 0 exactly (rule 2: the MFMA element
    does not depend on its place in the tile); no eps graph holds them; the kNN rank 0 of a duplicate group is its
    smallest column.  Zero vectors: d == 1."""
    dev = nat.device()
    n = 600
    for d in (9, 64, 1280):
        x = _emb(n, d, seed=d + 5)
        groups = [(3, 20), (15, 16), (31, 32), (100, 290), (255, 256), (10, 511), (40, 599), (5, 300, 450), (63, 64, 65)]
        for g in groups:
            for j in g[1:]:
                x[j] = x[g[0]]
        x[200] = 0
        x[201] = 0
        x = x.to(dev)
        xc = nat.cosine_prep(x)
        block = nat.cosine_dense(xc, xc)
        b = block.cpu().numpy()
        live = np.ones(n, dtype=bool)
        live[[200, 201]] = False
        assert np.all(np.diag(b)[live] == 0)
        for g in groups:
            for i in g:
                for j in g:
                    assert b[i, j] == 0, (d, i, j)
        assert np.all(b[200] == 1) and np.all(b[:, 201] == 1)
        zero_pairs = {(i, j) for i, j in zip(*np.nonzero(b == 0))}
        dup = {(i, i) for i in np.nonzero(live)[0]} | {(i, j) for g in groups for i in g for j in g}
        assert zero_pairs == dup, d
        idx, w = nat.cosine_knn(xc, xc, 4, first=0)
        idx = idx.cpu().numpy()
        for g in groups:
            for i in g:
                assert idx[i, 0] == min(g), (d, i, idx[i])
        for sim in (False, True):
            blk = nat.cosine_dense(xc, xc, similarity=sim)
            for c in CMPS:
                for eps in (0.0, 0.5, 1.0, 2.0):
                    e = 1 / (1 + eps) if sim else eps
                    ip, ix, _ = _check_eps(nat, xc, xc, getattr(nat, c), e, sim, blk)
                    rows = np.repeat(np.arange(n), np.diff(ip.cpu().numpy()))
                    assert not any((int(r), int(j)) in dup for r, j in zip(rows, ix.cpu().numpy()))


def test_eps_rows_beyond_the_slot_capacity(nat):
    """A tight cluster with cap = 4: most rows outgrow their slot and take the restricted second sweep."""
    rng = np.random.default_rng(5)
    dev = nat.device()
    for d in (9, 64, 1280):
        base = rng.normal(0, 1, d)
        e = np.concatenate([base + rng.normal(0, 0.05, (300, d)), rng.normal(0, 1, (700, d))]).astype(np.float16)
        xc = nat.cosine_prep(torch.from_numpy(e).to(dev))
        for sim in (False, True):
            block = nat.cosine_dense(xc, xc, similarity=sim)
            eps, cmp = (1 / 1.1, nat.CMP_GE) if sim else (0.1, nat.CMP_LE)
            big = _check_eps(nat, xc, xc, cmp, eps, sim, block, cap=100_000)
            assert int((torch.diff(big[0]) > 4).sum()) >= 250               # the overflow sweep does run
            for cap in (4, 1):
                got = _check_eps(nat, xc, xc, cmp, eps, sim, block, cap=cap)
                assert all(torch.equal(a, b) for a, b in zip(got, big))


def test_non_finite_elements_fall_back(nat):
    from prograph_amd.distance import cosine
    from prograph_amd.distance.cosine import _torch_cosine
    dev = nat.device()
    for bad in (float("inf"), float("-inf"), float("nan")):
        for pos in ((0, 0), (37, 5), (299, 63)):
            x = _emb(300, 64, seed=1).to(dev)
            x[pos] = bad
            assert nat.cosine_prep(x).nonfinite()
            y = _emb(20, 64, seed=2).to(dev)
            assert not nat.cosine_prep(y).nonfinite()
            for sim in (False, True):
                got, want = cosine(x, y, similarity=sim), _torch_cosine(x, y, sim)
                assert got.dtype == torch.float32 and torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0))
                got = cosine(y, x, similarity=sim)
                want = _torch_cosine(y, x, sim)
                assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0))


def test_operator_takes_the_kernel(nat):
    from prograph_amd.distance import cosine
    dev = nat.device()
    x, y = _emb(100, 17, seed=3).to(dev), _emb(30, 17, seed=4).to(dev)
    xc, yc = nat.cosine_prep(x), nat.cosine_prep(y)
    for sim in (False, True):
        assert np.array_equal(_bits(cosine(x, y, similarity=sim)), _bits(nat.cosine_dense(xc, yc, similarity=sim)))


def test_full_size_fused_equals_dense(nat):
    """N = 50 000, D = 1280: kNN 16 of the fused sweep against sorting the dense block in row blocks."""
    rng = np.random.default_rng(1280)
    n, d = 50_000, 1280
    dev = nat.device()
    x = torch.from_numpy(rng.standard_normal((n, d), dtype=np.float32).astype(np.float16)).to(dev)
    xc = nat.cosine_prep(x)
    fi, fw = nat.cosine_knn(xc, xc, 16, first=1)
    rows = 2048
    for r0 in range(0, n, rows):
        yc = nat.cosine_prep(x[r0:r0 + rows])
        si, sw = _sorted_ref(nat.cosine_dense(xc, yc), 16, 1, False)
        assert torch.equal(fi[r0:r0 + rows], si), r0
        assert np.array_equal(_bits(fw[r0:r0 + rows]), _bits(sw)), r0


def _prograph(tmp_path, n, name, seed=3):
    from prograph_amd import Prograph
    tok = synth.clustered_tokens(n, 8, seed=seed)
    f = tmp_path / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(seed).uniform(0, 1, n)}).to_csv(f)
    return Prograph(file=str(f))


def _row_bound(pg, graph, boolean):
    col = pg.graph[graph]
    nnz = np.array([len(c[0]) for c in col], dtype=np.float64)
    s = np.array([np.abs(np.asarray(c[1], dtype=np.float64)).sum() for c in col])
    return nnz * 2.0 ** -24 * (nnz if boolean else s) + 1e-300


def test_build_graph_cosine(nat, tmp_path, capsys):
    """build_graph(distance=cosine): the fused graphs equal the kernels' own selection, k / eps, similarity, idxs."""
    from prograph_amd.distance import cosine
    from prograph_amd.graph import CSRGraph, KNNGraph
    n, d = 700, 33
    pg = _prograph(tmp_path, n, "b", seed=2)
    capsys.readouterr()
    emb = _emb(n, d, seed=9, kind="clustered").numpy()
    emb[50] = emb[400]
    pg.graph["Embedded"] = list(emb.astype(np.float32))
    x = torch.from_numpy(emb).to(nat.device())
    xc = nat.cosine_prep(x)
    for sim in (False, True):
        G = pg.build_graph(representation="Embedded", k=8, similarity=sim, distance=cosine, output="csr")
        assert isinstance(G, KNNGraph) and G.dist.dtype == torch.float32 and G.final
        si, sw = _sorted_ref(nat.cosine_dense(xc, xc, similarity=sim), 8, 1, sim)
        assert torch.equal(G.idx, si) and np.array_equal(_bits(G.dist), _bits(sw))
        t = pg.build_graph(representation="Embedded", k=8, similarity=sim, distance=cosine)
        assert all(np.array_equal(a[0], b) and a[1].dtype == np.float32 and np.array_equal(a[1], c)
                   for a, b, c in zip(t, si.cpu().numpy(), sw.cpu().numpy()))
        eps = 0.2
        E = pg.build_graph(representation="Embedded", eps=eps, similarity=sim, distance=cosine, output="csr")
        assert isinstance(E, CSRGraph) and E.weights.dtype == torch.float32 and E.final
        want = _dense_eps(nat.cosine_dense(xc, xc, similarity=sim), nat.CMP_LE, 1 / (1 + eps) if sim else eps, sim)
        assert torch.equal(E.indptr, want[0]) and torch.equal(E.indices, want[1])
        assert np.array_equal(_bits(E.weights), _bits(want[2]))
        ip, ix, w = E.host()
        assert w.dtype == np.float32 and np.array_equal(w, want[2].cpu().numpy())
    sub = np.arange(0, n, 3)
    G = pg.build_graph(idxs=sub, representation="Embedded", k=5, distance=cosine, output="csr")
    sc = nat.cosine_prep(x[torch.as_tensor(sub, device=x.device)])
    si, sw = _sorted_ref(nat.cosine_dense(sc, sc), 5, 1, False)
    assert G.nrows == len(sub) and torch.equal(G.idx, si) and np.array_equal(_bits(G.dist), _bits(sw))


def test_build_graph_cosine_non_finite_takes_the_generic_path(nat, tmp_path, capsys):
    from prograph_amd.distance import cosine
    from prograph_amd.distance.cosine import _torch_cosine
    n, d = 120, 16
    pg = _prograph(tmp_path, n, "nf", seed=4)
    capsys.readouterr()
    emb = _emb(n, d, seed=10).numpy().astype(np.float32)
    emb[7, 3] = np.inf
    pg.graph["Embedded"] = list(emb)
    t = pg.build_graph(representation="Embedded", k=4, distance=cosine, output="csr")
    assert isinstance(t, list) and len(t) == n                       # the generic batch loop's tuples
    X = torch.from_numpy(emb.astype(np.float16)).to(nat.device())
    block = torch.cat([_torch_cosine(X, X[r0:r0 + 8], False) for r0 in range(0, n, 8)])     # the loop's batches of 8
    v, i = torch.sort(block, dim=1, stable=True)
    assert all(np.array_equal(a[0], b) for a, b in zip(t, i[:, 1:5].cpu().numpy()))


@pytest.mark.parametrize("kind", ["knn", "eps"])
def test_device_analytics_match_the_column_path(nat, tmp_path, capsys, kind):
    from prograph_amd.distance import cosine
    from prograph_amd.utils import save
    n, d = 2000, 16
    pg = _prograph(tmp_path, n, "an", seed=11)
    capsys.readouterr()
    rng = np.random.default_rng(12)
    centers = rng.normal(0, 1, (100, d))
    pg.graph["Embedded"] = list((centers[rng.integers(0, 100, n)] + rng.normal(0, 0.3, (n, d))).astype(np.float32))
    args = dict(k=10) if kind == "knn" else dict(eps=0.05)
    tuples = pg.build_graph(representation="Embedded", distance=cosine, store="E", **args)
    assert pg._device_graph("E") is not None and pg.csr_graphs["E"].final
    again = pg.build_graph(representation="Embedded", distance=cosine, **args)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].dtype == b[1].dtype
               for a, b in zip(tuples, again))
    assert all(a[1].dtype == np.float32 for a in tuples if len(a[0]))      # empty rows: the reference's int pair
    if kind == "eps":
        assert min(len(t[0]) for t in tuples) == 0 and max(len(t[0]) for t in tuples) > 0
    pg.graph["T"] = list(tuples)
    assert pg._device_graph("T") is None
    assert np.array_equal(pg.degree("E", boolean_weights=True), pg.degree("T", boolean_weights=True))
    dw, cw = pg.degree("E").astype(np.float64), pg.degree("T").astype(np.float64)
    assert np.all(np.abs(dw - cw) <= _row_bound(pg, "T", False)), float(np.abs(dw - cw).max())
    for b in (False, True):
        for mode in ("outdegree", "indegree"):
            de, dc = pg.dirichlet("E", boolean_weights=b, mode=mode), pg.dirichlet("T", boolean_weights=b, mode=mode)
            assert np.allclose(de, dc, rtol=1e-6, atol=0), (b, mode, de, dc)
    ve, vc = pg.local_variance("E"), pg.local_variance("T")
    assert np.array_equal(np.isnan(ve), np.isnan(vc))
    ok = ~np.isnan(vc)
    assert np.allclose(ve[ok], vc[ok], rtol=1e-12, atol=1e-14)
    from prograph_amd import Prograph
    assert save(pg, name="cs", directory=str(tmp_path) + "/", graphs="csr")
    back = Prograph(file=str(tmp_path / "cs.pkl"))
    capsys.readouterr()
    g0, g1 = pg.csr_graphs["E"], back.csr_graphs["E"]
    assert type(g0) is type(g1) and g1.final and g0.similarity == g1.similarity and g0.ncols == g1.ncols
    for a in (("idx", "dist") if kind == "knn" else ("indptr", "indices", "weights")):
        t0, t1 = getattr(g0, a), getattr(g1, a)
        assert t0.dtype == t1.dtype and torch.equal(t0.cpu(), t1.cpu())
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[1].dtype == b[1].dtype
               for a, b in zip(back.graph["E"], pg.graph["E"]))
    assert back._device_graph("E") is not None
    assert np.array_equal(back.degree("E"), pg.degree("E"))
