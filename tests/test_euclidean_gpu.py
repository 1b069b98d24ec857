"""
GPU checks of the Euclidean kernels (pg_euclidean_dense / _knn / _knn_round / _eps_*, prograph_amd/csrc/pg_cos.hip): the
fused graphs equal the selection over the dense block bit for bit (shared tile routine and epilogue), the values are
within the stated bound of fp64, identical vectors are exactly 0 wherever they sit in a tile and nothing else is, a zero
vector is an ordinary point, non-finite inputs take the torch expression, `build_graph(distance=euclidean)` and `search`
feed the device analytics, and `minkowski` is untouched.

The bound is on the SQUARE: |got^2 - d^2| <= B(D) (nx + ny) + 2^-22 d^2, B(D) = 2 D 2^-24 + 2^-21, with
d^2, nx, ny the exact values of the fp16 inputs.  Selections are compared in d^2: a column chosen in place of a better
one is within the sum of the two pairs' bounds of it, hence within twice the row's largest bound.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from prograph_amd import synth

pytestmark = pytest.mark.gpu

CMPS = ["CMP_LE", "CMP_LT", "CMP_EQ", "CMP_GE", "CMP_GT"]
DIMS = [1, 7, 8, 9, 15, 16, 17, 64, 100, 1280]
N, M = 300, 77                    # columns (not a multiple of 32 or 256: three workgroups' worth of tiles) and rows


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def _emb(n, d, seed, kind="normal", scale=1.0):
    rng = np.random.default_rng(seed)
    if kind == "clustered":
        centers = rng.normal(0, 1, (max(1, n // 40), d))
        e = centers[rng.integers(0, len(centers), n)] + rng.normal(0, 0.2, (n, d))
    else:
        e = rng.standard_normal((n, d))
    return torch.from_numpy((e * scale).astype(np.float16))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _B(d):
    return 2 * d * 2.0 ** -24 + 2.0 ** -21


def _ref2(x, y):
    """Exact d^2 of the fp16 values in fp64 (rows of y against rows of x), direct form, and the bound of every pair."""
    a, b = x.double().cpu().numpy(), y.double().cpu().numpy()
    d2 = np.stack([((r[None, :] - a) ** 2).sum(1) for r in b])
    na, nb = (a * a).sum(1), (b * b).sum(1)
    return d2, _B(a.shape[1]) * (na[None, :] + nb[:, None]) + 2.0 ** -22 * d2


def _sorted_ref(block, k, first, sim):
    v, i = torch.sort(block, dim=1, descending=sim, stable=True)
    i, v = i[:, first:first + k].to(torch.int32), v[:, first:first + k]
    if i.shape[1] < k:                                               # ranks beyond the row: -1, 0
        pad = k - i.shape[1]
        i = torch.cat([i, torch.full((i.shape[0], pad), -1, dtype=torch.int32, device=i.device)], 1)
        v = torch.cat([v, torch.zeros((v.shape[0], pad), dtype=v.dtype, device=v.device)], 1)
    return i, v


def _check_knn(nat, xc, yc, k, first, sim, block, **kw):
    fi, fw = nat.euclidean_knn(xc, yc, k, first=first, similarity=sim, **kw)
    si, sw = _sorted_ref(block, k, first, sim)
    assert torch.equal(fi, si), (k, first, sim)
    assert np.array_equal(_bits(fw), _bits(sw)), (k, first, sim)
    return fi


def _dense_eps(block, cmp, eps, sim, keep_zero=False):
    e = float(np.float32(eps))
    op = {0: torch.le, 1: torch.lt, 2: torch.eq, 3: torch.ge, 4: torch.gt}[cmp]
    hit = op(torch.full_like(block, e), block) if sim else op(block, torch.full_like(block, e))
    if not keep_zero:
        hit &= (block < 1) if sim else (block > 0)
    rows, cols = torch.nonzero(hit, as_tuple=True)
    indptr = torch.zeros(block.shape[0] + 1, dtype=torch.int64, device=block.device)
    indptr[1:] = torch.cumsum(hit.sum(1), 0)
    return indptr, cols.to(torch.int32), block[rows, cols]


def _check_eps(nat, xc, yc, cmp, eps, sim, block, cap=256, **kw):
    got = nat.euclidean_eps(xc, yc, cmp, eps, similarity=sim, cap=cap, **kw)
    want = _dense_eps(block, cmp, eps, sim, keep_zero=kw.get("keep_zero", False))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (cmp, eps, sim, cap)
    assert np.array_equal(_bits(got[2]), _bits(want[2])), (cmp, eps, sim, cap)
    return got


def _thresholds(block, sim):
    """Two values of the block itself (so that == has hits): its 3 % and 50 % quantiles."""
    v = np.sort(block.cpu().numpy().reshape(-1))
    v = v[(v < 1) if sim else (v > 0)]
    return [float(v[int(q * (len(v) - 1))]) for q in (0.03, 0.5)] if len(v) else [0.5]


@pytest.mark.parametrize("d", DIMS)
def test_fused_equals_dense(nat, d):
    """X self graphs and M != N with Y rows that are not in X: distances and similarities, k = 1, 16, 63 with first = 0
    and 1, all five comparators at two thresholds of the block's own."""
    dev = nat.device()
    x = _emb(N, d, seed=d).to(dev)
    y = _emb(M, d, seed=d + 1000).to(dev)
    xc, yc = nat.cosine_prep(x), nat.cosine_prep(y)
    assert not xc.nonfinite() and not yc.nonfinite()
    for a, b in ((xc, xc), (xc, yc)):
        dist = nat.euclidean_dense(a, b)
        sim = nat.euclidean_dense(a, b, similarity=True)
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


def test_knn_beyond_one_round(nat):
    """k = 64 and 130 through pg_euclidean_knn_round (and a last round that runs out of columns), Y rows in blocks."""
    dev = nat.device()
    x, y = _emb(N, 17, seed=21).to(dev), _emb(M, 17, seed=22).to(dev)
    x[40] = x[12]                                                     # a tie across a round's floor is by column
    xc, yc = nat.cosine_prep(x), nat.cosine_prep(y)
    for a, b in ((xc, xc), (xc, yc)):
        for s in (False, True):
            block = nat.euclidean_dense(a, b, similarity=s)
            for k, first in ((64, 0), (64, 1), (130, 0), (130, 1), (N, 1)):
                _check_knn(nat, a, b, k, first, s, block)
            _check_knn(nat, a, b, 130, 1, s, block, rows_per_block=64)


def test_eps_rows_beyond_the_slot_capacity(nat):
    """cap below the row counts: the rows beyond it take the restricted sweep over a row list (pg_euclidean_eps_fill_rows),
    the others the compaction; all of them, some of them, and with the Y rows in blocks."""
    dev = nat.device()
    for d in (9, 64, 1280):
        x, y = _emb(N, d, seed=d + 31, kind="clustered").to(dev), _emb(M, d, seed=d + 32, kind="clustered").to(dev)
        xc, yc = nat.cosine_prep(x), nat.cosine_prep(y)
        for a, b in ((xc, xc), (xc, yc)):
            for sim in (False, True):
                block = nat.euclidean_dense(a, b, similarity=sim)
                eps = _thresholds(block, sim)[0]
                cmp = nat.CMP_GE if sim else nat.CMP_LE
                big = _check_eps(nat, a, b, cmp, eps, sim, block, cap=100_000)
                counts = torch.diff(big[0])
                some = int(counts.median())                           # about half of the rows are beyond this cap
                assert 0 < int((counts > some).sum()) < b.n and int(counts.max()) > 4
                for cap, rpb in ((some, None), (4, None), (1, None), (some, 50)):
                    got = _check_eps(nat, a, b, cmp, eps, sim, block, cap=cap, rows_per_block=rpb)
                    assert all(torch.equal(p, q) for p, q in zip(got, big))


def test_restricted_sweep_with_a_row_list(nat):
    """pg_euclidean_eps_fill_rows on a row list of its own - unordered rows across tile and workgroup boundaries, a list
    that is no multiple of 32 - writes exactly those rows' segments of the dense block's CSR."""
    import ctypes
    dev = nat.device()
    x = _emb(N, 33, seed=41).to(dev)
    xc = nat.cosine_prep(x)
    block = nat.euclidean_dense(xc, xc)
    eps = _thresholds(block, False)[1]
    indptr, indices, weights = _dense_eps(block, nat.CMP_LT, eps, False)
    rows = torch.tensor([299, 0, 31, 32, 33, 127, 128, 255, 256, 17, 290, 5] + list(range(60, 95)), dtype=torch.int64, device=dev)
    got_i = torch.full_like(indices, -7)
    got_w = torch.full_like(weights, -7.0)
    y, yn, yr, m = xc.rows(0, xc.n)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = nat.lib().pg_euclidean_eps_fill_rows(p(xc.packed.buf), p(xc.norms), p(xc.rnorms), xc.n, xc.packed.npad, y, yn, yr, m,
                                              xc.packed.npad, xc.d, 0, nat.CMP_LT, float(np.float32(eps)), p(rows), len(rows),
                                              p(indptr), p(got_i), p(got_w), None)
    assert rc == 0
    torch.cuda.synchronize()
    listed = torch.zeros(N, dtype=torch.bool, device=dev)
    listed[rows] = True
    seg = torch.repeat_interleave(listed, torch.diff(indptr))
    assert seg.any() and not seg.all()
    assert torch.equal(got_i[seg], indices[seg]) and np.array_equal(_bits(got_w[seg]), _bits(weights[seg]))
    assert torch.all(got_i[~seg] == -7) and torch.all(got_w[~seg] == -7.0)          # nothing outside the listed rows


@pytest.mark.parametrize("scale", [1.0, 1e-3, 30.0])
@pytest.mark.parametrize("d", [1, 9, 64, 100, 1280])
def test_accuracy_against_fp64(nat, d, scale):
    dev = nat.device()
    x = _emb(N, d, seed=7 * d, kind="clustered", scale=scale).to(dev)
    y = _emb(M, d, seed=7 * d + 1, kind="clustered", scale=scale).to(dev)
    y[7] = x[3]
    x[11] = 0
    xc, yc = nat.cosine_prep(x), nat.cosine_prep(y)
    for a, b, xa, xb in ((xc, xc, x, x), (xc, yc, x, y)):
        ref2, bound = _ref2(xa, xb)
        got = nat.euclidean_dense(a, b).double().cpu().numpy()
        err = np.abs(got * got - ref2)
        worst = float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())
        print(f"D={d} scale={scale} {'self' if a is b else 'M!=N'}: max err/bound = {worst:.4f}")
        assert np.all(err <= bound), worst
        k = 16
        idx, _ = nat.euclidean_knn(a, b, k, first=0)
        idx = idx.cpu().numpy().astype(np.int64)
        mine = np.sort(np.take_along_axis(ref2, idx, 1), 1)
        best = np.sort(ref2, 1)[:, :k]
        assert np.all(np.abs(mine - best) <= 2 * bound.max(1)[:, None])
        r = np.sqrt(ref2)
        for eps in (float(np.quantile(r, 0.05)), float(np.quantile(r, 0.5))):
            ip, ix, _ = (t.cpu().numpy() for t in nat.euclidean_eps(a, b, nat.CMP_LE, eps))
            hit = np.zeros(ref2.shape, dtype=bool)
            hit[np.repeat(np.arange(ref2.shape[0]), np.diff(ip)), ix] = True
            e2 = float(np.float32(eps)) ** 2
            want = ref2 <= e2
            clear = (np.abs(ref2 - e2) > bound) & (ref2 > bound)          # of the threshold and of 0 by more than the bound
            left_out = int((~clear).sum())
            print(f"  eps={eps:.4g}: {left_out} of {clear.size} pairs left out")
            assert left_out <= 0.05 * clear.size, (left_out, clear.size)
            assert np.array_equal(hit[clear], want[clear]), eps


def test_duplicates_self_pairs_and_zero_vectors(nat):
    """Duplicated rows across 16 / 32 / 256 boundaries and lane halves, every self pair, two zero vectors: d == 0 exactly
    (the MFMA element does not depend on its place in the tile) and nowhere else; no eps graph holds them; the kNN rank
    0 of a duplicate group is its smallest column.  A zero vector's row is sqrt(ny): (0 + ny) - (0 + 0) is ny."""
    dev = nat.device()
    n = 600
    for d in (9, 64, 1280):
        x = _emb(n, d, seed=d + 5)
        groups = [(3, 20), (15, 16), (31, 32), (100, 290), (255, 256), (10, 511), (40, 599), (5, 300, 450), (63, 64, 65),
                  (200, 201)]
        for g in groups[:-1]:
            for j in g[1:]:
                x[j] = x[g[0]]
        x[200] = 0
        x[201] = 0
        x = x.to(dev)
        xc = nat.cosine_prep(x)
        block = nat.euclidean_dense(xc, xc)
        b = block.cpu().numpy()
        zero_pairs = {(i, j) for i, j in zip(*np.nonzero(b == 0))}
        dup = {(i, i) for i in range(n)} | {(i, j) for g in groups for i in g for j in g}
        assert zero_pairs == dup, d
        # correctly rounded, as the kernel's: the fp64 root of an fp32 value rounds to fp32 without a double-rounding error
        root = torch.from_numpy(np.sqrt(xc.norms[:n].cpu().numpy().astype(np.float64)).astype(np.float32))
        for z in (200, 201):
            assert np.array_equal(_bits(block[z]), _bits(root)) and np.array_equal(_bits(block[:, z]), _bits(root))
        idx, w = nat.euclidean_knn(xc, xc, 4, first=0)
        idx, w = idx.cpu().numpy(), w.cpu().numpy()
        assert np.all(w[:, 0] == 0)
        for g in groups:
            for i in g:
                assert idx[i, 0] == min(g), (d, i, idx[i])
        for sim in (False, True):
            blk = nat.euclidean_dense(xc, xc, similarity=sim)
            for c in CMPS:
                for eps in (0.0, float(np.median(b))):
                    e = 1 / (1 + eps) if sim else eps
                    ip, ix, _ = _check_eps(nat, xc, xc, getattr(nat, c), e, sim, blk)
                    rows = np.repeat(np.arange(n), np.diff(ip.cpu().numpy()))
                    assert not any((int(r), int(j)) in dup for r, j in zip(rows, ix.cpu().numpy()))
            # rows of queries keep them: d <= 0, or 1 <= s
            ip, ix, _ = _check_eps(nat, xc, xc, nat.CMP_LE, 1.0 if sim else 0.0, sim, blk, keep_zero=True)
            rows = np.repeat(np.arange(n), np.diff(ip.cpu().numpy()))
            assert {(int(r), int(j)) for r, j in zip(rows, ix.cpu().numpy())} == dup


def test_non_finite_elements_fall_back(nat):
    from prograph_amd.distance import euclidean
    from prograph_amd.distance.euclidean import _torch_euclidean
    dev = nat.device()
    for bad in (float("inf"), float("-inf"), float("nan")):
        for pos in ((0, 0), (37, 5), (299, 63)):
            x = _emb(N, 64, seed=1).to(dev)
            x[pos] = bad
            assert nat.cosine_prep(x).nonfinite()
            y = _emb(20, 64, seed=2).to(dev)
            for sim in (False, True):
                for p, q in ((x, y), (y, x)):
                    got, want = euclidean(p, q, similarity=sim), _torch_euclidean(p, q, sim)
                    assert got.dtype == torch.float32 and got.is_cuda
                    assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0))


def test_operator_takes_the_kernel(nat):
    from prograph_amd.distance import euclidean
    dev = nat.device()
    x, y = _emb(100, 17, seed=3).to(dev), _emb(30, 17, seed=4).to(dev)
    xc, yc = nat.cosine_prep(x), nat.cosine_prep(y)
    for sim in (False, True):
        assert np.array_equal(_bits(euclidean(x, y, similarity=sim)), _bits(nat.euclidean_dense(xc, yc, similarity=sim)))
        assert np.array_equal(_bits(euclidean(x, x, similarity=sim)), _bits(nat.euclidean_dense(xc, xc, similarity=sim)))
    # beyond fp16's sum range: minkowski's inf, here the value
    big = torch.full((1, 16), 4096, dtype=torch.float16, device=dev)
    assert float(euclidean(big, torch.zeros_like(big))) == 16384.0


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


def test_build_graph_euclidean(nat, tmp_path, capsys):
    """build_graph(distance=euclidean): the fused graphs equal the selection over euclidean(X, X); k / eps, similarity,
    k beyond one round, idxs relative to the subset."""
    from prograph_amd.distance import euclidean
    from prograph_amd.graph import CSRGraph, KNNGraph
    n, d = 700, 33
    pg = _prograph(tmp_path, n, "b", seed=2)
    capsys.readouterr()
    emb = _emb(n, d, seed=9, kind="clustered").numpy()
    emb[50] = emb[400]
    pg.graph["Embedded"] = list(emb.astype(np.float32))
    x = torch.from_numpy(emb).to(nat.device())
    for sim in (False, True):
        block = euclidean(x, x, similarity=sim)
        for k in (16, 70):
            G = pg.build_graph(representation="Embedded", k=k, similarity=sim, distance=euclidean, output="csr")
            assert isinstance(G, KNNGraph) and G.dist.dtype == torch.float32 and G.final
            si, sw = _sorted_ref(block, k, 1, sim)
            assert torch.equal(G.idx, si) and np.array_equal(_bits(G.dist), _bits(sw))
        t = pg.build_graph(representation="Embedded", k=16, similarity=sim, distance=euclidean)
        si, sw = _sorted_ref(block, 16, 1, sim)
        assert all(np.array_equal(a[0], b) and a[1].dtype == np.float32 and np.array_equal(a[1], c)
                   for a, b, c in zip(t, si.cpu().numpy(), sw.cpu().numpy()))
        eps = float(np.quantile(euclidean(x, x).cpu().numpy(), 0.02))
        for cap in (256, 3):
            E = pg.build_graph(representation="Embedded", eps=eps, similarity=sim, distance=euclidean, output="csr", cap=cap)
            assert isinstance(E, CSRGraph) and E.weights.dtype == torch.float32 and E.final
            want = _dense_eps(block, nat.CMP_LE, 1 / (1 + eps) if sim else eps, sim)
            assert int(want[0][-1]) > n and torch.equal(E.indptr, want[0]) and torch.equal(E.indices, want[1])
            assert np.array_equal(_bits(E.weights), _bits(want[2]))
        assert 400 not in E.to_tuples()[50][0]                           # the duplicate pair is dropped like a self pair
    sub = np.arange(0, n, 3)
    G = pg.build_graph(idxs=sub, representation="Embedded", k=5, distance=euclidean, output="csr")
    xs = x[torch.as_tensor(sub, device=x.device)]
    si, sw = _sorted_ref(euclidean(xs, xs), 5, 1, False)
    assert G.nrows == len(sub) and torch.equal(G.idx, si) and np.array_equal(_bits(G.dist), _bits(sw))
    assert int(G.idx.max()) < len(sub)


def test_search_euclidean(nat, tmp_path, capsys):
    """search(distance=euclidean): rank 0 and d = 0 are kept; k (one round and beyond) and eps; nearest_neighbour."""
    from prograph_amd.distance import euclidean
    from prograph_amd.graph import CSRGraph, KNNGraph
    n, d = 500, 20
    pg = _prograph(tmp_path, n, "s", seed=5)
    capsys.readouterr()
    emb = _emb(n, d, seed=13, kind="clustered").numpy()
    pg.graph["Embedded"] = list(emb.astype(np.float32))
    q = np.concatenate([emb[[7, 300]], _emb(40, d, seed=14, kind="clustered").numpy()]).astype(np.float32)
    x, y = torch.from_numpy(emb).to(nat.device()), torch.from_numpy(q).to(nat.device()).half()
    for sim in (False, True):
        block = euclidean(x, y, similarity=sim)
        for k in (1, 16, 100):
            G = pg.search(q, k=k, distance=euclidean, representation="Embedded", similarity=sim, output="csr")
            assert isinstance(G, KNNGraph) and G.final and G.dist.dtype == torch.float32
            si, sw = _sorted_ref(block, k, 0, sim)
            assert torch.equal(G.idx, si) and np.array_equal(_bits(G.dist), _bits(sw))
        assert int(G.idx[0, 0]) == 7 and int(G.idx[1, 0]) == 300 and float(G.dist[0, 0]) == (1.0 if sim else 0.0)
        eps = float(np.quantile(euclidean(x, y).cpu().numpy(), 0.03))
        E = pg.search(q, eps=eps, distance=euclidean, representation="Embedded", similarity=sim, output="csr")
        assert isinstance(E, CSRGraph) and E.final
        want = _dense_eps(block, nat.CMP_LE, 1 / (1 + eps) if sim else eps, sim, keep_zero=True)
        assert torch.equal(E.indptr, want[0]) and torch.equal(E.indices, want[1]) and np.array_equal(_bits(E.weights), _bits(want[2]))
        t = E.to_tuples()
        assert 7 in t[0][0] and 300 in t[1][0]
    rows, dmin = pg.nearest_neighbour(q[:3], distance=euclidean, representation="Embedded")
    assert dmin == 0 and len(rows) == 3


def test_non_finite_graphs_take_the_generic_path(nat, tmp_path, capsys):
    from prograph_amd.distance import euclidean
    from prograph_amd.distance.euclidean import _torch_euclidean
    n, d = 120, 16
    pg = _prograph(tmp_path, n, "nf", seed=4)
    capsys.readouterr()
    emb = _emb(n, d, seed=10).numpy().astype(np.float32)
    emb[7, 3] = np.inf
    pg.graph["Embedded"] = list(emb)
    assert pg._build_graph_euclidean(None, None, 4, False, "Embedded", None) is None
    t = pg.build_graph(representation="Embedded", k=4, distance=euclidean, output="csr")
    assert isinstance(t, list) and len(t) == n                       # the generic batch loop's tuples
    X = torch.from_numpy(emb.astype(np.float16)).to(nat.device())
    block = torch.cat([_torch_euclidean(X, X[r0:r0 + 8], False) for r0 in range(0, n, 8)])     # the loop's batches of 8
    v, i = torch.sort(block, dim=1, stable=True)
    assert all(np.array_equal(a[0], b) for a, b in zip(t, i[:, 1:5].cpu().numpy()))
    # queries: a non-finite dataset or query leaves the kernels as well
    q = _emb(6, d, seed=11).numpy().astype(np.float32)
    assert pg._search_embedding(torch.from_numpy(q), 3, False, "Embedded", euclidean) is None
    assert pg._search_eps_embedding(torch.from_numpy(q), 3.0, __import__("operator").le, False, "Embedded", euclidean) is None
    res = pg.search(q, k=3, distance=euclidean, representation="Embedded")
    want = torch.sort(_torch_euclidean(X, torch.from_numpy(q).to(X.device).half(), False), dim=1, stable=True)[1][:, :3]
    assert all(np.array_equal(a[0], b) for a, b in zip(res, want.cpu().numpy()))
    res = pg.search(q, eps=4.0, distance=euclidean, representation="Embedded")
    assert len(res) == 6 and all(7 not in r[0] for r in res)


@pytest.mark.parametrize("kind", ["knn", "eps"])
def test_device_analytics_match_the_column_path(nat, tmp_path, capsys, kind):
    from prograph_amd.distance import euclidean
    n, d = 2000, 16
    pg = _prograph(tmp_path, n, "an", seed=11)
    capsys.readouterr()
    rng = np.random.default_rng(12)
    centers = rng.normal(0, 1, (100, d))
    emb = (centers[rng.integers(0, 100, n)] + rng.normal(0, 0.3, (n, d))).astype(np.float32)
    pg.graph["Embedded"] = list(emb)
    args = dict(k=16) if kind == "knn" else dict(eps=1.2)
    tuples = pg.build_graph(representation="Embedded", distance=euclidean, store="E", **args)
    assert pg._device_graph("E") is not None and pg.csr_graphs["E"].final
    block = euclidean(torch.from_numpy(emb).half().to(nat.device()), torch.from_numpy(emb).half().to(nat.device()))
    if kind == "knn":
        si, sw = _sorted_ref(block, 16, 1, False)
        assert all(np.array_equal(a[0], b) and np.array_equal(a[1], c) for a, b, c in zip(tuples, si.cpu().numpy(), sw.cpu().numpy()))
    else:
        ip, ix, w = (t.cpu().numpy() for t in _dense_eps(block, nat.CMP_LE, 1.2, False))
        assert all(np.array_equal(t[0], ix[ip[r]:ip[r + 1]]) and np.array_equal(t[1], w[ip[r]:ip[r + 1]])
                   for r, t in enumerate(tuples) if len(t[0]))
        assert min(len(t[0]) for t in tuples) == 0 and max(len(t[0]) for t in tuples) > 0
    assert all(a[1].dtype == np.float32 for a in tuples if len(a[0]))      # empty rows: the reference's int pair
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
    A = pg.adjacency("E")
    assert A.shape == (n, n)


def test_minkowski_is_untouched(nat):
    """One small fp16 operand: the Minkowski block and its fused graph have the same bits before and after the
    Euclidean operator and kernels ran on the same staging."""
    from prograph_amd.distance import euclidean, minkowski
    dev = nat.device()
    x, y = _emb(N, 24, seed=51).to(dev), _emb(M, 24, seed=52).to(dev)
    before = minkowski(x, y)
    xp = nat.pack_f16(x)
    kb = nat.minkowski_knn(xp, xp, 8, first=1)
    euclidean(x, y)
    xc = nat.cosine_prep(xp)                                             # the same packed buffer
    nat.euclidean_knn(xc, xc, 8)
    nat.euclidean_eps(xc, xc, nat.CMP_LE, 5.0, cap=2)
    after = minkowski(x, y)
    ka = nat.minkowski_knn(xp, xp, 8, first=1)
    assert before.dtype == after.dtype == torch.float16 and torch.equal(before.view(torch.int16), after.view(torch.int16))
    assert torch.equal(kb[0], ka[0]) and torch.equal(kb[1].view(torch.int16), ka[1].view(torch.int16))
