"""
GPU checks of kNN graphs beyond 63 neighbours (pg_minkowski_knn_round, pg_cosine_knn_round, pg_f16_knn_round):
build_graph(distance=minkowski / cosine, k > 63) and long byte-token sequences must return exactly what the generic
batch loop returns (indices, weights and weight dtypes, bit for bit) - on ties that straddle every round boundary
too - keep device graphs for output="csr" / store=, and match the reference's goldens at large k.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import load_golden
from prograph_amd import synth

pytestmark = pytest.mark.gpu

KS = (64, 65, 100, 127, 128, 129, 300, 1023)


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def _prograph(tmp_path, n, name, tok=None):
    from prograph_amd import Prograph
    tok = synth.clustered_tokens(n, 8, seed=3) if tok is None else tok
    f = tmp_path / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(1).uniform(0, 1, len(tok))}).to_csv(f)
    return Prograph(file=str(f))


def _generic(dist):
    """The same operator behind another name: build_graph sends it to the generic batch loop."""
    return lambda X, Y, similarity=False: dist(X, Y, similarity=similarity)


def _same(got, want, k=None):
    assert len(got) == len(want)
    for r, ((gi, gw), (wi, ww)) in enumerate(zip(got, want)):
        wi, ww = (wi, ww) if k is None else (wi[:k], ww[:k])
        assert np.array_equal(gi, wi), r
        assert gw.dtype == ww.dtype, (r, gw.dtype, ww.dtype)
        assert np.array_equal(gw.view(np.uint8), ww.view(np.uint8)), r


def _sets(n_big=1100):
    rng = np.random.default_rng(5)
    grid = rng.integers(0, 8, size=(n_big, 2)).astype(np.float16)            # 64 points: hundreds of equal distances
    rep = rng.standard_normal((n_big, 64)).astype(np.float16)
    rep[100:300] = rep[7]                                                      # one vector 200 times
    wide = rng.standard_normal((420, 1280)).astype(np.float16)
    wide[10:40] = wide[3]
    return {"grid2": grid, "rep64": rep, "wide1280": wide}


@pytest.mark.parametrize("metric", ["minkowski", "cosine"])
def test_rounds_equal_the_generic_loop(nat, tmp_path, capsys, metric):
    from prograph_amd import distance
    from prograph_amd.graph import KNNGraph
    dist = getattr(distance, metric)
    for name, emb in _sets().items():
        n = emb.shape[0]
        pg = _prograph(tmp_path, n, name)
        capsys.readouterr()
        pg.graph["Embedded"] = list(emb.astype(np.float32))
        for sim in (False, True):
            want = pg.build_graph(representation="Embedded", k=1023, similarity=sim, distance=_generic(dist))
            for k in KS:
                G = pg.build_graph(representation="Embedded", k=k, similarity=sim, distance=dist, output="csr")
                assert isinstance(G, KNNGraph) and tuple(G.idx.shape) == (n, min(k, n - 1)) and G.idx.is_cuda
                _same(G.to_tuples(), want, k)
        sub = np.arange(1, n, 3)
        got = pg.build_graph(idxs=sub, representation="Embedded", k=100, distance=dist)
        _same(got, pg.build_graph(idxs=sub, representation="Embedded", k=100, distance=_generic(dist)))


def test_minkowski_with_an_inf_element(nat, tmp_path, capsys):
    from prograph_amd.distance import minkowski
    emb = np.random.default_rng(8).standard_normal((400, 64)).astype(np.float16)
    emb[17, 5] = np.inf
    emb[200, 9] = -np.inf
    pg = _prograph(tmp_path, 400, "inf")
    capsys.readouterr()
    pg.graph["Embedded"] = list(emb.astype(np.float32))
    for sim in (False, True):
        _same(pg.build_graph(representation="Embedded", k=100, similarity=sim, distance=minkowski),
              pg.build_graph(representation="Embedded", k=100, similarity=sim, distance=_generic(minkowski)))


def test_cosine_row_blocks(nat):
    x = torch.from_numpy(_sets()["rep64"]).to(nat.device())
    xc = nat.cosine_prep(x)
    for sim in (False, True):
        one = nat.cosine_knn(xc, xc, 200, first=1, similarity=sim)
        blocks = nat.cosine_knn(xc, xc, 200, first=1, similarity=sim, rows_per_block=96)
        assert torch.equal(one[0], blocks[0]) and torch.equal(one[1].view(torch.int32), blocks[1].view(torch.int32))


def test_long_sequences_equal_the_generic_loop(nat, tmp_path, capsys):
    from prograph_amd.distance import hamming
    from prograph_amd.graph import KNNGraph
    tok = synth.clustered_tokens(600, 300, seed=12, members=40)
    tok[5] = tok[45]
    tok[100:160] = tok[99]                                                     # sixty copies: ties across rounds
    pg = _prograph(tmp_path, 600, "long", tok=tok)
    capsys.readouterr()
    want = pg.build_graph(k=200, distance=_generic(hamming))
    for k in (64, 100, 200):
        G = pg.build_graph(k=k, output="csr")
        assert isinstance(G, KNNGraph) and tuple(G.idx.shape) == (600, k)
        _same(G.to_tuples(), want, k)


@pytest.mark.parametrize("kind", ["minkowski", "cosine", "long"])
def test_stored_graphs_feed_the_analytics(nat, tmp_path, capsys, kind):
    from prograph_amd import Prograph, distance
    from prograph_amd.utils import save
    rng = np.random.default_rng(21)
    n = 700
    if kind == "long":
        pg = _prograph(tmp_path, n, kind, tok=synth.clustered_tokens(n, 300, seed=4, members=50))
        args = dict(k=100)
    else:
        pg = _prograph(tmp_path, n, kind)
        pg.graph["Embedded"] = list(rng.standard_normal((n, 24)).astype(np.float32))
        args = dict(k=100, representation="Embedded", distance=getattr(distance, kind))
    capsys.readouterr()
    tuples = pg.build_graph(store="E", **args)
    assert pg._device_graph("E") is not None and "E" in pg.csr_graphs
    assert tuple(pg.csr_graphs["E"].idx.shape) == (n, 100)
    pg.graph["T"] = list(tuples)
    assert pg._device_graph("T") is None
    assert np.array_equal(pg.degree("E", boolean_weights=True), pg.degree("T", boolean_weights=True))
    assert np.allclose(pg.degree("E"), pg.degree("T"), rtol=1e-6, atol=0)
    for b in (False, True):
        assert np.allclose(pg.dirichlet("E", boolean_weights=b), pg.dirichlet("T", boolean_weights=b), rtol=1e-6, atol=0)
    ve, vc = pg.local_variance("E"), pg.local_variance("T")
    ok = ~np.isnan(vc)
    assert np.array_equal(np.isnan(ve), np.isnan(vc)) and np.allclose(ve[ok], vc[ok], rtol=1e-9, atol=1e-12)
    assert save(pg, name="bk", directory=str(tmp_path) + "/", graphs="csr")
    back = Prograph(file=str(tmp_path / "bk.pkl"))
    capsys.readouterr()
    g0, g1 = pg.csr_graphs["E"], back.csr_graphs["E"]
    assert type(g0) is type(g1) and torch.equal(g0.idx.cpu(), g1.idx.cpu()) and torch.equal(g0.dist.cpu(), g1.dist.cpu())


def test_minkowski_goldens_at_large_k(nat, tmp_path, capsys):
    """tests/golden/minkowski_f16_bigk.npz: the reference's own output at k = 100 .. 400.  d2 bit for bit.  d64 has
    one pair (row 657, column 715) whose fp16 distance the reference's CPU sum rounds one ulp lower than the dense
    kernel does - the per-pair arithmetic, not the selection (the round path equals selection over the dense block,
    test_rounds_equal_the_generic_loop) - so two neighbours of that row trade places; everything else is bitwise."""
    from prograph_amd.distance import minkowski
    src, g = load_golden("minkowski_f16"), load_golden("minkowski_f16_bigk")
    for name, cases in (("d2", ((100, False, 100), (299, False, 299), (400, False, 299))),
                        ("d64", ((100, False, 100), (100, True, 100)))):
        emb = src[f"{name}_emb"]
        pg = _prograph(tmp_path, emb.shape[0], "g" + name)
        capsys.readouterr()
        pg.graph["Embedded"] = list(emb)
        for k, sim, stored in cases:
            key = f"{name}_knn{stored}" + ("_sim" if sim else "")
            t = pg.build_graph(representation="Embedded", k=k, similarity=sim, distance=minkowski)
            idx, w = np.stack([x[0] for x in t]), np.stack([x[1] for x in t])
            assert w.dtype == np.float16
            wulp = np.abs(w.view(np.int16).astype(np.int64) - g[key + "_w"].view(np.int16).astype(np.int64))
            rows = np.nonzero((idx != g[key + "_idx"]).any(1) | (wulp > 0).any(1))[0]
            assert list(rows) == ([] if name == "d2" else [657]), (name, k, sim, rows[:10])
            assert wulp.max() <= (0 if name == "d2" else 1), (name, k, sim)
