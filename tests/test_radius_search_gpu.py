"""
Radius (eps) search of queries on the device: the fused Hamming kernel pair (pg_query_eps_count / _fill) against a torch
oracle that uses no project kernel, search(eps=) against build_graph(eps=), long sequences, and the Minkowski / cosine
paths (keep-zero mode of the eps entries) against selection over the project's own dense blocks, which the fused kernels
equal bit for bit.  Every comparison is exact: indices, weights, dtypes and order.
"""
import operator

import numpy as np
import pandas as pd
import pytest
import torch

from prograph_amd import _native as nat, synth
from test_search_gpu import _data

pytestmark = pytest.mark.gpu

COMPS = {nat.CMP_LE: operator.le, nat.CMP_LT: operator.lt, nat.CMP_EQ: operator.eq, nat.CMP_GE: operator.ge,
         nat.CMP_GT: operator.gt}
EPS = (0, 1, 2, 4, 1.5)


def _data_eps(q, n, l, bits, seed):
    """test_search_gpu._data (random queries, copies of dataset rows, duplicated dataset rows) with the third quarter of
    the queries replaced by dataset rows with 1-3 substitutions.  At (Q, N, L) = (200, 20 000, 64), seed 7 (numpy, on the
    CPU): eps <= 2 gives 3 134 entries, 65 empty rows, 102 rows with a d = 0 hit, a longest row of 103; eps <= 4 a longest
    row of 259; d >= 60 has 3 110 372 entries."""
    X, Y = _data(q, n, l, bits, seed)
    rng = np.random.default_rng(seed + 1)
    rows = rng.integers(0, n, size=q // 4)
    for i, r in enumerate(rows):
        y = X[r].copy()
        pos = rng.choice(l, size=int(rng.integers(1, 4)), replace=False)
        y[pos] = rng.integers(0 if bits == 8 else 1, 256 if bits == 8 else 21, size=len(pos))
        Y[q // 2 + i] = y
    return X, Y


def _distances(X, Y):
    """(Q, N) int64 Hamming distances on the device: a torch broadcast, no project kernel."""
    dev = nat.device()
    X, Y = torch.as_tensor(X, device=dev), torch.as_tensor(Y, device=dev)
    rows = max(1, (1 << 28) // (X.shape[0] * X.shape[1]))
    return torch.cat([(Y[r0:r0 + rows, None, :] != X[None, :, :]).sum(2) for r0 in range(0, Y.shape[0], rows)])


def _where(keep, values):
    """(indptr, indices, weights) of torch.where(keep): rows ascending, columns ascending within a row."""
    r, c = torch.where(keep)
    indptr = torch.zeros(keep.shape[0] + 1, dtype=torch.int64, device=keep.device)
    indptr[1:] = torch.cumsum(keep.sum(1), 0)
    return indptr, c, values[r, c]


def _equal(got, want, wdtype):
    indptr, indices, weights = got
    assert indptr.dtype == torch.int64 and indices.dtype == torch.int32 and weights.dtype == wdtype
    assert torch.equal(indptr, want[0]), "indptr"
    assert torch.equal(indices.to(torch.int64), want[1]), "indices"
    assert torch.equal(weights, want[2].to(wdtype)), "weights"


WIDTHS = [(20, 5), (32, 5), (64, 5), (100, 5), (200, 5), (64, 8), (128, 8)]
SHAPES = [(1, 1), (7, 255), (8, 257), (9, 5000), (200, 5000), (1000, 257), (1, 50000), (200, 50000)]


# every shape at every width, and the largest shape at one width per alphabet
CASES = [(q, n, l, bits) for q, n in SHAPES for l, bits in WIDTHS] + [(1000, 50000, 64, 5), (1000, 50000, 128, 8)]


@pytest.mark.parametrize("q,n,l,bits", CASES)
def test_query_eps_against_torch(q, n, l, bits):
    X, Y = _data_eps(q, n, l, bits, seed=q + n + l)
    dp = nat.pack(torch.as_tensor(X), bits=bits)
    qp = nat.pack(torch.as_tensor(Y), bits=bits)
    d = _distances(X, Y)
    for cmp, comp in COMPS.items():
        for eps in EPS:
            _equal(nat.query_eps(qp, dp, cmp, eps), _where(comp(d, eps), d), torch.uint8)


def test_piece_count_does_not_change_the_output():
    for q, n, l in ((3, 50000, 64), (9, 20000, 32), (200, 5000, 100)):
        X, Y = _data_eps(q, n, l, 5, seed=3)
        dp, qp = nat.pack(torch.as_tensor(X), bits=5), nat.pack(torch.as_tensor(Y), bits=5)
        planned = int(nat.lib().pg_query_eps_segments(q, n)) // 4
        assert planned > 2
        for cmp, eps in ((nat.CMP_LE, 2), (nat.CMP_GE, l - 6)):
            want = nat.query_eps(qp, dp, cmp, eps)
            assert want[1].numel() > 0
            for pieces in (1, 2, planned // 2, planned, (n + 127) // 128):
                got = nat.query_eps(qp, dp, cmp, eps, pieces=pieces)
                assert all(torch.equal(a, b) for a, b in zip(got, want)), pieces
        with pytest.raises(RuntimeError):
            nat.query_eps(qp, dp, nat.CMP_LE, 2, pieces=(n + 127) // 128 + 1)


def test_rows_empty_with_zero_hits_and_beyond_the_slot_cap():
    X, Y = _data_eps(200, 20000, 64, 5, seed=7)
    dp, qp = nat.pack(torch.as_tensor(X), bits=5), nat.pack(torch.as_tensor(Y), bits=5)
    d = _distances(X, Y)
    for eps in (2, 4):
        want = _where(d <= eps, d)
        _equal(nat.query_eps(qp, dp, nat.CMP_LE, eps), want, torch.uint8)
        counts = (want[0][1:] - want[0][:-1]).cpu().numpy()
        assert (counts == 0).sum() > 0                                     # rows without a hit
        assert ((d == 0).sum(1) > 0).sum().item() > 0                      # rows with a d = 0 hit, which is kept
        if eps == 4:
            assert counts.max() > 256                                      # beyond the default cap of the slot paths
    # a large result comes back complete and ordered
    got = nat.query_eps(qp, dp, nat.CMP_GE, 60)
    assert got[1].numel() > 3_000_000
    _equal(got, _where(d >= 60, d), torch.uint8)


def _prograph(tmp_path, tok, name):
    from prograph_amd import Prograph
    f = tmp_path / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    return Prograph(file=str(f))


def test_search_of_dataset_rows_is_build_graph_plus_the_duplicates(tmp_path, capsys):
    tok = synth.clustered_tokens(20000, 48, seed=2)
    tok[19000] = tok[3]
    tok[7] = tok[3]
    pg = _prograph(tmp_path, tok, "synth")
    capsys.readouterr()
    rows = np.array([3, 7, 19000, 11, 4000, 19999, 0])
    same = {r: set(np.nonzero((tok == tok[r]).all(1))[0]) for r in rows}
    assert same[3] == {3, 7, 19000}
    for e, sim in ((1, False), (2, False), (3, True), (2.5, False)):
        graph = pg.build_graph(eps=e, similarity=sim)
        for inp in (tok[rows], [pg("Sequence")[r] for r in rows]):
            got = pg.search(inp, eps=e, similarity=sim)
            for r, (gi, gw) in zip(rows, got):
                zero = gw == (1 if sim else 0)
                assert set(gi[zero]) == same[r]                            # the removed entries: the row and its duplicates
                wi, ww = graph[r]
                assert np.array_equal(gi[~zero], wi)
                if len(wi):
                    assert gw.dtype == ww.dtype and np.array_equal(gw[~zero], ww)
    G = pg.search(tok[rows], eps=2, output="csr")
    assert G.nrows == len(rows) and G.ncols == len(tok) and G.weights.dtype == torch.uint8 and G.indptr.is_cuda
    for (gi, gw), (ti, tw) in zip(G.to_tuples(), pg.search(tok[rows], eps=2)):
        assert np.array_equal(gi, ti) and np.array_equal(gw, tw)
    # neighbourhood of a string that is not in the dataset
    s = pg("Sequence")[11]
    mutated = ("W" if s[0] != "W" else "Y") + s[1:]
    assert mutated not in pg.seq_idxs
    d = (pg.tokenize([mutated]) != tok).sum(1)
    assert list(pg.neighbourhood(mutated, 2).index) == list(pg.graph.index[d <= 2]) and (d <= 2).sum() >= 1


@pytest.mark.parametrize("l", [300, 600])
def test_long_sequences_against_torch(tmp_path, capsys, l):
    tok = synth.clustered_tokens(600, l, seed=6, members=30)
    tok[550] = tok[4]
    pg = _prograph(tmp_path, tok, "long")
    capsys.readouterr()
    rng = np.random.default_rng(2)
    Y = np.concatenate([tok[[4, 9]], rng.integers(1, 21, size=(3, l)).astype(np.uint8)])
    Y[1, 5] = Y[1, 5] % 20 + 1
    Y2 = np.concatenate([Y, np.ones((5, 40), dtype=np.uint8)], axis=1)          # longer than the dataset
    for Q in (Y, Y2):
        Xp = np.zeros((len(tok), Q.shape[1]), dtype=np.uint8)
        Xp[:, :l] = tok
        d = _distances(Xp, Q)
        for comp in COMPS.values():
            for eps in (0, 3, l // 4, 2.5):
                G = pg.search(Q, eps=eps, comp=comp, output="csr")
                _equal((G.indptr, G.indices, G.weights), _where(comp(d, eps), d), torch.int16)
    got = pg.search(tok[4], eps=0)
    assert list(got[0][0]) == [4, 550] and got[0][1].dtype == np.int64 and list(got[0][1]) == [0, 0]
    sim = pg.search(tok[4], eps=0, similarity=True)
    assert sim[0][1].dtype == np.float32 and list(sim[0][1]) == [1, 1]


def _embedded(tmp_path, capsys, emb, name):
    pg = _prograph(tmp_path, synth.clustered_tokens(emb.shape[0], 8, seed=4), name)
    capsys.readouterr()
    pg.graph["Embedded"] = list(emb)
    return pg


@pytest.mark.parametrize("d", [64, 200])
def test_minkowski_staged_equals_fused_equals_dense_selection(tmp_path, capsys, d):
    from prograph_amd.distance import minkowski
    rng = np.random.default_rng(5)
    emb = (rng.standard_normal((3000, d)) * 0.5).astype(np.float16)
    emb[2500] = emb[10]
    pg = _embedded(tmp_path, capsys, emb, "m")
    few = np.concatenate([emb[[10, 7]], (rng.standard_normal((5, d)) * 0.5).astype(np.float16)])
    many = np.concatenate([few, emb, emb[::-1][:1200]])
    assert len(few) < pg._MINK_STAGED_ROWS <= len(many)
    dev = nat.device()
    xp = nat.pack_f16(torch.as_tensor(emb, device=dev))
    yp = nat.pack_f16(torch.as_tensor(many, device=dev))
    scale = float(np.sqrt(d) * 0.5)
    for sim in (False, True):
        block = nat.minkowski_dense(xp, yp, similarity=sim)
        for comp in COMPS.values():
            for eps in (0, 0.6 * scale, 1.2 * scale):
                e = 1 / (1 + eps) if sim else eps
                e16 = float(np.float16(e))
                want = _where(comp(e16, block) if sim else comp(block, e16), block)
                G = pg.search(many, eps=eps, comp=comp, distance=minkowski, representation="Embedded", similarity=sim,
                              output="csr")                                  # the fused kernels
                _equal((G.indptr, G.indices, G.weights), want, torch.float16)
                S = pg.search(few, eps=eps, comp=comp, distance=minkowski, representation="Embedded", similarity=sim,
                              output="csr")                                  # dense block + selection
                n7 = int(G.indptr[len(few)].item())
                assert torch.equal(S.indptr, G.indptr[:len(few) + 1])
                assert torch.equal(S.indices, G.indices[:n7]) and torch.equal(S.weights, G.weights[:n7])
                assert S.weights.dtype == torch.float16
    got = pg.search(emb[10], eps=0, distance=minkowski, representation="Embedded")
    assert list(got[0][0]) == [10, 2500] and got[0][1].dtype == np.float16 and list(got[0][1]) == [0, 0]   # d = 0 kept
    got = pg.search(emb[10], eps=0, distance=minkowski, representation="Embedded", similarity=True)
    assert list(got[0][0]) == [10, 2500] and list(got[0][1]) == [1, 1]


def test_cosine_fused_equals_dense_selection(tmp_path, capsys):
    from prograph_amd.distance import cosine
    rng = np.random.default_rng(9)
    emb = rng.standard_normal((3000, 64)).astype(np.float16)
    emb[2500] = emb[10]
    emb[77] = 0                                                               # a zero vector: d = 1 to everything
    pg = _embedded(tmp_path, capsys, emb, "c")
    Y = np.concatenate([emb[[10, 7, 77]], rng.standard_normal((6, 64)).astype(np.float16),
                        np.zeros((1, 64), dtype=np.float16), emb[:300]])
    dev = nat.device()
    xc, yc = nat.cosine_prep(torch.as_tensor(emb, device=dev)), nat.cosine_prep(torch.as_tensor(Y, device=dev))
    for sim in (False, True):
        block = nat.cosine_dense(xc, yc, similarity=sim)
        for comp in COMPS.values():
            for eps in (0, 0.7, 1, 1.25):
                e = float(np.float32(1 / (1 + eps) if sim else eps))
                want = _where(comp(e, block) if sim else comp(block, e), block)
                G = pg.search(Y, eps=eps, comp=comp, distance=cosine, representation="Embedded", similarity=sim, output="csr")
                assert G.final and G.nrows == len(Y) and G.ncols == len(emb)
                _equal((G.indptr, G.indices, G.weights), want, torch.float32)
    got = pg.search(emb[10], eps=0, distance=cosine, representation="Embedded")
    assert list(got[0][0]) == [10, 2500] and got[0][1].dtype == np.float32 and list(got[0][1]) == [0, 0]   # d = 0 kept
    got = pg.search(emb[77], eps=1, comp=operator.eq, distance=cosine, representation="Embedded")
    assert len(got[0][0]) == len(emb) and set(got[0][1]) == {1.0}            # the zero vector: d = 1 everywhere
    # an operand with an inf: the generic loop still answers, from the operator's own values
    bad = emb[:4].copy()
    bad[1, 3] = np.inf
    got = pg.search(bad, eps=0.7, distance=cosine, representation="Embedded")
    dd = cosine(torch.as_tensor(emb, device=dev), torch.as_tensor(bad, device=dev))
    for (gi, gw), row in zip(got, dd):
        j = torch.where(row <= 0.7)[0]
        assert np.array_equal(gi, j.cpu().numpy()) and np.array_equal(gw, row[j].cpu().numpy())
    assert 0 in got[0][0] and 2 in got[2][0]


def test_eps_entries_without_keep_zero_are_unchanged(tmp_path, capsys):
    from prograph_amd.distance import cosine, minkowski
    rng = np.random.default_rng(11)
    emb = (rng.standard_normal((2000, 64)) * 0.5).astype(np.float16)
    emb[1500] = emb[10]
    pg = _embedded(tmp_path, capsys, emb, "u")
    dev = nat.device()
    X = torch.as_tensor(emb, device=dev)
    xp = nat.pack_f16(X)
    # fp16 selection and fused Minkowski without the flag: the self-graph of build_graph, d = 0 excluded
    block = nat.minkowski_dense(xp, xp)
    e16 = float(np.float16(3.0))
    want = _where((block <= e16) & (block > 0), block)
    _equal(nat.f16_eps(block, nat.CMP_LE, 3.0), want, torch.float16)
    _equal(nat.minkowski_eps(xp, xp, nat.CMP_LE, 3.0), want, torch.float16)
    G = pg.build_graph(eps=3.0, distance=minkowski, representation="Embedded", output="csr")
    _equal((G.indptr, G.indices, G.weights), want, torch.float16)
    assert 10 not in G.to_tuples()[10][0] and 1500 not in G.to_tuples()[10][0]
    kept = nat.f16_eps(block, nat.CMP_LE, 3.0, keep_zero=True)
    assert kept[1].numel() == want[1].numel() + int((block == 0).sum().item())
    # cosine
    xc = nat.cosine_prep(X)
    cb = nat.cosine_dense(xc, xc)
    e32 = float(np.float32(0.8))
    want = _where((cb <= e32) & (cb > 0), cb)
    _equal(nat.cosine_eps(xc, xc, nat.CMP_LE, 0.8), want, torch.float32)
    G = pg.build_graph(eps=0.8, distance=cosine, representation="Embedded", output="csr")
    _equal((G.indptr, G.indices, G.weights), want, torch.float32)
    # the Hamming graph entries are untouched: the constructor's eps = 1 graph against the torch oracle, d = 0 excluded
    tok = pg.tokenized
    d = _distances(tok, tok)
    G = pg.build_graph(eps=1, output="csr")
    _equal((G.indptr, G.indices, G.weights), _where((d <= 1) & (d > 0), d), torch.uint8)
