"""
Queries against the dataset on the device: the fused Hamming query kernel (pg_query_knn_hamming) against the staged path
(pg_hamming_dense + pg_f16_knn with first = 0) and an independent torch oracle, search() against build_graph(), the
embedding paths against operator + stable sort, nearest_neighbour, and the reference's Minkowski distances.
Every comparison is exact unless a tolerance is stated.
"""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import load_golden
from prograph_amd import _native as nat, synth

pytestmark = pytest.mark.gpu


def _oracle(X, Y, k):
    """ranks 0..min(k, N)-1 of the stable sort of the Hamming distances (torch broadcast, no project kernel)."""
    dev = nat.device()
    X, Y = torch.as_tensor(X, device=dev), torch.as_tensor(Y, device=dev)
    rows = max(1, (1 << 28) // (X.shape[0] * X.shape[1]))
    idx, w = [], []
    for r0 in range(0, Y.shape[0], rows):
        d = (Y[r0:r0 + rows, None, :] != X[None, :, :]).sum(2)
        s = torch.sort(d, dim=1, stable=True)
        idx.append(s[1][:, :k].cpu().numpy())
        w.append(s[0][:, :k].cpu().numpy())
    return np.concatenate(idx), np.concatenate(w)


def _staged(dp, Y, k):
    idx, w = [], []
    rows = max(64, (1 << 27) // dp.n)
    for r0 in range(0, Y.shape[0], rows):
        q = nat.pack(torch.as_tensor(Y[r0:r0 + rows]), bits=dp.bits, width=dp.l)
        i, d = nat.f16_knn(nat.hamming_dense(dp, q, out_bytes=2), k, first=0)
        idx.append(i.cpu().numpy())
        w.append(d.cpu().numpy().astype(np.int64))
    return np.concatenate(idx), np.concatenate(w)


def _data(q, n, l, bits, seed):
    X = synth.clustered_tokens(n, l, seed=seed)
    if bits == 8:
        X = (X.astype(np.int64) * 11 % 256).astype(np.uint8)                 # byte alphabet
    rng = np.random.default_rng(seed)
    Y = rng.integers(0 if bits == 8 else 1, 256 if bits == 8 else 21, size=(q, l)).astype(np.uint8)
    if n > 3:
        X[n - 2] = X[1]                                                       # duplicated rows far apart
        X[n // 2] = X[1]
    pick = rng.integers(0, n, size=q)
    half = q // 2
    Y[:half] = X[pick[:half]]                                                 # copies of dataset rows
    if q > 2:
        Y[q - 1] = X[1]
        Y[0, :] = X[n - 1]
    return X, Y


CASES = [  # (Q, N, L, bits, k)
    (1, 1, 20, 5, 1), (7, 300, 32, 5, 16), (64, 300, 255, 5, 63), (7, 300, 20, 5, 1023), (1, 300, 64, 5, 300),
    (1000, 20000, 64, 5, 64), (64, 20000, 64, 5, 65), (7, 20000, 20, 5, 200), (1, 20000, 128, 8, 1023),
    (1000, 20000, 128, 8, 16), (1, 200000, 64, 5, 16), (100, 200000, 32, 5, 1), (10000, 200000, 64, 5, 16),
]


@pytest.mark.parametrize("q,n,l,bits,k", CASES)
def test_fused_query_equals_staged_and_oracle(q, n, l, bits, k):
    X, Y = _data(q, n, l, bits, seed=q + n + l + k)
    dp = nat.pack(torch.as_tensor(X), bits=bits)
    qp = nat.pack(torch.as_tensor(Y), bits=bits)
    kk = min(k, n)
    idx, dist = nat.query_knn(qp, dp, kk)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy().astype(np.int64)
    si, sw = _staged(dp, Y, kk)
    assert np.array_equal(idx, si) and np.array_equal(dist, sw)
    sub = slice(None) if q * n <= 2 * 10 ** 7 else slice(0, 64)
    oi, ow = _oracle(X, Y[sub], kk)
    assert np.array_equal(idx[sub], oi) and np.array_equal(dist[sub], ow)
    if n > 3 and q > 2:
        r = min(3, kk)
        assert list(idx[q - 1, :r]) == [1, n // 2, n - 2][:r] and list(dist[q - 1, :r]) == [0] * r
    if k > n:                                                                 # ranks beyond N do not exist
        i2, d2 = nat.query_knn(qp, dp, k)
        assert (i2[:, n:] == -1).all() and (d2[:, n:] == 255).all()


def test_small_workspace_gives_the_same_lists():
    """Fewer pieces than planned (a workspace below pg_query_workspace_bytes) - down to one - change nothing."""
    import ctypes
    X, Y = _data(3, 50000, 64, 5, seed=9)
    dp, qp = nat.pack(torch.as_tensor(X), bits=5), nat.pack(torch.as_tensor(Y), bits=5)
    want = [t.cpu().numpy() for t in nat.query_knn(qp, dp, 32)]
    L = nat.lib()
    full = int(L.pg_query_workspace_bytes(3, 50000, 32))
    assert full > 0
    for wsb in (full // 3, 3 * 32 * 4 * 2, 0):
        ws = torch.empty(max(full, 1), dtype=torch.uint8, device=dp.buf.device)
        idx = torch.empty((3, 32), dtype=torch.int32, device=ws.device)
        dist = torch.empty((3, 32), dtype=torch.uint8, device=ws.device)
        rc = L.pg_query_knn_hamming(nat._ptr(qp.buf), 3, qp.npad, nat._ptr(dp.buf), dp.n, dp.npad, dp.l, 5, 32, None, None,
                                    nat._ptr(idx), nat._ptr(dist), nat._ptr(ws) if wsb else None, wsb, nat._stream())
        assert rc == 0
        assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(dist.cpu().numpy(), want[1])


def _prograph(tmp_path, tok, name):
    from prograph_amd import Prograph
    f = tmp_path / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    return Prograph(file=str(f))


def _ranks_1_on(got, want):
    assert len(got) == len(want)
    for (gi, gw), (wi, ww) in zip(got, want):
        assert np.array_equal(gi[1:], wi) and gw.dtype == ww.dtype and np.array_equal(gw[1:], ww)


def test_search_of_dataset_rows_is_build_graph_hamming(tmp_path, capsys):
    g = load_golden("ref_synthetic_csv")
    pg = _prograph(tmp_path, g["tokens"], "golden")
    capsys.readouterr()
    seqs = list(pg("Sequence"))
    for k in (1, 16, 100):
        _ranks_1_on(pg.search(seqs, k + 1), pg.build_graph(k=k))
    got = pg.search(seqs, 17)
    assert np.array_equal(np.stack([i[1:] for i, _ in got]), g["knn16_idx"])
    _ranks_1_on(pg.search(seqs, 5, similarity=True), pg.build_graph(k=4, similarity=True))
    tok = synth.clustered_tokens(20000, 48, seed=2)
    tok[19000] = tok[3]
    pg = _prograph(tmp_path, tok, "synth")
    capsys.readouterr()
    for k in (16, 100):
        _ranks_1_on(pg.search(pg.tokenized, k + 1), pg.build_graph(k=k))


@pytest.mark.parametrize("dist_name", ["minkowski", "cosine"])
def test_search_of_dataset_rows_is_build_graph_embeddings(tmp_path, capsys, dist_name):
    from prograph_amd.distance import cosine, minkowski
    distance = {"minkowski": minkowski, "cosine": cosine}[dist_name]
    g = load_golden("minkowski_f16")
    for name in ("d64", "d1280"):
        emb = g[f"{name}_emb"]
        pg = _prograph(tmp_path, synth.clustered_tokens(emb.shape[0], 8, seed=3), name)
        capsys.readouterr()
        pg.graph["Embedded"] = list(emb)
        for k in (1, 16, 100):
            for sim in (False, True):
                _ranks_1_on(pg.search(emb, k + 1, distance=distance, representation="Embedded", similarity=sim),
                            pg.build_graph(k=k, distance=distance, representation="Embedded", similarity=sim))
        if distance is minkowski:                                 # the fused kernel (many queries) gives the same lists
            Y = np.tile(emb, (8 if name == "d1280" else 5, 1))
            G = pg.search(Y, 20, distance=minkowski, representation="Embedded", output="csr")
            S = pg.search(Y[:7], 20, distance=minkowski, representation="Embedded", output="csr")
            assert Y.shape[0] >= pg._MINK_STAGED_ROWS
            assert torch.equal(G.idx[:7], S.idx) and torch.equal(G.dist[:7], S.dist)


@pytest.mark.parametrize("dist_name", ["minkowski", "cosine"])
def test_embedding_queries_against_operator(tmp_path, capsys, dist_name):
    from prograph_amd.distance import cosine, minkowski
    distance = {"minkowski": minkowski, "cosine": cosine}[dist_name]
    rng = np.random.default_rng(5)
    emb = rng.standard_normal((3000, 64)).astype(np.float16)
    emb[2500] = emb[10]
    pg = _prograph(tmp_path, synth.clustered_tokens(3000, 8, seed=4), "e")
    capsys.readouterr()
    pg.graph["Embedded"] = list(emb)
    dev = nat.device()
    X = torch.as_tensor(emb, device=dev)
    for Y in (np.concatenate([emb[[10, 7]], rng.standard_normal((5, 64)).astype(np.float16)]),
              rng.standard_normal((3, 40)).astype(np.float32)):              # shorter: zero padded
        for sim in (False, True):
            for k in (1, 16, 70):
                got = pg.search(Y, k, distance=distance, representation="Embedded", similarity=sim)
                Yd = torch.as_tensor(Y, dtype=torch.float16, device=dev)
                s = torch.sort(distance(X, Yd, similarity=sim), dim=1, stable=True, descending=sim)
                wi, ww = s[1][:, :k].cpu().numpy(), s[0][:, :k].cpu().numpy()
                for (gi, gw), a, b in zip(got, wi, ww):
                    assert np.array_equal(gi, a) and gw.dtype == b.dtype and np.array_equal(gw, b)
    got = pg.search(emb[10], 2, distance=distance, representation="Embedded")
    assert list(got[0][0]) == [10, 2500]


def test_long_sequences_against_operator(tmp_path, capsys):
    from prograph_amd.distance import hamming
    tok = synth.clustered_tokens(600, 300, seed=6, members=30)
    tok[550] = tok[4]
    pg = _prograph(tmp_path, tok, "long")
    capsys.readouterr()
    rng = np.random.default_rng(2)
    Y = np.concatenate([tok[[4, 9]], rng.integers(1, 21, size=(3, 300)).astype(np.uint8)])
    Y2 = np.concatenate([Y, np.ones((5, 40), dtype=np.uint8)], axis=1)          # longer than the dataset
    for Q in (Y, Y2):
        for k in (1, 65, 600):
            got = pg.search(Q, k)
            d = hamming(torch.as_tensor(tok, device=nat.device()), torch.as_tensor(Q, device=nat.device()))
            s = torch.sort(d, dim=1, stable=True)
            for (gi, gw), a, b in zip(got, s[1][:, :k].cpu().numpy(), s[0][:, :k].cpu().numpy()):
                assert np.array_equal(gi, a) and gw.dtype == b.dtype and np.array_equal(gw, b)
    assert list(pg.search(tok[4], 2)[0][0]) == [4, 550]


def test_nearest_neighbour(tmp_path, capsys):
    tok = synth.clustered_tokens(5000, 40, seed=8)
    tok[4000] = tok[12]
    pg = _prograph(tmp_path, tok, "nn")
    capsys.readouterr()
    seqs = list(pg("Sequence"))
    rows, d = pg.nearest_neighbour(seqs[4000])
    assert list(rows.index) == [pg.graph.index[12]] and d == 0
    m = list(seqs[77])
    m[3] = "W" if m[3] != "W" else "Y"
    m[20] = "W" if m[20] != "W" else "Y"
    m = "".join(m)
    rows, d = pg.nearest_neighbour(m)
    want = _oracle(pg.tokenized, pg.tokenize([m]), 1)
    assert list(rows.index) == [pg.graph.index[int(want[0][0, 0])]] and d == want[1][0, 0] <= 2
    rows, d = pg.nearest_neighbour([m, seqs[5]])
    assert len(rows) == 2 and d == 0


def test_reference_minkowski_distances():
    """tests/golden/minkowski_f16.npz: the reference operator's distances of the first 64 rows against all rows; their
    stable sort is what search() must return (d1280: the accumulation order differs from the reference's, so weights
    within one fp16 ulp and >= 98 % of the rows identical)."""
    import tempfile
    from prograph_amd import Prograph
    from prograph_amd.distance import minkowski
    g = load_golden("minkowski_f16")
    for name in ("d2", "d64", "d1280"):
        emb, ref = g[f"{name}_emb"], g[f"{name}_dist64"].astype(np.float32)
        with tempfile.TemporaryDirectory() as tmp:
            f = f"{tmp}/{name}.csv"
            pd.DataFrame({"Sequence": synth.tokens_to_strings(synth.clustered_tokens(emb.shape[0], 8, seed=3)),
                          "Fitness": np.zeros(emb.shape[0])}).to_csv(f)
            pg = Prograph(file=f)
        pg.graph["Embedded"] = list(emb)
        # (d1280: k as in test_minkowski_f16_against_the_reference; over 100 ranks a one-ulp move reorders more rows)
        for k in ((1, 5, 16) if name == "d1280" else (1, 5, 16, 100)):
            G = pg.search(emb[:64], k, distance=minkowski, representation="Embedded", output="csr")
            idx, w = G.idx.cpu().numpy(), G.dist.cpu().numpy()
            order = np.argsort(ref, axis=1, kind="stable")[:, :k]
            wref = np.take_along_axis(g[f"{name}_dist64"], order, 1)
            ulp = np.abs(w.view(np.int16).astype(np.int64) - wref.view(np.int16).astype(np.int64))
            if name == "d1280":
                assert ulp.max() <= 1 and (idx == order).all(1).mean() >= 0.98
            else:
                assert ulp.max() == 0 and np.array_equal(idx, order)
