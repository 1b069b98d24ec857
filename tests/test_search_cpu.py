"""
Host logic of `Prograph.search` / `nearest_neighbour` (queries that need not be in the dataset) with the CPU stand-in
of tests/fake_native.py, plus fakes of the query entries defined here, and the argument checks of the new C entries
(refused on the host, before any launch: no GPU needed).
"""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import fake_native
from oracle import prograph_oracle as O
from prograph_amd import _native, synth


def _fake_query_knn(qp, dp, k):
    l = max(qp.l, dp.l)
    d = O.hamming(fake_native._pad_to(dp.tok, l), fake_native._pad_to(qp.tok, l))
    s = torch.sort(d, dim=1, stable=True)
    idx = torch.full((qp.n, k), -1, dtype=torch.int32)
    dist = torch.full((qp.n, k), 255, dtype=torch.uint8)
    kk = min(k, dp.n)
    idx[:, :kk] = s[1][:, :kk].to(torch.int32)
    dist[:, :kk] = s[0][:, :kk].to(torch.uint8)
    return idx, dist


def _fake_pack_bytes(raw, lut, bits=_native.BITS_5, want_tokens=True, check=True):
    tok = np.asarray(lut)[np.asarray(raw)]
    return fake_native.FakePlanes(tok, bits), (torch.from_numpy(tok.astype(np.uint8)) if want_tokens else None)


@pytest.fixture
def fake(monkeypatch):
    fake_native.install(monkeypatch)
    calls = []
    monkeypatch.setattr(_native, "query_knn", lambda qp, dp, k: (calls.append(("query_knn", qp.l, dp.l)), _fake_query_knn(qp, dp, k))[1])
    monkeypatch.setattr(_native, "pack_bytes", lambda *a, **kw: (calls.append(("pack_bytes",)), _fake_pack_bytes(*a, **kw))[1])
    return calls


def _prograph(tmp_path, tok, name="s"):
    from prograph_amd import Prograph
    f = tmp_path / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    return Prograph(file=str(f))


def _want(X, Y, k, sim=False):
    """ranks 0..min(k, N)-1 of the stable sort of the padded Hamming distances (numpy)."""
    l = max(X.shape[1], Y.shape[1])
    Xp, Yp = fake_native._pad_to(X, l), fake_native._pad_to(Y, l)
    d = (Yp[:, None, :] != Xp[None, :, :]).sum(2)
    order = np.argsort(d, axis=1, kind="stable")[:, :min(k, len(X))]
    w = np.take_along_axis(d, order, 1)
    return order, ((1 / (1 + w)).astype(np.float32) if sim else w)


def _same(got, want):
    idx, w = want
    assert len(got) == len(idx)
    for (gi, gw), wi, ww in zip(got, idx, w):
        assert np.array_equal(gi, wi) and gw.dtype == ww.dtype and np.array_equal(gw, ww)


@pytest.fixture
def pg(fake, tmp_path, capsys):
    tok = synth.clustered_tokens(120, 12, seed=4, members=20)
    tok[77] = tok[5]                                        # a duplicated row
    tok[100] = tok[5]
    p = _prograph(tmp_path, tok)
    capsys.readouterr()
    return p


def test_strings_tokens_and_shapes(pg, fake):
    X = pg.tokenized
    rng = np.random.default_rng(1)
    seqs = [pg("Sequence")[5], pg("Sequence")[9], "ACDXXQ", "".join(rng.choice(list("ACDEFGHIKL"), 12))]
    T = pg.tokenize(seqs)
    for k in (1, 3, 16, 120, 500):
        want = _want(X, T, k)
        _same(pg.search(seqs, k), want)
        _same(pg.search(T, k), want)
    assert ("pack_bytes",) in fake
    _same(pg.search(seqs[0], 4), _want(X, T[:1], 4))                   # one string = a list of one
    _same(pg.search(T[1], 4), _want(X, T[1:2], 4))                     # 1-D tokens = one query
    hit = pg.search(seqs[0], 3)[0]
    assert hit[0][0] == 5 and hit[1][0] == 0 and list(hit[0][:3]) == [5, 77, 100]   # rank 0 kept, lowest index first
    _same(pg.search(seqs, 6, similarity=True), _want(X, T, 6, sim=True))


def test_shorter_and_longer_queries(pg, fake):
    X = pg.tokenized
    short = ["ACD", "K"]
    long_ = [pg("Sequence")[3] + "ACDEF", "A" * 30]
    for q in (short, long_):
        T = pg.tokenize(q)
        _same(pg.search(q, 8), _want(X, T, 8))
        _same(pg.search(T, 8), _want(X, T, 8))
    # a longer query packs the dataset at the query's width for that call: its extra positions count against zeros
    assert any(c[0] == "query_knn" and c[1] == c[2] == 30 for c in fake)
    assert pg.search(long_[0], 1)[0][1][0] == 5


def test_argument_errors(pg):
    with pytest.raises(ValueError):
        pg.search("ACD", 0)
    with pytest.raises(TypeError):
        pg.search("ACD", 2.0)
    with pytest.raises(TypeError):
        pg.search("ACD", 1.5)
    for empty in ([], np.zeros((0, 12), dtype=np.int64)):
        with pytest.raises(ValueError):
            pg.search(empty, 3)


def test_csr_output_keeps_rank_zero(pg):
    from prograph_amd.graph import KNNGraph
    T = pg.tokenize(["ACDEFGHIKLMN", pg("Sequence")[7]])
    for k in (5, 200):
        G = pg.search(T, k, output="csr")
        assert isinstance(G, KNNGraph) and G.first == 0 and G.nrows == 2 and G.ncols == len(pg)
        tup = pg.search(T, k)
        for (gi, gw), (ti, tw) in zip(G.to_tuples(), tup):
            assert np.array_equal(gi, ti) and np.array_equal(gw, tw)
        C = G.as_csr()
        assert C.nrows == 2 and C.nnz == 2 * min(k, len(pg))


def test_container_cut_by_first():
    from prograph_amd.graph import KNNGraph
    n, k = 5, 8
    idx = torch.arange(3 * k, dtype=torch.int32).reshape(3, k)
    dist = torch.zeros((3, k), dtype=torch.uint8)
    assert KNNGraph(idx, dist, n).host()[0].shape == (3, n - 1)                # self-graph: ranks 1..N-1
    assert KNNGraph(idx, dist, n, first=0).host()[0].shape == (3, n)           # query result: min(k, N) ranks
    assert KNNGraph(idx, dist, n, first=0).as_csr().nnz == 3 * n
    assert KNNGraph(idx, dist, 20, first=0).host()[0].shape == (3, k)


def test_generic_distance_against_numpy(pg):
    X = pg.tokenized.astype(np.float32)
    T = pg.tokenize(["ACDEFGHIKL", "MNPQ", pg("Sequence")[11]])

    def l1(A, B, similarity=False):
        A, B = A.to(torch.float32), B.to(torch.float32)
        B = torch.nn.functional.pad(B, (0, A.shape[1] - B.shape[1]))
        d = (B[:, None, :] - A[None, :, :]).abs().sum(2)
        return 1 / (1 + d) if similarity else d

    Tp = fake_native._pad_to(T, X.shape[1]).astype(np.float32)
    d = np.abs(Tp[:, None, :] - X[None]).sum(2)
    for sim in (False, True):
        got = pg.search(T, 7, distance=l1, similarity=sim)
        vals = (1 / (1 + d)).astype(np.float32) if sim else d
        order = np.argsort(-vals if sim else vals, axis=1, kind="stable")[:, :7]
        for (gi, gw), wi, wrow in zip(got, order, vals):
            assert np.array_equal(gi, wi) and np.array_equal(gw, wrow[wi])
    G = pg.search(T, 7, distance=l1, output="csr")
    assert G.first == 0 and G.host()[0].shape == (3, 7)


def test_nearest_neighbour(pg):
    seqs = pg("Sequence")
    rows, d = pg.nearest_neighbour(seqs[100])                  # rows 5, 77 and 100 are equal: the lowest index wins
    assert list(rows.index) == [pg.graph.index[5]] and d == 0
    mutated = "W" + seqs[9][1:] if seqs[9][0] != "W" else "Y" + seqs[9][1:]
    rows, d = pg.nearest_neighbour([mutated, seqs[9]], batch_size=2)
    want = _want(pg.tokenized, pg.tokenize([mutated, seqs[9]]), 1)
    assert list(rows.index) == [pg.graph.index[int(i)] for i in want[0][:, 0]]
    assert d == 0 and want[1][0, 0] <= 1


# ---- the C entries: declared, bound, exported, and refused on the host before any launch
def test_query_entries_validate_arguments():
    L = _native.lib()
    for name in ("pg_query_knn_hamming", "pg_query_workspace_bytes"):
        assert name in _native.SYMBOLS and hasattr(L, name)
    p = ctypes.c_void_p(256)          # never dereferenced: every call below is refused on the host
    BAD, LONG, MANY = -1, -2, -3

    def call(qp=p, nq=10, qnpad=256, dbp=p, ndb=300, dbnpad=512, l=64, bits=5, k=8, floor=None, last=None, idx=p, dist=p,
             ws=p, wsb=1 << 20):
        return L.pg_query_knn_hamming(qp, nq, qnpad, dbp, ndb, dbnpad, l, bits, k, floor, last, idx, dist, ws, wsb, None)

    assert call(qp=None) == BAD and b"pg_query_knn_hamming" in L.pg_last_error()
    assert call(dbp=None) == BAD and call(idx=None) == BAD and call(dist=None) == BAD
    assert call(k=0) == BAD and call(k=65) == BAD and call(k=-3) == BAD
    assert call(bits=6) == BAD and call(bits=0) == BAD
    assert call(nq=0) == BAD and call(ndb=0) == BAD
    assert call(dbnpad=300) == BAD and call(qnpad=5) == BAD
    assert call(l=300) == LONG and call(l=160, bits=8) == LONG
    assert call(ndb=1 << 24, dbnpad=1 << 24) == MANY
    assert L.pg_query_workspace_bytes(0, 300, 8) == 0 and L.pg_query_workspace_bytes(1, 300, 65) == 0
    # one query against 200 000 rows is split into pieces (a list of k keys each), 10^5 queries are not
    assert L.pg_query_workspace_bytes(1, 200000, 16) >= 64 * 16 * 4
    assert L.pg_query_workspace_bytes(100000, 200000, 16) == 0
    assert L.pg_query_workspace_bytes(1, 200000, 64) <= 8192 * 4                 # the merge's LDS bound
