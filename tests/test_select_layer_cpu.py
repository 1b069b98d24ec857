"""
The selection layer's host side without a GPU: `_native.cat_csr` on hand-made parts, and the block helper of
prograph.py (`_staged` / `_select_blocks` / `_block_rows`) through the CPU stand-ins - a graph or search cut into
several row blocks is the graph or search of one block, on every staged route and for both kinds of block (fp16, int32).
"""
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import fake_aln_native
import fake_lev_long_native
import fake_lev_native
import fake_long_native
import fake_native
import fake_sub_native
import lev_testdata as LT
from prograph_amd import _native, synth
from prograph_amd.distance import alignment, levenshtein, local_alignment, substitution


def _part(counts, seed):
    rng = np.random.default_rng(seed)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    nnz = int(indptr[-1])
    return (torch.from_numpy(indptr), torch.from_numpy(rng.integers(0, 50, nnz).astype(np.int32)),
            torch.from_numpy(rng.uniform(0, 1, nnz).astype(np.float16)))


def test_cat_csr():
    one = _part([2, 0, 1], 0)
    got = _native.cat_csr([one])
    assert all(g is p for g, p in zip(got, one))                        # one part: the same tensor objects
    parts = [_part([3, 1], 1), _part([0, 0], 2), _part([2, 0, 4], 3)]  # 2 rows, 2 rows without entries, 3 rows
    before = [[t.clone() for t in p] for p in parts]
    indptr, indices, weights = _native.cat_csr(parts)
    counts = np.concatenate([np.diff(p[0].numpy()) for p in parts])
    assert indptr.dtype == torch.int64 and indices.dtype == torch.int32 and weights.dtype == torch.float16
    assert np.array_equal(indptr.numpy(), np.concatenate([[0], np.cumsum(counts)]))
    assert np.array_equal(indices.numpy(), np.concatenate([p[1].numpy() for p in parts]))
    assert np.array_equal(weights.numpy().view(np.uint16), np.concatenate([p[2].numpy() for p in parts]).view(np.uint16))
    assert indptr.numel() == 8 and int(indptr[-1]) == 10 == indices.numel() == weights.numel()
    assert all(torch.equal(t, b) for p, q in zip(parts, before) for t, b in zip(p, q))   # the parts are left alone


def _prograph(tmp_path, tok):
    from prograph_amd import Prograph
    f = tmp_path / "s.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    return Prograph(file=str(f))


def _same(a, b):
    """two graphs as csr containers: the same arrays, dtypes and shapes"""
    assert type(a) is type(b)
    names = ("indptr", "indices", "weights") if hasattr(a, "indptr") else ("idx", "dist")
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), name
    ta, tb = a.to_tuples(), b.to_tuples()
    assert len(ta) == len(tb)
    for (ai, aw), (bi, bw) in zip(ta, tb):
        assert np.array_equal(ai, bi) and aw.dtype == bw.dtype and np.array_equal(aw, bw)


def _blockwise_equals_whole(monkeypatch, P, calls, elems, min_blocks, kind="f16"):
    """calls: name -> thunk returning a csr-output graph; every one gives the same graph with _BLOCK_ELEMS = elems, in
    at least min_blocks selection calls, all of them of the block kind (fp16 or int32) the route is meant to take"""
    from prograph_amd import Prograph
    whole = {name: fn() for name, fn in calls.items()}
    seen = []
    def spy(name, real):
        def call(*a, **kw):
            seen.append((name[:3], a[0].shape[0]))                     # the block's kind and its rows
            return real(*a, **kw)
        return call
    for name in ("f16_knn", "f16_eps", "i32_knn", "i32_eps"):
        monkeypatch.setattr(_native, name, spy(name, getattr(_native, name)))
    monkeypatch.setattr(Prograph, "_BLOCK_ELEMS", elems)
    for name, fn in calls.items():
        del seen[:]
        _same(fn(), whole[name])
        assert len(seen) >= min_blocks and {s_[0] for s_ in seen} == {kind}, (name, seen)
    return whole


def test_long_hamming_in_blocks(monkeypatch, tmp_path, capsys):
    fake_native.install(monkeypatch)
    monkeypatch.setattr(_native, "f16_eps", fake_lev_native._f16_eps)   # the stand-in that knows keep_zero (searches)
    tok = synth.clustered_tokens(300, 300, seed=5, members=20)         # 300 positions: beyond one record
    tok[77] = tok[5]
    P = _prograph(tmp_path, tok)
    capsys.readouterr()
    T = tok[:150].copy()                                               # queries: rows of the dataset, some changed
    T[::3, :4] = (T[::3, :4] % 20) + 1
    assert P._block_rows(300, 300, 64) == 300 and P._block_rows(300, 150, 64) == 150   # unpatched: one block each
    _blockwise_equals_whole(monkeypatch, P, {
        "graph k": lambda: P.build_graph(k=5, output="csr"),
        "graph eps": lambda: P.build_graph(eps=3, comp=operator.le, output="csr"),
        "search k": lambda: P.search(T, k=5, output="csr"),
        "search eps": lambda: P.search(T, eps=3, output="csr"),
    }, elems=300 * 64, min_blocks=3)                                   # 64-row blocks: 5 for the graph, 3 for the queries
    assert P._block_rows(300, 300, 64) == 64 and P._block_rows(300, 7, 1) == 7
    G = P.build_graph(k=5, output="csr")
    assert G.dist.dtype == torch.int16 and P.search(T, eps=3, output="csr").weights.dtype == torch.int16


def test_levenshtein_in_blocks(monkeypatch, tmp_path):
    fake_lev_native.install(monkeypatch)
    monkeypatch.setenv("PG_LEV_ROUTE", "dense")                        # the dense blocks for every row and threshold
    tok = LT.set_a()[:130]
    P = _prograph(tmp_path, tok)
    T = tok[:9].copy()
    T[::2, 0] = (T[::2, 0] % 20) + 1
    _blockwise_equals_whole(monkeypatch, P, {
        "graph k": lambda: P.build_graph(k=5, distance=levenshtein, output="csr"),
        "graph eps": lambda: P.build_graph(eps=3, comp=operator.le, distance=levenshtein, output="csr"),
        "search k": lambda: P.search(T, k=5, distance=levenshtein, output="csr"),
        "search eps": lambda: P.search(T, eps=3, distance=levenshtein, output="csr"),
    }, elems=130 * 3, min_blocks=3)                                    # graph: 64 + 64 + 2 rows; queries: 3 at a time
    assert P.build_graph(k=5, distance=levenshtein, output="csr").dist.dtype == torch.uint8
    assert P.search(T, eps=3, distance=levenshtein, output="csr").weights.dtype == torch.uint8


N_SHORT = 130                                                          # three graph blocks of at least 64 rows


def _route_in_blocks(monkeypatch, tmp_path, distance, eps, wdtype, wide=False, kind="f16"):
    """graph and search under `distance`, k and eps, whole and in blocks; `wide`: the same short sequences as a column of
    129 positions, which takes the routes beyond 128 positions while the stand-ins' recurrences stay short"""
    tok, _ = synth.clustered_varlen_tokens(N_SHORT, Lmax=12, Lmin=8, seed=5, members=10)
    tok = tok.copy()
    tok[77] = tok[5]
    P = _prograph(tmp_path, tok)
    X, rep = tok.astype(np.int64), "Tokenized"
    if wide:
        X, rep = np.zeros((N_SHORT, 129), dtype=np.int64), "Wide"
        X[:, :tok.shape[1]] = tok
        P.graph[rep] = list(X)
    T = X[:9].copy()                                                   # queries: rows of the dataset, every other one changed
    T[::2, 0] = (T[::2, 0] % 20) + 1
    kw = dict(distance=distance, representation=rep, output="csr")
    whole = _blockwise_equals_whole(monkeypatch, P, {
        "graph k": lambda: P.build_graph(k=5, **kw),
        "graph eps": lambda: P.build_graph(eps=eps, **kw),
        "search k": lambda: P.search(T, k=5, **kw),
        "search eps": lambda: P.search(T, eps=eps, **kw),
    }, elems=N_SHORT * 3, min_blocks=3, kind=kind)                     # graph: 64 + 64 + 2 rows; queries: 3 (int32: 1) at a time
    assert whole["graph k"].dist.dtype == whole["search k"].dist.dtype == wdtype
    assert whole["graph eps"].weights.dtype == whole["search eps"].weights.dtype == wdtype
    for name in ("graph eps", "search eps"):                           # a threshold that keeps some pairs and drops some
        g = whole[name]
        assert 0 < g.indices.numel() < (g.indptr.numel() - 1) * N_SHORT, name


def _cost(a=21, top=9):
    C = np.triu(np.random.default_rng(1).integers(1, top + 1, (a, a)), 1)
    return C + C.T


def _scores(a=21):
    S = np.triu(np.random.default_rng(2).integers(-4, 2, (a, a)), 1)
    S = S + S.T
    S[np.arange(a), np.arange(a)] = np.random.default_rng(3).integers(2, 6, a)
    return S


def test_substitution_in_blocks(monkeypatch, tmp_path):
    fake_sub_native.install(monkeypatch)
    _route_in_blocks(monkeypatch, tmp_path, substitution(_cost()), 30, torch.int16)


def test_alignment_in_blocks(monkeypatch, tmp_path):
    fake_aln_native.install(monkeypatch)
    _route_in_blocks(monkeypatch, tmp_path, alignment(_cost(), 2), 20, torch.int16)


def test_alignment_long_in_blocks(monkeypatch, tmp_path):
    fake_long_native.install(monkeypatch)
    _route_in_blocks(monkeypatch, tmp_path, alignment(_cost(), 2, gap_open=3), 20, torch.int32, wide=True, kind="i32")


def test_levenshtein_long_in_blocks(monkeypatch, tmp_path):
    fake_lev_long_native.install(monkeypatch)
    _route_in_blocks(monkeypatch, tmp_path, levenshtein, 4, torch.int16, wide=True)


@pytest.mark.parametrize("wide", [False, True])
def test_local_scores_in_blocks(monkeypatch, tmp_path, wide):
    """a score route: largest first, the mirrored comparator, the diagonal dropped from the graph - fp16 and int32 blocks"""
    fake_long_native.install(monkeypatch)
    _route_in_blocks(monkeypatch, tmp_path, local_alignment(_scores(), 3, gap_open=2), 12, torch.int32 if wide else torch.int16,
                     wide=wide, kind="i32" if wide else "f16")
