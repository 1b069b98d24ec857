"""
The selection layer's host side without a GPU: `_native.cat_csr` on hand-made parts, and the block helper of
prograph.py (`_select_blocks` / `_block_rows`) through the CPU stand-ins - a graph or search cut into several row
blocks is the graph or search of one block.
"""
import operator

import numpy as np
import pandas as pd
import torch

import fake_lev_native
import fake_native
import lev_testdata as LT
from prograph_amd import _native, synth
from prograph_amd.distance import levenshtein


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


def _blockwise_equals_whole(monkeypatch, P, calls, elems, min_blocks):
    """calls: name -> thunk returning a csr-output graph; every one gives the same graph with _BLOCK_ELEMS = elems, in
    at least min_blocks selection calls"""
    from prograph_amd import Prograph
    whole = {name: fn() for name, fn in calls.items()}
    seen = []
    for name in ("f16_knn", "f16_eps"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _r=real, **kw: (seen.append(a[0].shape[0]), _r(*a, **kw))[1])
    monkeypatch.setattr(Prograph, "_BLOCK_ELEMS", elems)
    for name, fn in calls.items():
        del seen[:]
        _same(fn(), whole[name])
        assert len(seen) >= min_blocks, (name, seen)


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
