"""
Host logic of the kNN rounds beyond 63 neighbours (pg_f16_knn_round, pg_minkowski_knn_round, pg_cosine_knn_round),
without a GPU: a numpy model of the floor rule must reproduce the stable argsort's ranks 1..k for every k when the
real round loop of _native (knn_rounds and the three wrappers) drives it; build_graph routes k up to MAX_K_ROUNDS to
the device graphs and everything else to the generic loop; the C entries refuse bad arguments before any launch.
"""
import ctypes
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import fake_native
from prograph_amd import _native, synth


# ---- a numpy model of the kernels: keys, the floor-free call and one round after the floors
def _keys(vals, descending):
    """The kernels' sortable keys: fp16 bits (mk_key) or fp32 bits (cs_key), reversed for descending order."""
    if vals.dtype == np.float16:
        b = vals.view(np.uint16).astype(np.int64)
        return 0xFFFF - b if descending else b
    b = vals.view(np.uint32).astype(np.int64)
    return 0xFFFFFFFF - b if descending else b


def _head(vals, k, first, descending):
    """pg_*_knn: ranks first..first+k-1 of every row's (key, column) order."""
    m, n = vals.shape
    idx = np.full((m, k), -1, dtype=np.int32)
    w = np.zeros((m, k), dtype=vals.dtype)
    order = np.argsort(_keys(vals, descending), axis=1, kind="stable")[:, first:first + k]
    idx[:, :order.shape[1]] = order
    w[:, :order.shape[1]] = np.take_along_axis(vals, order, 1)
    return torch.from_numpy(idx), torch.from_numpy(w)


def _round(vals, k, floor_idx, floor_w, idx_out, w_out, descending):
    """pg_*_knn_round: the k smallest (key, column) pairs strictly after each row's floor; floor index -1 = exhausted."""
    keys = _keys(vals, descending)
    fk = _keys(floor_w.numpy().copy(), descending)
    fc = floor_idx.numpy()
    cols = np.arange(vals.shape[1])
    for r in range(vals.shape[0]):
        idx_out[r] = -1
        w_out[r] = 0
        if fc[r] < 0:
            continue
        after = np.nonzero((keys[r] > fk[r]) | ((keys[r] == fk[r]) & (cols > fc[r])))[0]
        pick = after[np.lexsort((after, keys[r][after]))][:k]
        idx_out[r, :len(pick)] = torch.from_numpy(pick.astype(np.int32))
        w_out[r, :len(pick)] = torch.from_numpy(vals[r, pick])


class _Op:
    """Stands in for a PackedF16 / CosineOperand: its block of values against the X operand."""
    def __init__(self, vals):
        self.vals, self.n, self.d = vals, vals.shape[0], 3
        self.buf = torch.zeros(1, dtype=torch.uint8)
        self.packed = self


@pytest.fixture
def fake_rounds(monkeypatch):
    """The floor-free calls and the three round wrappers answered by the model; the round loop is the real one."""
    real = {name: getattr(_native, name) for name in ("f16_knn", "minkowski_knn", "cosine_knn")}

    def f16_knn(block, k, first=1, descending=False):
        if first + k > 64:
            return real["f16_knn"](block, k, first, descending)
        return _head(block.numpy(), k, first, descending)

    def minkowski_knn(xp, yp, k, first=1, similarity=False):
        if first + k > 64:
            return real["minkowski_knn"](xp, yp, k, first, similarity)
        return _head(yp.vals, k, first, similarity)

    def cosine_knn(xc, yc, k, first=1, similarity=False, rows_per_block=_native._COS_ROWS):
        if first + k > 64:
            return real["cosine_knn"](xc, yc, k, first, similarity, rows_per_block)
        return _head(yc.vals, k, first, similarity)

    monkeypatch.setattr(_native, "f16_knn", f16_knn)
    monkeypatch.setattr(_native, "minkowski_knn", minkowski_knn)
    monkeypatch.setattr(_native, "cosine_knn", cosine_knn)
    monkeypatch.setattr(_native, "f16_knn_round",
                        lambda block, k, fi, fw, oi, ow, descending=False: _round(block.numpy(), k, fi, fw, oi, ow, descending))
    monkeypatch.setattr(_native, "minkowski_knn_round",
                        lambda xp, yp, k, fi, fw, oi, ow, similarity=False: _round(yp.vals, k, fi, fw, oi, ow, similarity))
    monkeypatch.setattr(_native, "cosine_knn_round",
                        lambda xc, yc, k, fi, fw, oi, ow, similarity=False, rows_per_block=0:
                        _round(yc.vals, k, fi, fw, oi, ow, similarity))


def _tied(rng, m, n, dtype, levels):
    """Non-negative values from a handful of levels: ties everywhere, across every round boundary."""
    return rng.choice(np.linspace(0, 2, levels), size=(m, n)).astype(dtype)


def _want(vals, k, descending):
    order = np.argsort(_keys(vals, descending), axis=1, kind="stable")[:, 1:k + 1]
    return order, np.take_along_axis(vals, order, 1)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("levels", [1, 3, 17])
def test_floor_rule_reproduces_the_stable_sort(fake_rounds, desc, levels):
    rng = np.random.default_rng(levels + 7 * desc)
    v16 = _tied(rng, 9, 700, np.float16, levels)
    v32 = _tied(rng, 9, 700, np.float32, levels)
    for k in (1, 63, 64, 65, 100, 127, 128, 129, 191, 192, 300, 699):
        want = _want(v16, k, desc)
        for got in (_native.f16_knn(torch.from_numpy(v16), k, first=1, descending=desc),
                    _native.minkowski_knn(_Op(v16), _Op(v16), k, first=1, similarity=desc)):
            assert got[0].shape == (9, k) and got[1].dtype == torch.float16
            assert np.array_equal(got[0].numpy(), want[0]), k
            assert np.array_equal(got[1].numpy().view(np.uint16), want[1].view(np.uint16)), k
        want = _want(v32, k, desc)
        got = _native.cosine_knn(_Op(v32), _Op(v32), k, first=1, similarity=desc)
        assert got[1].dtype == torch.float32
        assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1]), k


def test_rows_run_out_of_ranks(fake_rounds):
    """k beyond the columns: ranks that do not exist are -1 / 0, and an exhausted floor (-1) stays exhausted."""
    v = _tied(np.random.default_rng(2), 5, 90, np.float16, 4)
    for k in (89, 90, 150, 300):
        idx, w = _native.f16_knn(torch.from_numpy(v), k)
        want = _want(v, k, False)[0]
        assert np.array_equal(idx.numpy()[:, :89], want) and (idx.numpy()[:, 89:] == -1).all()
        assert (w.numpy()[:, 89:] == 0).all()


def test_round_loop_writes_column_slices(monkeypatch):
    """knn_rounds: one floor-free call of 64 - first ranks, then rounds of 64, each floored on the previous last column."""
    calls = []

    def head(kk):
        calls.append(("head", kk))
        return torch.zeros((4, kk), dtype=torch.int32), torch.zeros((4, kk), dtype=torch.float16)

    def step(kk, fi, fw, oi, ow):
        calls.append(("round", kk, fi.stride(0), oi.stride(0), oi.storage_offset() - fi.storage_offset()))
        oi.fill_(len(calls))

    idx, _ = _native.knn_rounds(4, 200, 1, torch.float16, torch.device("cpu"), head, step)
    assert calls == [("head", 63), ("round", 64, 200, 200, 1), ("round", 64, 200, 200, 1), ("round", 9, 200, 200, 1)]
    assert (idx[:, 63:127] == 2).all() and (idx[:, 127:191] == 3).all() and (idx[:, 191:] == 4).all()
    with pytest.raises(ValueError):
        _native.knn_rounds(4, _native.MAX_K_ROUNDS + 1, 1, torch.float16, torch.device("cpu"), head, step)


# ---- routing in build_graph
def _prograph(tmp_path, tok, name="r"):
    from prograph_amd import Prograph
    f = tmp_path / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    return Prograph(file=str(f))


def test_long_sequences_keep_device_graphs_beyond_63(monkeypatch, tmp_path, capsys):
    """Byte tokens beyond one engine record (L = 300) with k = 100: a KNNGraph of width 100, kept by store=, equal to
    the generic loop's tuples - through the fake selection of tests/fake_native.py on the CPU."""
    from prograph_amd.distance import hamming
    from prograph_amd.graph import KNNGraph
    fake_native.install(monkeypatch)
    tok = synth.clustered_tokens(150, 300, seed=5, members=30)
    tok[3] = tok[40]
    pg = _prograph(tmp_path, tok)
    capsys.readouterr()
    G = pg.build_graph(k=100, output="csr")
    assert isinstance(G, KNNGraph) and tuple(G.idx.shape) == (150, 100)
    want = pg.build_graph(k=100, distance=lambda X, Y, similarity=False: hamming(X, Y, similarity=similarity))
    got = pg.build_graph(k=100, store="E")
    assert "E" in pg.csr_graphs and pg.graph["E"] is not None
    for (gi, gw), (wi, ww) in zip(got, want):
        assert np.array_equal(gi, wi) and np.array_equal(gw.astype(np.float64), ww.astype(np.float64))


def _spies(monkeypatch, pg):
    called = []
    for name in ("_build_graph_minkowski", "_build_graph_cosine", "_build_graph_long"):
        monkeypatch.setattr(type(pg), name, lambda self, *a, _n=name, **k: called.append(_n))
    return called


def test_routing_up_to_max_k_rounds(monkeypatch, tmp_path, capsys):
    from prograph_amd.distance import cosine, minkowski
    fake_native.install(monkeypatch)
    pg = _prograph(tmp_path, synth.clustered_tokens(30, 8, seed=1))
    capsys.readouterr()
    pg.graph["Embedded"] = list(np.random.default_rng(1).standard_normal((30, 5)).astype(np.float32))
    called = _spies(monkeypatch, pg)
    for dist, name in ((minkowski, "_build_graph_minkowski"), (cosine, "_build_graph_cosine")):
        for k in (64, 100, _native.MAX_K_ROUNDS):
            called.clear()
            pg.build_graph(representation="Embedded", k=k, distance=dist)      # the spy answers None: generic then
            assert called == [name], (name, k)
        called.clear()
        t = pg.build_graph(representation="Embedded", k=_native.MAX_K_ROUNDS + 1, distance=dist)
        assert not called and len(t) == 30
        t = pg.build_graph(representation="Embedded", eps=0.5, distance=dist, comp=operator.ne)
        assert not called and len(t) == 30


def test_long_routing_up_to_max_k_rounds(monkeypatch, tmp_path, capsys):
    fake_native.install(monkeypatch)
    pg = _prograph(tmp_path, synth.clustered_tokens(20, 300, seed=2, members=5), "l")
    capsys.readouterr()
    called = _spies(monkeypatch, pg)
    pg.build_graph(k=_native.MAX_K_ROUNDS)
    assert called == ["_build_graph_long"]
    called.clear()
    t = pg.build_graph(k=_native.MAX_K_ROUNDS + 1)
    assert not called and len(t) == 20
    t = pg.build_graph(eps=3, comp=operator.ne)
    assert not called and len(t) == 20


# ---- the C ABI of the round entries: declared, bound, exported, and argument checks before any launch
def test_round_entries_validate_arguments():
    L = _native.lib()
    for name in ("pg_f16_knn_round", "pg_minkowski_knn_round", "pg_cosine_knn_round"):
        assert name in _native.SYMBOLS and hasattr(L, name)
    p = ctypes.c_void_p(256)          # never dereferenced: every call below is refused on the host
    f16 = [p, 10, 300, 300]
    for k in (0, 65):
        assert L.pg_f16_knn_round(*f16, k, 0, p, p, 64, p, p, 64, None) == -1
        assert b"pg_f16_knn_round" in L.pg_last_error()
    assert L.pg_f16_knn_round(*f16, 64, 0, None, p, 64, p, p, 64, None) == -1          # no floor
    assert L.pg_f16_knn_round(*f16, 64, 0, p, None, 64, p, p, 64, None) == -1
    assert L.pg_f16_knn_round(*f16, 64, 0, p, p, 64, p, p, 63, None) == -1            # ldo < k
    assert L.pg_f16_knn_round(p, 10, 300, 200, 8, 0, p, p, 64, p, p, 64, None) == -1   # ld < n
    mk = [p, 10, 256, p, 10, 256, 8, 0]
    for k in (0, 65):
        assert L.pg_minkowski_knn_round(*mk, k, p, p, 64, p, p, 64, None) == -1
        assert b"pg_minkowski_knn_round" in L.pg_last_error()
    assert L.pg_minkowski_knn_round(*mk, 8, None, p, 64, p, p, 64, None) == -1
    assert L.pg_minkowski_knn_round(p, 10, 100, p, 10, 256, 8, 0, 8, p, p, 64, p, p, 64, None) == -1   # x_npad % 256
    assert L.pg_minkowski_knn_round(p, 10, 256, p, 300, 256, 8, 0, 8, p, p, 64, p, p, 64, None) == -1  # y_npad < m
    ops = [p, p, p, 10, 256, p, p, p, 10, 256, 8, 0]
    for k in (0, 65):
        assert L.pg_cosine_knn_round(*ops, k, p, p, 64, p, p, 64, None) == -1
        assert b"pg_cosine_knn_round" in L.pg_last_error()
    assert L.pg_cosine_knn_round(*ops, 8, p, None, 64, p, p, 64, None) == -1
    assert L.pg_cosine_knn_round(p, None, p, 10, 256, p, p, p, 10, 256, 8, 0, 8, p, p, 64, p, p, 64, None) == -1
