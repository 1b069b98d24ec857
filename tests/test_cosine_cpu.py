"""
CPU checks of the cosine distance: the operator's import and export, its torch expression (the path for anything
that is not a finite fp16 device tensor) against an fp64 restatement of the contract, `build_graph(distance=cosine)`
through the generic batch loop on CPU-staged data, the `final=True` graph containers that carry the kernels' fp32
values, and the argument checks of the new C-ABI entries (no launch, no GPU needed).
"""
import ctypes
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import fake_native
from prograph_amd import _native, synth
from prograph_amd.graph import CSRGraph, KNNGraph, load_graphs, save_graphs


def _bound(d):
    return d * 2.0 ** -24 + 2.0 ** -21


def _d64(x, y):
    """The contract in fp64: rows of y against rows of x; zero vectors -> 1; clamp to [0, 2]."""
    a, b = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    na, nb = (a * a).sum(1), (b * b).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1 - (b @ a.T) / np.sqrt(nb)[:, None] / np.sqrt(na)[None, :]
    d = np.clip(d, 0, 2)
    d[(na[None, :] == 0) | (nb[:, None] == 0)] = 1
    return d


def test_cosine_is_exported():
    from prograph_amd import distance
    from prograph_amd.distance import cosine
    from prograph_amd.distance.cosine import cosine as c2
    assert distance.cosine is cosine is c2 and callable(cosine)


@pytest.mark.parametrize("d", [1, 3, 16, 100])
def test_torch_expression_against_fp64(d):
    from prograph_amd.distance import cosine
    rng = np.random.default_rng(d)
    x = rng.standard_normal((40, d)).astype(np.float16)
    y = rng.standard_normal((13, d)).astype(np.float16)
    x[5] = 0
    y[2] = 0
    y[4] = x[9]
    y[6] = -x[1]
    for a, b in ((x, y), (torch.from_numpy(x), torch.from_numpy(y)), (x.astype(np.float32), y.astype(np.float64))):
        got = cosine(a, b)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.shape == (13, 40)
        g = got.numpy().astype(np.float64)
        ref = _d64(x, y)
        assert np.abs(g - ref).max() <= _bound(d)
        assert np.all(g[:, 5] == 1) and np.all(g[2] == 1)
        assert np.all((g >= 0) & (g <= 2))
        s = cosine(a, b, similarity=True)
        assert s.dtype == torch.float32 and torch.equal(s, 1 / (1 + got))
    # D = 1: every pair is parallel, antiparallel or involves a zero
    x1 = np.array([[1.0], [-2.0], [0.0], [0.5]], dtype=np.float16)
    g = cosine(x1, x1).numpy()
    ref = _d64(x1, x1)
    assert np.abs(g - ref).max() <= _bound(1) and np.all(g[2] == 1) and np.all(g[:, 2] == 1)


def test_identical_rows_are_zero_when_the_sums_agree():
    """Rule 2 on the torch path: p == nx == ny bitwise gives exactly 0 (here with values whose sums are exact)."""
    from prograph_amd.distance import cosine
    x = np.array([[1, 2, 3, 4], [1, 2, 3, 4], [2, 4, 6, 8], [0, 0, 0, 0]], dtype=np.float16)
    g = cosine(x, x).numpy()
    assert g[0, 1] == 0 and g[1, 0] == 0 and g[0, 0] == 0 and g[2, 2] == 0
    assert g[3, 3] == 1 and g[0, 3] == 1
    assert 0 <= g[0, 2] <= _bound(4)


def test_operands_are_cleaned_like_the_other_operators():
    from prograph_amd.distance import cosine
    with pytest.raises(ValueError):
        cosine(np.zeros((0, 3)), np.ones((2, 3)))
    got = cosine(np.ones((2, 3)), np.ones((1, 5)))                    # shorter operand right-padded with zeros
    assert got.shape == (1, 2) and np.all(np.abs(got.numpy() - (1 - 3 / np.sqrt(15))) < 1e-6)


def _prograph(tmp_path, n, seed=3):
    from prograph_amd import Prograph
    tok = synth.clustered_tokens(n, 8, seed=seed)
    f = tmp_path / "c.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(seed).uniform(0, 1, n)}).to_csv(f)
    return Prograph(file=str(f))


def test_build_graph_generic_on_cpu(monkeypatch, tmp_path, capsys):
    from prograph_amd.distance import cosine
    fake_native.install(monkeypatch)
    n, d = 150, 12
    pg = _prograph(tmp_path, n)
    capsys.readouterr()
    rng = np.random.default_rng(4)
    emb = rng.standard_normal((n, d)).astype(np.float16)
    emb[30] = 0
    pg.graph["Embedded"] = list(emb.astype(np.float32))
    ref = _d64(emb, emb)
    bound = _bound(d)
    k = 6
    t = pg.build_graph(representation="Embedded", k=k, distance=cosine)
    assert len(t) == n
    order = np.argsort(ref, axis=1, kind="stable")
    for r, (ix, w) in enumerate(t):
        assert len(ix) == k and w.dtype == np.float32
        assert np.all(np.diff(w) >= 0)                                 # ascending distances
        assert np.abs(w - ref[r, ix]).max() <= bound
        # the fp64 distances of the returned columns equal the fp64 ranks 1..k within twice the bound
        assert np.abs(np.sort(ref[r, ix]) - ref[r, order[r, 1:k + 1]]).max() <= 2 * bound
    ts = pg.build_graph(representation="Embedded", k=k, similarity=True, distance=cosine)
    for r, (ix, w) in enumerate(ts):
        assert np.all(np.diff(w) <= 0) and np.abs(w - 1 / (1 + ref[r, ix])).max() <= bound
    eps = 0.6
    te = pg.build_graph(representation="Embedded", eps=eps, distance=cosine)
    clear = (np.abs(ref - eps) > bound) & (ref > bound)          # self pairs: torch's fp32 sums need not agree bitwise
    want = ref <= eps
    for r, (ix, w) in enumerate(te):
        hit = np.zeros(n, dtype=bool)
        hit[ix] = True
        assert np.array_equal(hit[clear[r]], want[r][clear[r]]), r
        assert np.all(np.abs(w - ref[r, ix]) <= bound) and np.all(w > 0)
    assert len(te[30][0]) == 0                                           # the zero vector: d = 1 everywhere


# ---- containers with final fp32 values
INDPTR = np.array([0, 2, 2, 5, 6], dtype=np.int64)
INDICES = np.array([1, 3, 0, 1, 3, 2], dtype=np.int32)
F32 = np.array([0.25, 1.5, 0.0999, 2.0, 1e-7, 0.33333334], dtype=np.float32)
KIDX = np.array([[1, 2], [0, 3], [3, 1], [2, 0]], dtype=np.int32)      # every slot filled (empty ones: test_graph_containers_cpu.py)
KF32 = np.array([[0.5, 0.79], [0.5, 1.25], [1.0, 1.75], [1.0, 0.0]], dtype=np.float32)


def _csr(w, similarity, final=True):
    return CSRGraph(torch.from_numpy(INDPTR), torch.from_numpy(INDICES), torch.from_numpy(w), 4, similarity=similarity,
                    final=final)


def _knn(w, similarity, final=True):
    return KNNGraph(torch.from_numpy(KIDX), torch.from_numpy(w), 4, similarity=similarity, final=final)


@pytest.mark.parametrize("sim", [False, True])
def test_final_weights_pass_through(sim):
    g = _csr(F32, sim)
    ip, ix, w = g.host()
    assert np.array_equal(ip, INDPTR) and ix.dtype == np.int64 and np.array_equal(ix, INDICES)
    assert w.dtype == np.float32 and np.array_equal(w, F32)
    t = g.to_tuples()
    for r in (0, 2, 3):
        a, b = INDPTR[r], INDPTR[r + 1]
        assert np.array_equal(t[r][0], INDICES[a:b]) and t[r][1].dtype == np.float32 and np.array_equal(t[r][1], F32[a:b])
    k = _knn(KF32, sim)
    kix, kw = k.host()
    assert np.array_equal(kix, KIDX) and kw.dtype == np.float32 and np.array_equal(kw, KF32)
    assert all(b.dtype == np.float32 for _, b in k.to_tuples())
    c = k.as_csr()
    assert c.final and c.weights.dtype == torch.float32 and np.array_equal(c.host()[2], KF32.reshape(-1))
    # without final=True float32 weights keep their Hamming meaning (test_other_weight_dtypes_unchanged)
    assert not np.array_equal(_csr(F32, True, final=False).host()[2], F32)


@pytest.mark.parametrize("sim", [False, True])
def test_final_weights_reach_the_row_reductions_as_float32(monkeypatch, sim):
    seen = []

    def spy(indptr, indices, weights, **kw):
        seen.append(None if weights is None else weights)
        return fake_native._csr_row_stats(indptr, indices, weights, **kw)
    monkeypatch.setattr(_native, "csr_row_stats", spy)
    deg = _csr(F32, sim).degree()
    assert seen[-1].dtype == torch.float32 and np.array_equal(seen[-1].numpy(), F32)
    want = np.zeros(4)
    np.add.at(want, np.repeat(np.arange(4), np.diff(INDPTR)), F32.astype(np.float64))
    assert np.allclose(deg, want.astype(np.float32), rtol=1e-7, atol=0)
    f = np.array([0.25, 0.5, 1.0, 0.0])
    nb = np.array([[1, 2], [0, 3], [3, 1], [2, 0]], dtype=np.int32)
    kw = np.array([[0.5, 0.75], [0.5, 1.25], [1.0, 1.5], [1.0, 0.125]], dtype=np.float32)
    got = KNNGraph(torch.from_numpy(nb), torch.from_numpy(kw), 4, similarity=sim, final=True).as_csr().dirichlet(f)
    A = np.zeros((4, 4))
    for r in range(4):
        for j in range(2):
            A[r, nb[r, j]] += float(kw[r, j])
    assert np.isclose(got, f @ (np.diag(A.sum(1)) - A) @ f, rtol=1e-12)


@pytest.mark.parametrize("sim", [False, True])
def test_final_graphs_round_trip_the_side_car(tmp_path, sim):
    p = str(tmp_path / "g.npz")
    save_graphs(p, {"E": _csr(F32, sim), "K": _knn(KF32, sim), "H": _csr(F32, sim, final=False)}, tokens_fingerprint=7)
    z = np.load(p)
    assert list(z["E/meta"]) == [0, 4, int(sim), 0, 1] and list(z["H/meta"]) == [0, 4, int(sim), 0, 0]
    got = load_graphs(p, device="cpu", tokens_fingerprint=7)
    e, k, h = got["E"], got["K"], got["H"]
    assert e.final and k.final and not h.final and e.similarity == sim and k.similarity == sim
    assert np.array_equal(e.host()[2], F32) and np.array_equal(k.host()[1], KF32)
    assert np.array_equal(h.host()[2], _csr(F32, sim, final=False).host()[2])


def test_old_four_entry_metas_still_load(tmp_path):
    p = str(tmp_path / "old.npz")
    np.savez(p, **{"E/indptr": INDPTR, "E/indices": INDICES, "E/weights": np.array([1, 2, 3, 1, 2, 4], dtype=np.uint8),
                   "E/meta": np.array([0, 4, 1, 0], dtype=np.int64),
                   "K/idx": KIDX, "K/dist": np.array([[1, 2], [1, 3], [2, 2], [1, 0]], dtype=np.uint8),
                   "K/meta": np.array([1, 4, 0, 0], dtype=np.int64)})
    got = load_graphs(p, device="cpu")
    assert set(got) == {"E", "K"} and not got["E"].final and not got["K"].final
    assert got["E"].similarity and np.array_equal(got["E"].host()[2], (1 / (1 + torch.tensor([1, 2, 3, 1, 2, 4]))).numpy())
    assert np.array_equal(got["K"].host()[1], np.array([[1, 2], [1, 3], [2, 2], [1, 0]]))


def test_cosine_dispatch_needs_the_comparators(monkeypatch, tmp_path, capsys):
    """A comparator outside the five orderings goes to the generic loop, never to the cosine kernels."""
    from prograph_amd.distance import cosine
    fake_native.install(monkeypatch)
    pg = _prograph(tmp_path, 40)
    capsys.readouterr()
    pg.graph["Embedded"] = list(np.random.default_rng(1).standard_normal((40, 5)).astype(np.float32))
    called = []
    monkeypatch.setattr(type(pg), "_build_graph_cosine", lambda self, *a, **k: called.append(1))
    t = pg.build_graph(representation="Embedded", eps=0.5, distance=cosine, comp=operator.ne)
    assert not called and len(t) == 40


# ---- the C ABI of the cosine kernels: present, and argument checks before any launch (no GPU needed)
def test_cosine_entries_validate_arguments():
    L = _native.lib()
    for name in ("pg_cosine_prep", "pg_cosine_dense", "pg_cosine_knn", "pg_cosine_eps_slots", "pg_cosine_eps_compact",
                 "pg_cosine_eps_fill_rows"):
        assert name in _native.SYMBOLS and hasattr(L, name)
    p = ctypes.c_void_p(256)          # never dereferenced: every call below is refused on the host
    rc = L.pg_cosine_prep(p, 10, 100, 8, p, p, p, None)                  # npad not a multiple of 256
    assert rc == -1 and b"pg_cosine_prep: bad argument" in L.pg_last_error()
    rc = L.pg_cosine_prep(p, 10, 256, 0, p, p, p, None)
    assert rc == -1 and b"pg_cosine_prep" in L.pg_last_error()
    rc = L.pg_cosine_prep(p, 10, 256, 8, p, p, None, None)
    assert rc == -1 and b"pg_cosine_prep" in L.pg_last_error()
    ops = [p, p, p, 10, 256, p, p, p, 10, 256, 8]
    rc = L.pg_cosine_dense(*ops, 0, p, 5, None)                          # ldo < n
    assert rc == -1 and b"pg_cosine_dense: bad argument" in L.pg_last_error()
    rc = L.pg_cosine_dense(p, None, p, 10, 256, p, p, p, 10, 256, 8, 0, p, 10, None)
    assert rc == -1 and b"pg_cosine_dense" in L.pg_last_error()
    rc = L.pg_cosine_knn(None, p, p, 10, 256, p, p, p, 10, 256, 8, 0, 4, 1, p, p, None)
    assert rc == -1 and b"pg_cosine_knn: bad argument" in L.pg_last_error()
    rc = L.pg_cosine_knn(*ops, 0, 60, 5, p, p, None)
    assert rc == -1 and b"first + k must be at most 64" in L.pg_last_error()
    rc = L.pg_cosine_knn(*ops, 0, 0, 1, p, p, None)
    assert rc == -1 and b"first + k" in L.pg_last_error()
    rc = L.pg_cosine_knn(p, p, p, 10, 100, p, p, p, 10, 256, 8, 0, 4, 1, p, p, None)     # x_npad not a multiple of 256
    assert rc == -1 and b"bad argument" in L.pg_last_error()
    rc = L.pg_cosine_knn(p, p, p, 10, 256, p, p, p, 300, 256, 8, 0, 4, 1, p, p, None)    # y_npad < m
    assert rc == -1 and b"bad argument" in L.pg_last_error()
    rc = L.pg_cosine_eps_slots(*ops, 0, 0, 0.5, 16, None, p, p, None)
    assert rc == -1 and b"pg_cosine_eps_slots: bad argument" in L.pg_last_error()
    rc = L.pg_cosine_eps_slots(*ops, 0, 7, 0.5, 16, p, p, p, None)      # no such comparator
    assert rc == -1 and b"pg_cosine_eps_slots" in L.pg_last_error()
    rc = L.pg_cosine_eps_slots(*ops, 0, 0, 0.5, 0, p, p, p, None)       # cap < 1
    assert rc == -1 and b"pg_cosine_eps_slots" in L.pg_last_error()
    rc = L.pg_cosine_eps_compact(10, 16, p, p, None, p, p, p, None)
    assert rc == -1 and b"pg_cosine_eps_compact: bad argument" in L.pg_last_error()
    rc = L.pg_cosine_eps_fill_rows(*ops, 0, 0, 0.5, None, 3, p, p, p, None)
    assert rc == -1 and b"pg_cosine_eps_fill_rows: bad argument" in L.pg_last_error()
    rc = L.pg_cosine_eps_fill_rows(*ops, 0, 0, 0.5, p, 0, p, p, p, None)
    assert rc == -1 and b"pg_cosine_eps_fill_rows" in L.pg_last_error()
