"""
CPU checks of the device-graph containers with fp16 Minkowski weights (prograph_amd/graph.py) and of the
argument checks of the fused Minkowski C-ABI entries (pg_minkowski_knn / pg_minkowski_eps_*).  The
containers are built from CPU tensors here; on the GPU the same code runs on device tensors.

fp16 weights are final values (distances or similarities 1/(1+d) as the kernels computed them): they pass
through host(), to_tuples(), as_csr() and the .npz side-car unchanged whatever `similarity` says, and reach
the row reductions as float32.  uint8 / int16 / float32 weights keep their Hamming meaning.
"""
import ctypes

import numpy as np
import pytest
import torch

import fake_native
from prograph_amd import _native
from prograph_amd.graph import CSRGraph, KNNGraph, load_graphs, save_graphs

INDPTR = np.array([0, 2, 2, 5, 6], dtype=np.int64)
INDICES = np.array([1, 3, 0, 1, 3, 2], dtype=np.int32)
F16 = np.array([0.79052734, 1.5, 0.0999, 65504.0, np.inf, 0.33325195], dtype=np.float16)
KIDX = np.array([[1, 2], [0, 3], [3, 1], [2, 0]], dtype=np.int32)      # every slot filled (empty ones: test_graph_containers_cpu.py)
KF16 = np.array([[0.5, 0.79052734], [0.5, 2.25], [1.0, 3.0], [1.0, 0.0]], dtype=np.float16)


def _csr(w, similarity):
    return CSRGraph(torch.from_numpy(INDPTR), torch.from_numpy(INDICES), torch.from_numpy(w), 4, similarity=similarity)


def _knn(w, similarity):
    return KNNGraph(torch.from_numpy(KIDX), torch.from_numpy(w), 4, similarity=similarity)


def _bits(a):
    return np.asarray(a).view(np.uint16)


@pytest.mark.parametrize("sim", [False, True])
def test_csr_fp16_weights_pass_through(sim):
    g = _csr(F16, sim)
    ip, ix, w = g.host()
    assert np.array_equal(ip, INDPTR) and ix.dtype == np.int64 and np.array_equal(ix, INDICES)
    assert w.dtype == np.float16 and np.array_equal(_bits(w), _bits(F16))
    t = g.to_tuples()
    assert len(t) == 4 and len(t[1][0]) == 0 and t[1][0].dtype == int and t[1][1].dtype == int
    for r in (0, 2, 3):
        a, b = INDPTR[r], INDPTR[r + 1]
        assert t[r][0].dtype == np.int64 and np.array_equal(t[r][0], INDICES[a:b])
        assert t[r][1].dtype == np.float16 and np.array_equal(_bits(t[r][1]), _bits(F16[a:b]))
    I, J, V = g.coords()
    assert V.dtype == np.float32 and np.array_equal(V, F16.astype(np.float32)) and np.array_equal(J, INDICES)


@pytest.mark.parametrize("sim", [False, True])
def test_knn_fp16_weights_pass_through(sim):
    g = _knn(KF16, sim)
    ix, w = g.host()
    assert ix.dtype == np.int64 and np.array_equal(ix, KIDX[:, :2])
    assert w.dtype == np.float16 and np.array_equal(_bits(w), _bits(KF16))
    t = g.to_tuples()
    assert all(a.dtype == np.int64 and b.dtype == np.float16 for a, b in t)
    assert np.array_equal(_bits(np.stack([b for _, b in t])), _bits(KF16))
    c = g.as_csr()
    assert c.weights.dtype == torch.float16 and np.array_equal(_bits(c.host()[2]), _bits(KF16.reshape(-1)))
    assert np.array_equal(c.host()[1], KIDX.reshape(-1))


@pytest.mark.parametrize("sim", [False, True])
def test_fp16_graphs_round_trip_the_side_car(tmp_path, sim):
    p = str(tmp_path / "g.npz")
    save_graphs(p, {"E": _csr(F16, sim), "K": _knn(KF16, sim)}, tokens_fingerprint=7)
    got = load_graphs(p, device="cpu", tokens_fingerprint=7)
    assert set(got) == {"E", "K"}
    e, k = got["E"], got["K"]
    assert isinstance(e, CSRGraph) and isinstance(k, KNNGraph) and e.similarity == sim and k.similarity == sim
    assert e.weights.dtype == torch.float16 and np.array_equal(_bits(e.weights.numpy()), _bits(F16))
    assert k.dist.dtype == torch.float16 and np.array_equal(_bits(k.dist.numpy()), _bits(KF16))
    assert np.array_equal(e.indptr.numpy(), INDPTR) and np.array_equal(k.idx.numpy(), KIDX)
    assert np.array_equal(_bits(e.host()[2]), _bits(F16)) and np.array_equal(_bits(k.host()[1]), _bits(KF16))


@pytest.mark.parametrize("sim", [False, True])
def test_fp16_weights_reach_the_row_reductions_as_float32(monkeypatch, sim):
    seen = []

    def spy(indptr, indices, weights, **kw):
        seen.append(None if weights is None else weights.dtype)
        return fake_native._csr_row_stats(indptr, indices, weights, **kw)
    monkeypatch.setattr(_native, "csr_row_stats", spy)
    g = _csr(F16, sim)
    deg = g.degree()
    assert seen == [torch.float32]
    want = np.zeros(4)
    np.add.at(want, np.repeat(np.arange(4), np.diff(INDPTR)), F16.astype(np.float64))
    assert np.array_equal(deg, want.astype(np.float32))
    f = np.array([0.25, 0.5, 1.0, 0.0])
    nb = np.array([[1, 2], [0, 3], [3, 1], [2, 0]], dtype=np.int32)
    kw = np.array([[0.5, 0.75], [0.5, 2.25], [1.0, 3.0], [1.0, 1.5]], dtype=np.float16)
    kn = KNNGraph(torch.from_numpy(nb), torch.from_numpy(kw), 4, similarity=sim).as_csr()
    got = kn.dirichlet(f)
    assert seen[-1] == torch.float32
    A = np.zeros((4, 4))
    for r in range(4):
        for j in range(2):
            A[r, nb[r, j]] += float(kw[r, j])
    assert np.isclose(got, f @ (np.diag(A.sum(1)) - A) @ f, rtol=1e-12)


# ---- other weight dtypes: exactly what they gave before fp16 weights existed
@pytest.mark.parametrize("sim", [False, True])
@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.float32])
def test_other_weight_dtypes_unchanged(monkeypatch, dt, sim, tmp_path):
    wv = np.array([1, 2, 3, 1, 2, 4], dtype=dt)
    g = _csr(wv, sim)
    ip, ix, w = g.host()
    w64 = wv.astype(np.int64) if dt != np.float32 else torch.from_numpy(wv).to(torch.int64).numpy()
    want = (1 / (1 + torch.from_numpy(w64))).numpy() if sim else w64
    assert w.dtype == want.dtype and np.array_equal(w, want) and ix.dtype == np.int64
    seen = []

    def spy(indptr, indices, weights, **kw):
        seen.append(weights.dtype)
        return fake_native._csr_row_stats(indptr, indices, weights, **kw)
    monkeypatch.setattr(_native, "csr_row_stats", spy)
    g.degree()
    assert seen == [torch.float32 if (sim or dt == np.int16) else torch.from_numpy(wv).dtype]
    kw = np.array([[1, 2], [1, 3], [2, 2], [1, 0]], dtype=dt)
    k = _knn(kw, sim)
    kidx, kwt = k.host()
    d = torch.from_numpy(kw[:, :2]).to(torch.int64)
    assert np.array_equal(kwt, (1 / (1 + d)).numpy() if sim else d.numpy()) and kwt.dtype == ((1 / (1 + d)).numpy() if sim else d.numpy()).dtype
    assert k.as_csr().weights.dtype == torch.from_numpy(kw).dtype
    p = str(tmp_path / "o.npz")
    save_graphs(p, {"E": g, "K": k})
    back = load_graphs(p, device="cpu")
    assert back["E"].weights.dtype == g.weights.dtype and np.array_equal(back["E"].host()[2], w)
    assert back["K"].dist.dtype == k.dist.dtype and np.array_equal(back["K"].host()[1], kwt)


# ---- the C ABI of the fused kernels: present, and argument checks before any launch (no GPU needed)
def test_fused_minkowski_entries_validate_arguments():
    L = _native.lib()
    for name in ("pg_minkowski_knn", "pg_minkowski_eps_slots", "pg_minkowski_eps_compact", "pg_minkowski_eps_fill_rows"):
        assert name in _native.SYMBOLS and hasattr(L, name)
    p = ctypes.c_void_p(256)          # never dereferenced: every call below is refused on the host
    rc = L.pg_minkowski_knn(None, 10, 256, p, 10, 256, 8, 0, 4, 1, p, p, None)
    assert rc == -1 and b"pg_minkowski_knn: bad argument" in L.pg_last_error()
    rc = L.pg_minkowski_knn(p, 10, 256, p, 10, 256, 8, 0, 60, 5, p, p, None)
    assert rc == -1 and b"first + k must be at most 64" in L.pg_last_error()
    rc = L.pg_minkowski_knn(p, 10, 256, p, 10, 256, 8, 0, 0, 1, p, p, None)
    assert rc == -1 and b"first + k" in L.pg_last_error()
    rc = L.pg_minkowski_knn(p, 10, 100, p, 10, 256, 8, 0, 4, 1, p, p, None)     # x_npad not a multiple of 256
    assert rc == -1 and b"bad argument" in L.pg_last_error()
    rc = L.pg_minkowski_eps_slots(p, 10, 256, p, 10, 256, 8, 0, 0, 1.0, 16, None, p, p, None)
    assert rc == -1 and b"pg_minkowski_eps_slots: bad argument" in L.pg_last_error()
    rc = L.pg_minkowski_eps_slots(p, 10, 256, p, 10, 256, 8, 0, 7, 1.0, 16, p, p, p, None)      # no such comparator
    assert rc == -1 and b"pg_minkowski_eps_slots" in L.pg_last_error()
    rc = L.pg_minkowski_eps_compact(10, 16, p, p, None, p, p, p, None)
    assert rc == -1 and b"pg_minkowski_eps_compact: bad argument" in L.pg_last_error()
    rc = L.pg_minkowski_eps_fill_rows(p, 10, 256, p, 10, 256, 8, 0, 0, 1.0, None, 3, p, p, p, None)
    assert rc == -1 and b"pg_minkowski_eps_fill_rows: bad argument" in L.pg_last_error()
