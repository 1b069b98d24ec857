"""
CPU checks of the Euclidean distance: the operator's import and export, its torch expression (the path for anything
that is not a finite fp16 device tensor) against an fp64 restatement within the stated bound, the rules of the contract
(duplicates exactly 0, a zero vector an ordinary point, no overflow where `minkowski` gives inf), `build_graph` and
`search` through the generic loop on CPU-staged data, the `final=True` containers, and the argument checks of the five
new C-ABI entries (no launch, no GPU needed).

The bound is on the SQUARE, because the form cancels: with the exact d^2 of the fp16 values
    |got^2 - d^2| <= B(D) (nx + ny) + 2^-22 d^2,    B(D) = 2 D 2^-24 + 2^-21.
Selections are therefore compared in d^2: a column chosen in place of a better one is within the sum of the two pairs'
bounds of it, hence within twice the row's largest bound.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import fake_native
from prograph_amd import _native, synth
from prograph_amd.graph import CSRGraph, KNNGraph, load_graphs, save_graphs


def _B(d):
    return 2 * d * 2.0 ** -24 + 2.0 ** -21


def _ref2(x, y):
    """Exact d^2 of the fp16 values in fp64 (rows of y against rows of x), direct form, and the bound of every pair."""
    a, b = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    d2 = ((b[:, None, :] - a[None, :, :]) ** 2).sum(2)
    na, nb = (a * a).sum(1), (b * b).sum(1)
    return d2, _B(a.shape[1]) * (na[None, :] + nb[:, None]) + 2.0 ** -22 * d2


def test_euclidean_is_exported():
    from prograph_amd import distance
    from prograph_amd.distance import euclidean
    from prograph_amd.distance.euclidean import euclidean as e2
    assert distance.euclidean is euclidean is e2 and callable(euclidean)
    assert "B(D) = 2 D 2^-24 + 2^-21" in distance.euclidean.__globals__["__doc__"]     # the module states the tolerance


@pytest.mark.parametrize("scale", [1e-3, 1.0, 30.0])
@pytest.mark.parametrize("d", [1, 3, 16, 100])
def test_torch_expression_against_fp64(d, scale):
    from prograph_amd.distance import euclidean
    rng = np.random.default_rng(d)
    x = (rng.standard_normal((40, d)) * scale).astype(np.float16)
    y = (rng.standard_normal((13, d)) * scale).astype(np.float16)
    x[5] = 0
    y[2] = 0
    y[4] = x[9]
    y[6] = -x[1]
    ref2, bound = _ref2(x, y)
    for a, b in ((x, y), (torch.from_numpy(x), torch.from_numpy(y)), (x.astype(np.float32), y.astype(np.float64))):
        got = euclidean(a, b)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and got.shape == (13, 40)
        g = got.numpy().astype(np.float64)
        err = np.abs(g * g - ref2)
        worst = float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max())     # two zero vectors: 0 of 0
        print(f"D={d} scale={scale}: max err/bound = {worst:.3f}")
        assert np.all(err <= bound), worst
        assert np.all(g >= 0) and np.all(np.isfinite(g))
        s = euclidean(a, b, similarity=True)
        assert s.dtype == torch.float32 and torch.equal(s, 1 / (1 + got))


def test_identical_rows_are_zero_when_the_sums_agree():
    """p == nx == ny bitwise gives exactly 0 (values whose sums are exact); two zero vectors are identical."""
    from prograph_amd.distance import euclidean
    x = np.array([[1, 2, 3, 4], [1, 2, 3, 4], [2, 4, 6, 8], [0, 0, 0, 0]], dtype=np.float16)
    g = euclidean(x, x).numpy()
    assert g[0, 1] == 0 and g[1, 0] == 0 and g[0, 0] == 0 and g[2, 2] == 0 and g[3, 3] == 0
    assert abs(float(g[0, 2]) ** 2 - 30) <= _B(4) * (30 + 120) + 2.0 ** -22 * 30
    assert np.array_equal(euclidean(x, x, similarity=True).numpy()[[0, 1, 3], [1, 0, 3]], np.ones(3, dtype=np.float32))


def test_a_zero_vector_is_an_ordinary_point():
    from prograph_amd.distance import euclidean
    rng = np.random.default_rng(8)
    y = rng.standard_normal((20, 11)).astype(np.float16)
    z = np.zeros((1, 11), dtype=np.float16)
    ny = (torch.from_numpy(y).float() ** 2).sum(1)
    assert torch.equal(euclidean(z, y)[:, 0], torch.sqrt(ny))         # d(0, y) = sqrt(ny): (0 + ny) - (0 + 0), torch's own root
    assert torch.equal(euclidean(y, z)[0], torch.sqrt(ny))
    assert np.allclose(euclidean(z, y)[:, 0].numpy(), np.sqrt((y.astype(np.float64) ** 2).sum(1)), rtol=1e-6, atol=0)


def test_no_overflow_beyond_the_fp16_sum_range():
    from prograph_amd.distance import euclidean, minkowski
    x = np.full((1, 16), 4096, dtype=np.float16)
    z = np.zeros((1, 16), dtype=np.float16)
    assert np.isinf(minkowski(torch.from_numpy(x), torch.from_numpy(z)).numpy()).all()
    assert euclidean(x, z).numpy()[0, 0] == 16384.0
    top = np.full((2, 64), 65504, dtype=np.float16)
    top[1] = -top[1]
    g = euclidean(top, top).numpy().astype(np.float64)                # the largest finite fp16 operands
    ref2, bound = _ref2(top, top)
    assert np.all(np.isfinite(g)) and np.all(np.abs(g * g - ref2) <= bound)


def test_operands_are_cleaned_like_the_other_operators():
    from prograph_amd.distance import euclidean
    with pytest.raises(ValueError):
        euclidean(np.zeros((0, 3)), np.ones((2, 3)))
    got = euclidean(np.ones((2, 3)), np.ones((1, 5)))                 # shorter operand right-padded with zeros
    assert got.shape == (1, 2) and np.all(np.abs(got.numpy().astype(np.float64) ** 2 - 2) <= _B(5) * 8 + 2.0 ** -22 * 2)


def _prograph(tmp_path, n, seed=3):
    from prograph_amd import Prograph
    tok = synth.clustered_tokens(n, 8, seed=seed)
    f = tmp_path / "e.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(seed).uniform(0, 1, n)}).to_csv(f)
    return Prograph(file=str(f))


def test_build_graph_and_search_generic_on_cpu(monkeypatch, tmp_path, capsys):
    from prograph_amd.distance import euclidean
    fake_native.install(monkeypatch)
    n, d = 150, 12
    pg = _prograph(tmp_path, n)
    capsys.readouterr()
    rng = np.random.default_rng(4)
    emb = rng.standard_normal((n, d)).astype(np.float16)
    emb[30] = 0
    pg.graph["Embedded"] = list(emb.astype(np.float32))
    ref2, bound = _ref2(emb, emb)
    rowb = bound.max(1)
    k = 6
    t = pg.build_graph(representation="Embedded", k=k, distance=euclidean)
    assert len(t) == n
    order = np.argsort(ref2, axis=1, kind="stable")
    for r, (ix, w) in enumerate(t):
        assert len(ix) == k and w.dtype == np.float32 and r not in ix
        assert np.all(np.diff(w) >= 0)                                 # ascending distances
        assert np.all(np.abs(w.astype(np.float64) ** 2 - ref2[r, ix]) <= bound[r, ix])
        # the returned columns' exact values equal the exact ranks 1..k within twice the bound
        assert np.abs(np.sort(ref2[r, ix]) - ref2[r, order[r, 1:k + 1]]).max() <= 2 * rowb[r]
    ts = pg.build_graph(representation="Embedded", k=k, similarity=True, distance=euclidean)
    for (ix, w), (jx, v) in zip(t, ts):
        assert np.array_equal(ix, jx) and np.all(np.diff(v) <= 0) and np.array_equal(v, 1 / (1 + torch.from_numpy(w)).numpy())
    eps = 3.5
    te = pg.build_graph(representation="Embedded", eps=eps, distance=euclidean)
    # clear of the threshold (whose fp32 rounding moves eps^2 by 2^-23 eps^2 at most) and of 0 by more than the bound
    clear = (np.abs(ref2 - eps * eps) > bound + 2.0 ** -22 * eps * eps) & (ref2 > bound)
    left_out = (~clear).sum() - n                                         # the self pairs are not clear by construction
    print(f"eps graph: {left_out} of {n * n} pairs left out")
    assert left_out <= 0.05 * n * n
    want = ref2 <= eps * eps
    nnz = 0
    for r, (ix, w) in enumerate(te):
        hit = np.zeros(n, dtype=bool)
        hit[ix] = True
        nnz += len(ix)
        assert np.array_equal(hit[clear[r]], want[r][clear[r]]), r
        assert np.all(np.abs(w.astype(np.float64) ** 2 - ref2[r, ix]) <= bound[r, ix]) and np.all(w > 0)
    assert 0 < nnz < n * n // 2
    # queries: rank 0 is kept, min(k, N) ranks, the zero vector is a point like any other
    q = np.concatenate([emb[:5], rng.standard_normal((4, d)).astype(np.float16)])
    q2, qb = _ref2(emb, q)
    res = pg.search(q.astype(np.float32), k=k, distance=euclidean, representation="Embedded")
    qorder = np.argsort(q2, axis=1, kind="stable")
    for r, (ix, w) in enumerate(res):
        assert len(ix) == k and np.all(np.diff(w) >= 0)
        assert np.abs(np.sort(q2[r, ix]) - q2[r, qorder[r, :k]]).max() <= 2 * qb[r].max()
    assert all(res[r][0][0] == r for r in range(5))                    # a query equal to a dataset row has it first
    res = pg.search(q.astype(np.float32), eps=eps, distance=euclidean, representation="Embedded")
    qclear = (np.abs(q2 - eps * eps) > qb + 2.0 ** -22 * eps * eps)
    assert (~qclear).sum() <= 0.05 * q2.size
    for r, (ix, w) in enumerate(res):
        hit = np.zeros(n, dtype=bool)
        hit[ix] = True
        assert np.array_equal(hit[qclear[r]], (q2[r] <= eps * eps)[qclear[r]]), r
    assert all(r in res[r][0] for r in range(5))                       # d = 0 is a hit for queries


def test_euclidean_dispatch(monkeypatch, tmp_path, capsys):
    """build_graph(distance=euclidean) asks `_build_graph_euclidean` for the five orderings only; its None (here: the
    staging is not on a device) leads to the generic loop."""
    import operator
    from prograph_amd.distance import euclidean
    fake_native.install(monkeypatch)
    pg = _prograph(tmp_path, 40)
    capsys.readouterr()
    pg.graph["Embedded"] = list(np.random.default_rng(1).standard_normal((40, 5)).astype(np.float32))
    called = []
    real = type(pg)._build_graph_euclidean

    def spy(self, *a, **k):
        called.append(real(self, *a, **k))
        return called[-1]
    monkeypatch.setattr(type(pg), "_build_graph_euclidean", spy)
    t = pg.build_graph(representation="Embedded", eps=1.5, distance=euclidean, comp=operator.ne)
    assert not called and len(t) == 40
    t = pg.build_graph(representation="Embedded", eps=1.5, distance=euclidean)
    assert called == [None] and len(t) == 40


# ---- containers with final fp32 values, as the Euclidean graphs carry them
INDPTR = np.array([0, 2, 2, 5, 6], dtype=np.int64)
INDICES = np.array([1, 3, 0, 1, 3, 2], dtype=np.int32)
F32 = np.array([0.25, 16384.0, 0.0999, 2.0, 1e-7, 361.33334], dtype=np.float32)
KIDX = np.array([[1, 2], [0, 3], [3, 1], [2, 0]], dtype=np.int32)      # every slot filled (empty ones: test_graph_containers_cpu.py)
KF32 = np.array([[0.5, 7.79], [0.5, 1.25], [1.0, 175.5], [1.0, 0.0]], dtype=np.float32)


@pytest.mark.parametrize("sim", [False, True])
def test_final_graphs_round_trip(tmp_path, sim):
    e = CSRGraph(torch.from_numpy(INDPTR), torch.from_numpy(INDICES), torch.from_numpy(F32), 4, similarity=sim, final=True)
    k = KNNGraph(torch.from_numpy(KIDX), torch.from_numpy(KF32), 4, similarity=sim, final=True)
    p = str(tmp_path / "g.npz")
    save_graphs(p, {"E": e, "K": k}, tokens_fingerprint=7)
    got = load_graphs(p, device="cpu", tokens_fingerprint=7)
    assert got["E"].final and got["K"].final and got["E"].similarity == sim and got["K"].similarity == sim
    assert np.array_equal(got["E"].host()[2], F32) and np.array_equal(got["K"].host()[1], KF32)
    assert np.array_equal(got["E"].host()[0], INDPTR) and np.array_equal(got["K"].host()[0], KIDX)


# ---- the C ABI of the Euclidean entries: present, and argument checks before any launch (no GPU needed)
def test_euclidean_entries_validate_arguments():
    L = _native.lib()
    for name in ("pg_euclidean_dense", "pg_euclidean_knn", "pg_euclidean_knn_round", "pg_euclidean_eps_slots",
                 "pg_euclidean_eps_fill_rows"):
        assert name in _native.SYMBOLS and hasattr(L, name)
    p = ctypes.c_void_p(256)          # never dereferenced: every call below is refused on the host
    ops = [p, p, p, 10, 256, p, p, p, 10, 256, 8]
    rc = L.pg_euclidean_dense(*ops, 0, p, 5, None)                       # ldo < n
    assert rc == -1 and b"pg_euclidean_dense: bad argument" in L.pg_last_error()
    rc = L.pg_euclidean_dense(p, None, p, 10, 256, p, p, p, 10, 256, 8, 0, p, 10, None)
    assert rc == -1 and b"pg_euclidean_dense" in L.pg_last_error()
    rc = L.pg_euclidean_dense(p, p, None, 10, 256, p, p, p, 10, 256, 8, 0, p, 10, None)     # rnorms must still be given
    assert rc == -1 and b"pg_euclidean_dense" in L.pg_last_error()
    rc = L.pg_euclidean_dense(p, p, p, 10, 256, p, p, p, 65535 * 32 + 1, 1 << 22, 8, 0, p, 10, None)
    assert rc == -1 and b"m too large for one launch" in L.pg_last_error()
    rc = L.pg_euclidean_knn(None, p, p, 10, 256, p, p, p, 10, 256, 8, 0, 4, 1, p, p, None)
    assert rc == -1 and b"pg_euclidean_knn: bad argument" in L.pg_last_error()
    rc = L.pg_euclidean_knn(*ops, 0, 60, 5, p, p, None)
    assert rc == -1 and b"pg_euclidean_knn: first + k must be at most 64" in L.pg_last_error()
    rc = L.pg_euclidean_knn(*ops, 0, 0, 1, p, p, None)
    assert rc == -1 and b"first + k" in L.pg_last_error()
    rc = L.pg_euclidean_knn(p, p, p, 10, 100, p, p, p, 10, 256, 8, 0, 4, 1, p, p, None)     # x_npad not a multiple of 256
    assert rc == -1 and b"bad argument" in L.pg_last_error()
    rc = L.pg_euclidean_knn(p, p, p, 10, 256, p, p, p, 300, 256, 8, 0, 4, 1, p, p, None)    # y_npad < m
    assert rc == -1 and b"bad argument" in L.pg_last_error()
    rc = L.pg_euclidean_knn(p, p, p, 10, 256, p, p, p, 10, 256, 0, 0, 4, 1, p, p, None)     # d < 1
    assert rc == -1 and b"bad argument" in L.pg_last_error()
    rc = L.pg_euclidean_knn_round(*ops, 0, 16, None, p, 16, p, p, 16, None)               # no floor
    assert rc == -1 and b"pg_euclidean_knn_round: bad argument" in L.pg_last_error()
    rc = L.pg_euclidean_knn_round(*ops, 0, 16, p, p, 16, p, p, 8, None)                   # ldo < k
    assert rc == -1 and b"pg_euclidean_knn_round: bad argument" in L.pg_last_error()
    rc = L.pg_euclidean_knn_round(*ops, 0, 65, p, p, 16, p, p, 80, None)
    assert rc == -1 and b"pg_euclidean_knn_round: k must be 1..64" in L.pg_last_error()
    rc = L.pg_euclidean_eps_slots(*ops, 0, 0, 0.5, 16, None, p, p, None)
    assert rc == -1 and b"pg_euclidean_eps_slots: bad argument" in L.pg_last_error()
    rc = L.pg_euclidean_eps_slots(*ops, 0, 7, 0.5, 16, p, p, p, None)     # no such comparator
    assert rc == -1 and b"pg_euclidean_eps_slots" in L.pg_last_error()
    rc = L.pg_euclidean_eps_slots(*ops, 0, 0, 0.5, 0, p, p, p, None)      # cap < 1
    assert rc == -1 and b"pg_euclidean_eps_slots" in L.pg_last_error()
    rc = L.pg_euclidean_eps_fill_rows(*ops, 0, 0, 0.5, None, 3, p, p, p, None)
    assert rc == -1 and b"pg_euclidean_eps_fill_rows: bad argument" in L.pg_last_error()
    rc = L.pg_euclidean_eps_fill_rows(*ops, 0, 0, 0.5, p, 0, p, p, p, None)
    assert rc == -1 and b"pg_euclidean_eps_fill_rows" in L.pg_last_error()
    rc = L.pg_euclidean_eps_fill_rows(*ops, 0, 9, 0.5, p, 3, p, p, p, None)
    assert rc == -1 and b"pg_euclidean_eps_fill_rows" in L.pg_last_error()
