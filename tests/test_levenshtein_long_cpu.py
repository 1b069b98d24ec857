"""
Levenshtein beyond 128 positions, without a GPU: the recurrence of pg_lev_long.h as a sanitized host program, the numpy
reference of tests/lev_long_testdata.py pinned against the plain double loop and the C oracle, the argument checks of the
new C entries, and the host logic of the long routes through the stand-in tests/fake_lev_long_native.py.
"""
import ctypes
import operator
import os
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

import fake_lev_long_native as F
import lev_long_testdata as LL
import lev_testdata as LT
from conftest import REPO
from prograph_amd import _native
from prograph_amd.distance import levenshtein


# ---------------------------------------------------------------- 1. the kernel's own functions on the host
def test_recurrence_host_program_under_sanitizers():
    """tests/capi_lev_long: the step, the segment loop, the read-off and the row masks the kernel calls, compiled for
    the host with -fsanitize=address,undefined and run in the kernel's order over boundary lengths x families at every
    instantiated block count, against a plain Wagner-Fischer in C++."""
    capi = os.path.join(REPO, "tests", "capi_lev_long")
    subprocess.check_call(["make", "-s", "-C", capi])
    out = subprocess.run([os.path.join(capi, "_build", "lev_long_check")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "lev_long host check OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert "block counts 1 2 4 8 16" in out.stdout


# ---------------------------------------------------------------- 2. the reference and the set
def test_reference_equals_the_double_loop_and_the_c_oracle():
    X, Y = LL.long_x(), LL.long_y()
    xs = [r for r, l in enumerate(LL.X_LENS) if l <= 260]
    ys = [i for i, l in enumerate(LL.Y_LENS) if l <= 260]
    assert len(xs) >= 25 and len(ys) >= 8
    want = LT.wagner_fischer(X[xs][:, :260], Y[ys][:, :260])
    assert np.array_equal(LL.wagner_fischer_rows(X[xs][:, :260], Y[ys][:, :260]), want)
    assert np.array_equal(LL.long_matrix()[np.ix_(ys, xs)], want)          # the one matrix, where the double loop reaches
    B = LT.set_b()
    assert np.array_equal(LL.wagner_fischer_rows(B, B[::7]), LT.oracle_pairs(B, B[::7]))


def test_long_set_holds_what_the_gpu_tests_need():
    X, Y, D = LL.long_x(), LL.long_y(), LL.long_matrix()
    assert X.shape == (64, 2048) and Y.shape == (13, 2048) and D.shape == (13, 64)
    lx, ly = LT.lengths(X), LT.lengths(Y)
    assert len(set(lx)) == 64 and set(LL.REQUIRED) <= set(lx) and tuple(ly) == LL.Y_LENS
    assert X.max() == 31 and Y.max() == 31
    assert all((r[:l] != 0).all() and not r[l:].any() for r, l in zip(X, lx))
    assert set(LL.x_layout(r)[1] for r in range(64)) == set(LL.FAMILIES)
    assert (D == 0).sum() >= 7 and ((D > 0) & (D <= 8)).sum() >= 10 and (D == 2048).sum() >= 2
    assert D[0, LL.X_LENS.index(2048)] == 2048 and D[12, 0] == 2048          # the empty row against 2048 tokens, both ways
    assert np.array_equal(D[0], lx)                                          # d(empty, x) = len(x)
    assert (np.abs(ly[:, None] - lx[None, :]) <= D).all() and (D <= np.maximum(ly[:, None], lx[None, :])).all()


# ---------------------------------------------------------------- 3. the C ABI
def test_new_c_entries_reject_bad_arguments_without_a_launch():
    lib = _native.lib()
    p = ctypes.c_void_p(16)
    bad = lib.pg_last_error
    dense = lib.pg_levenshtein_long_dense
    assert dense(p, 1, 256, p, 2049, p, 1, 256, p, 128, p, 8, 1, None) == -2 and b"2048" in bad()      # PG_E_TOOLONG
    assert dense(p, 1, 256, p, 128, p, 1, 256, p, 2049, p, 2, 1, None) == -2
    assert dense(None, 1, 256, p, 300, p, 1, 256, p, 300, p, 8, 1, None) == -1                          # NULL pointers
    assert dense(p, 1, 256, None, 300, p, 1, 256, p, 300, p, 8, 1, None) == -1
    assert dense(p, 1, 256, p, 300, None, 1, 256, p, 300, p, 8, 1, None) == -1
    assert dense(p, 1, 256, p, 300, p, 1, 256, None, 300, p, 8, 1, None) == -1
    assert dense(p, 1, 256, p, 300, p, 1, 256, p, 300, None, 8, 1, None) == -1
    assert dense(p, 0, 256, p, 300, p, 1, 256, p, 300, p, 8, 1, None) == -1                             # sizes
    assert dense(p, 1, 256, p, 300, p, 0, 256, p, 300, p, 8, 1, None) == -1
    assert dense(p, 1, 256, p, 0, p, 1, 256, p, 300, p, 8, 1, None) == -1
    assert dense(p, 1, 256, p, 300, p, 1, 256, p, -1, p, 8, 1, None) == -1
    assert dense(p, 1, 255, p, 300, p, 1, 256, p, 300, p, 8, 1, None) == -1                             # npad
    assert dense(p, 2, 256, p, 300, p, 1, 256, p, 300, p, 8, 1, None) == -1                             # ldo < n
    assert dense(p, 1, 256, p, 300, p, 1, 256, p, 300, p, 4, 1, None) == -1 and b"2 or 8" in bad()      # int32 output: no
    pack = lib.pg_lev_long_pack
    assert pack(p, 1, 2049, 2049, p, 256, p, p, None) == -2
    assert pack(None, 1, 300, 300, p, 256, p, p, None) == -1 and pack(p, 1, 300, 300, p, 256, p, None, None) == -1
    assert pack(p, 0, 300, 300, p, 256, p, p, None) == -1 and pack(p, 1, 300, 299, p, 256, p, p, None) == -1
    assert pack(p, 1, 300, 300, p, 100, p, p, None) == -1
    # the one-word kernel keeps its limit
    assert lib.pg_levenshtein_dense(p, 1, 256, p, p, 1, 256, p, 129, p, 8, 1, None) == -1 and b"1..128" in bad()
    assert _native.LEV_LONG_MAX_L == 2048 and lib.pg_version() == 3


# ---------------------------------------------------------------- 4. host routing through the stand-in
def _prograph(tmp_path, tok):
    from prograph_amd import Prograph
    f = tmp_path / "long.pkl"
    seqs = LL.strings(tok)
    pd.DataFrame({"Sequence": seqs, "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_pickle(str(f))
    P = Prograph(file=str(f), seed_seq=seqs[-1], amino_acids=LL.ALPHABET)
    width = int(LT.lengths(tok).max())
    assert np.array_equal(P.tokenized, tok[:, :width])
    return P


def _rows_upto(width, step=1):
    rows = [r for r, l in enumerate(LL.X_LENS) if l <= width]
    rows = rows[::step] + ([rows[-1]] if (len(rows) - 1) % step else [])
    assert LL.X_LENS[rows[-1]] == width
    return LL.long_x()[rows][:, :width]


def _names():
    return [c[0] for c in F.calls]


def _same_tuples(got, want_idx, want_w, wdtype=np.int64):
    assert len(got) == len(want_idx)
    for (gi, gw), wi, ww in zip(got, want_idx, want_w):
        assert len(gi) == len(wi)
        if len(wi):
            assert gi.dtype == np.int64 and gw.dtype == wdtype
        assert np.array_equal(gi, wi) and np.array_equal(gw, ww)


@pytest.mark.parametrize("width, step", [(129, 1), (2048, 4)])
def test_long_widths_reach_the_long_entry(tmp_path, monkeypatch, width, step):
    F.install(monkeypatch)
    tok = _rows_upto(width, step)
    n = len(tok)
    P = _prograph(tmp_path, tok)
    D = LL.wagner_fischer_rows(tok, tok)
    # the operator (device tokens: the stand-in has none, so the question is patched)
    import sys
    mod = sys.modules["prograph_amd.distance.levenshtein"]
    monkeypatch.setattr(mod, "_on_device", lambda t: True)
    monkeypatch.setattr(mod, "_torch_levenshtein", None)
    del F.calls[:]
    d = levenshtein(torch.from_numpy(tok), torch.from_numpy(tok[:5]))
    assert d.dtype == torch.int64 and np.array_equal(d.numpy(), D[:5])
    assert F.calls == [("long_operand", n, width), ("long_operand", 5, width), ("long_dense", 5, 8)]
    # kNN graphs: fp16 blocks, ranks from 1, int16 weights; rounds beyond 63 are the selection's business
    for k in (1, 5, n + 3):
        del F.calls[:]
        G = P.build_graph(k=k, distance=levenshtein, output="csr")
        kk = min(k, n - 1)
        assert F.calls == [("long_operand", n, width), ("long_dense", n, 2), ("f16_knn", kk, 1, False)]
        wi, wd = LL.knn_from_matrix(D, kk, 1)
        assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.first == 1
        assert np.array_equal(G.idx.numpy(), wi) and np.array_equal(G.dist.numpy(), wd)
    _same_tuples(P.build_graph(k=4, distance=levenshtein), *LL.knn_from_matrix(D, 4, 1, np.int64))
    sim = P.build_graph(k=4, distance=levenshtein, similarity=True)
    _same_tuples(sim, LL.knn_from_matrix(D, 4, 1)[0], (1 / (1 + torch.from_numpy(LL.knn_from_matrix(D, 4, 1, np.int64)[1]))).numpy(),
                 np.float32)
    # eps graphs: every comparator on the fp16 selection, d > 0 only; nothing in 1..thr is the empty graph without a launch
    mid = int(np.median(D))
    for comp, eps, thr in (("le", 8, 8.0), ("le", 8.5, 8.0), ("lt", 9, 9.0), ("eq", mid, float(mid)), ("ge", mid, float(mid)),
                           ("gt", mid + 0.5, float(mid)), ("le", 3000, 3000.0),
                           ("eq", 2.5, None), ("le", 0.5, None), ("lt", 1, None)):
        del F.calls[:]
        G = P.build_graph(eps=eps, distance=levenshtein, comp=LT.OPS[comp], output="csr")
        ip, ix, w = LL.csr_from_matrix(D, LT.OPS[comp], eps)
        assert np.array_equal(G.indptr.numpy(), ip) and np.array_equal(G.indices.numpy(), ix) and np.array_equal(G.weights.numpy(), w), (comp, eps)
        assert G.indices.dtype == torch.int32 and G.weights.dtype == torch.int16 and G.indptr.dtype == torch.int64
        if thr is None:
            assert F.calls == [("long_operand", n, width)] and ip[-1] == 0, (comp, eps, F.calls)
        else:
            assert F.calls == [("long_operand", n, width), ("long_dense", n, 2),
                               ("f16_eps", _native.CMP_LE + ("le", "lt", "eq", "ge", "gt").index(comp), thr, False)], (comp, eps, F.calls)
    assert "eps" not in _names() and "banded_knn" not in _names() and "dense" not in _names()
    # search: rank 0 / d = 0 kept, int16 weights
    q = np.zeros((3, width), dtype=np.uint8)
    q[0, :5] = tok[3, :5]
    q[1] = tok[n - 1]
    q[2, :width - 1] = tok[n - 1, 1:]
    DQ = LL.wagner_fischer_rows(tok, q)
    del F.calls[:]
    G = P.search(q, k=4, distance=levenshtein, output="csr")
    assert F.calls == [("long_operand", n, width), ("long_operand", 3, width), ("long_dense", 3, 2), ("f16_knn", 4, 0, False)]
    wi, wd = LL.knn_from_matrix(DQ, 4, 0)
    assert G.first == 0 and G.dist.dtype == torch.int16 and np.array_equal(G.idx.numpy(), wi) and np.array_equal(G.dist.numpy(), wd)
    assert wd[1, 0] == 0
    del F.calls[:]
    G = P.search(LL.strings(q), eps=6, distance=levenshtein, output="csr")
    assert _names() == ["long_operand", "long_operand", "long_dense", "f16_eps"] and F.calls[-1] == ("f16_eps", _native.CMP_LE, 6.0, True)
    ip, ix, w = LL.csr_from_matrix(DQ, operator.le, 6, keep_zero=True)
    assert ip[-1] >= 2 and w.min() == 0
    assert np.array_equal(G.indptr.numpy(), ip) and np.array_equal(G.indices.numpy(), ix) and np.array_equal(G.weights.numpy(), w)
    assert G.weights.dtype == torch.int16
    rows, dmin = P.nearest_neighbour(LL.strings(q)[2], distance=levenshtein)
    assert list(rows.index) == [int(wi[2, 0])] and dmin == wd[2, 0]
    hood = P.neighbourhood(LL.strings(q)[1], 6, distance=levenshtein)
    assert list(hood.index) == list(ix[ip[1]:ip[2]])
    assert np.array_equal(P.calc_neighbours(LL.strings(q)[1], eps=2, distance=levenshtein, comp=operator.le), np.nonzero(DQ[1] <= 2)[0])


def test_unequal_widths_reach_the_long_entry_from_search(tmp_path, monkeypatch):
    F.install(monkeypatch)
    narrow, wide = _rows_upto(128), _rows_upto(2048, 4)
    wide_q = np.ascontiguousarray(LL.long_y()[[9, 12]])                      # 1024 and 2048 tokens
    narrow_q = np.ascontiguousarray(LL.long_y()[[1, 3]][:, :128])            # 1 and 128 tokens
    P = _prograph(tmp_path, narrow)
    del F.calls[:]
    got = P.search(LL.strings(wide_q), k=3, distance=levenshtein)            # a wide query against a narrow dataset
    assert F.calls == [("long_operand", len(narrow), 128), ("long_operand", 2, 2048), ("long_dense", 2, 2), ("f16_knn", 3, 0, False)]
    _same_tuples(got, *LL.knn_from_matrix(LL.wagner_fischer_rows(narrow, wide_q), 3, 0, np.int64))
    del F.calls[:]
    got = P.search(wide_q, eps=1030, distance=levenshtein, comp=operator.lt)
    assert F.calls[-1] == ("f16_eps", _native.CMP_LT, 1030.0, True) and "long_dense" in _names()
    ip, ix, w = LL.csr_from_matrix(LL.wagner_fischer_rows(narrow, wide_q), operator.lt, 1030, keep_zero=True)
    assert 0 < ip[1] and ip[2] == ip[1]
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    P = _prograph(tmp_path, wide)
    del F.calls[:]
    got = P.search(LL.strings(narrow_q), k=2, distance=levenshtein)          # a narrow query against a wide dataset
    assert F.calls == [("long_operand", len(wide), 2048), ("long_operand", 2, 128), ("long_dense", 2, 2), ("f16_knn", 2, 0, False)]
    _same_tuples(got, *LL.knn_from_matrix(LL.wagner_fischer_rows(wide, narrow_q), 2, 0, np.int64))


def test_width_128_makes_exactly_the_calls_it_made(tmp_path, monkeypatch):
    F.install(monkeypatch)
    tok = _rows_upto(128)
    n = len(tok)
    P = _prograph(tmp_path, tok)
    D = LT.pair_matrix(tok, tok)
    del F.calls[:]
    G = P.build_graph(k=3, distance=levenshtein, output="csr")
    far = int((LT.knn_from_matrix(D, 3, 1)[1][:, 2] > 8).sum())
    assert 0 < far < n and F.calls == [("banded_knn", n), ("dense", far), ("f16_knn", 3, 1, False)]
    assert G.dist.dtype == torch.uint8 and np.array_equal(G.idx.numpy(), LT.knn_from_matrix(D, 3, 1)[0])
    del F.calls[:]
    G = P.build_graph(eps=3, distance=levenshtein, output="csr")
    assert F.calls == [("eps", n)] and G.weights.dtype == torch.uint8
    del F.calls[:]
    G = P.build_graph(eps=20, distance=levenshtein, output="csr")
    assert F.calls == [("dense", n), ("f16_eps", _native.CMP_LE, 20.0, False)] and G.weights.dtype == torch.uint8
    del F.calls[:]
    G = P.search(tok[:4], k=2, distance=levenshtein, output="csr")
    assert F.calls == [("dense", 4), ("f16_knn", 2, 0, False)] and G.dist.dtype == torch.uint8
    import sys
    mod = sys.modules["prograph_amd.distance.levenshtein"]
    monkeypatch.setattr(mod, "_on_device", lambda t: True)
    del F.calls[:]
    d = levenshtein(torch.from_numpy(tok), torch.from_numpy(tok[:4]))
    assert F.calls == [("dense", 4)] and np.array_equal(d.numpy(), D[:4])


def test_what_the_long_kernel_does_not_take_stays_where_it_was(tmp_path, monkeypatch):
    F.install(monkeypatch)
    tok = _rows_upto(129)
    n = len(tok)
    P = _prograph(tmp_path, tok)
    rng = np.random.default_rng(9)

    def rows(width, lens):
        T = np.zeros((len(lens), width), dtype=np.int64)
        for r, l in zip(T, lens):
            r[:l] = rng.integers(1, 32, l)
        return T
    too_wide = rows(2049, (2049, 2040, 5, 0, 300))
    token32 = rows(200, (200, 150, 129, 3, 0))
    token32[1, 140] = 32
    interior = rows(200, (200, 150, 129, 3, 0))
    interior[0, 130] = 0
    import sys
    mod = sys.modules["prograph_amd.distance.levenshtein"]
    for name, T in (("TooWide", too_wide), ("Token32", token32), ("Interior", interior)):
        P.graph[name] = list(T[:1]) * (n - len(T)) + list(T)
        sub = np.arange(n - len(T), n)
        want = np.asarray(mod._torch_levenshtein(torch.from_numpy(T.astype(np.uint8)), torch.from_numpy(T.astype(np.uint8))))
        if name != "Interior":
            assert np.array_equal(want, LL.wagner_fischer_rows(T, T))
        del F.calls[:]
        got = P.build_graph(k=2, distance=levenshtein, representation=name, idxs=sub)
        assert "long_dense" not in _names() and "dense" not in _names() and "f16_knn" not in _names(), (name, F.calls)
        wi, wd = LL.knn_from_matrix(want, 2, 1, np.int64)
        _same_tuples(got, wi, wd)
        del F.calls[:]
        got = P.search(T[:2], k=2, distance=levenshtein, representation=name)
        assert "long_dense" not in _names() and "dense" not in _names(), (name, F.calls)
        # the operator: the torch expression, whatever the device question says
        monkeypatch.setattr(mod, "_on_device", lambda t: True)
        del F.calls[:]
        d = levenshtein(torch.from_numpy(T), torch.from_numpy(T[:3]))
        assert np.array_equal(d.numpy(), want[:3]) and "long_dense" not in _names() and "dense" not in _names()
        monkeypatch.setattr(mod, "_on_device", lambda t: t.is_cuda)
    # no device: the long routes are not taken at all
    F.install(monkeypatch, ready=False)
    del F.calls[:]
    got = P.build_graph(k=2, distance=levenshtein)
    assert not F.calls
    _same_tuples(got, *LL.knn_from_matrix(LL.wagner_fischer_rows(tok, tok), 2, 1, np.int64))
    assert P.search(tok[:2], k=1, distance=levenshtein)[1][0][0] == 1 and not F.calls
