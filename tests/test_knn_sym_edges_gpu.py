"""
The symmetric kNN sweep (pg_mm_knn_sym_kernel, pg_knn_sym_merge_kernel, pg_knn_sym_decide_kernel) at its
seams: the cap (delivery d < cap, eviction at rank-k distance >= cap), the slot of delivered keys (cnt == capL kept, capL + 1
evicted; 8 and the production 256), sixteen lists a row, one group and two (L = 1 .. 64, multiples of 32 and not), graphs of
1 .. 64 rows, the 32-row rectangular kernel gated behind the sweep, and the routes that must decline it.  The inputs are
tests/knn_sym_testdata.py's, pinned to their seams without a GPU by tests/test_knn_sym_edges_cpu.py.

Every entry of (indices, distances) against the C oracle AND byte for byte against the rectangular path (PG_KNN_SYM=0) in
the same process, PG_ENGINE=mfma throughout.  Every call runs with PG_DEBUG_PLAN=1 and is held to the planner's line:
"[pg plan sym] rows=N:" present for the forced call, absent for PG_KNN_SYM=0 - a launch that quietly declined the sweep
would compare the rectangular path with itself.
"""
import numpy as np
import pytest
import torch

import knn_sym_testdata as D
from test_knn_sym_gpu import case as clustered_case

FAR = {"PG_KNN_SYM_EVICT_LIMIT": D.OUT_OF_REACH}             # only the merge and pg_knn_rows_kernel write the result


def oracle(tok, ks, fast=False):
    from oracle import c_oracle as Co
    return {k: Co.knn(tok, k, fast=fast) for k in ks}


def launch(monkeypatch, capfd, rows, cols, k, sym, env):
    """one knn_graph call under `env` -> (indices, distances, the call took the symmetric path)"""
    from prograph_amd import _native as nat
    monkeypatch.setenv("PG_ENGINE", "mfma")
    monkeypatch.setenv("PG_DEBUG_PLAN", "1")
    monkeypatch.setenv("PG_MM_R", "2")
    monkeypatch.setenv("PG_KNN_SYM", sym)
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    capfd.readouterr()
    idx, dist = [x.cpu().numpy() for x in nat.knn_graph(rows, cols, k)]
    err = capfd.readouterr().err
    for key in env:
        monkeypatch.delenv(key)
    line = f"[pg plan sym] rows={rows.n}:"
    assert ("[pg plan sym]" in err) == (line in err), err
    return idx, dist, line in err


def check(monkeypatch, capfd, tok, ref, envs, bits=5):
    """every k of `ref` under every env: the forced call takes the sweep and equals the oracle and the rectangular call"""
    from prograph_amd import _native as nat
    planes = nat.pack(torch.from_numpy(tok), bits=bits)
    for k, (oidx, odist) in ref.items():
        for env in envs:
            ridx, rdist, took = launch(monkeypatch, capfd, planes, planes, k, "0", env)
            assert not took, (k, env, "PG_KNN_SYM=0 took the symmetric path")
            idx, dist, took = launch(monkeypatch, capfd, planes, planes, k, "1", env)
            assert took, (k, env, "the forced call did not take the symmetric path")
            bad = np.flatnonzero((idx != oidx).any(axis=1) | (dist != odist).any(axis=1))
            assert bad.size == 0, (tok.shape, k, env, "oracle: rows", bad[:8], idx[bad[:2]], oidx[bad[:2]], dist[bad[:2]], odist[bad[:2]])
            assert idx.tobytes() == ridx.tobytes() and dist.tobytes() == rdist.tobytes(), (tok.shape, k, env, "rectangular path")


@pytest.mark.gpu
@pytest.mark.parametrize("l", D.WIDTHS)
@pytest.mark.parametrize("n", D.WIDTH_NS)
def test_group_counts_and_widths(monkeypatch, capfd, n, l):
    """G = 1 (L <= 32: 32 plane-0 bits of signature, cap 7) and G = 2 (cap 10) at widths that fill a group and that do not.
    L <= 5: every pair is below the cap - the dense form, rows from 257 on overflow the production slot.  First what the
    merge and pg_knn_rows_kernel write, then the default limit (N / 16 evicted rows: dense data fall back)."""
    tok = D.width_case(n, l)
    check(monkeypatch, capfd, tok, oracle(tok, D.WIDTH_KS), (FAR, {}))


@pytest.mark.gpu
@pytest.mark.parametrize("order", D.ORDERS)
@pytest.mark.parametrize("l", [64, 32])
def test_cap_seams(monkeypatch, capfd, l, order):
    """ladders: rows with rank-k distance one below the cap, at it and above it (test_cap_seams_of_the_ladders), their
    neighbours at distance cap - 1 delivered and at distance cap not.  Default cap (10 / 7), a cap of 3 and one above every
    distance; limit out of reach, then the default one."""
    tok, _ = D.ladder_case(l, order)
    c = D.CAPS[l]
    ref = oracle(tok, sorted(set(D.cap_ks(c) + D.cap_ks(3))))
    own = {k: ref[k] for k in D.cap_ks(c)}
    check(monkeypatch, capfd, tok, own, (FAR, {}))
    check(monkeypatch, capfd, tok, ref, ({"PG_KNN_GUESS": "3", **FAR}, {"PG_KNN_GUESS": "3"}))
    check(monkeypatch, capfd, tok, own, ({"PG_KNN_GUESS": "65", **FAR}, {"PG_KNN_GUESS": "65"}))


@pytest.mark.gpu
@pytest.mark.parametrize("size,stride", D.SLOT8_CLUSTERS)
def test_slots_of_eight_at_the_seam(monkeypatch, capfd, size, stride):
    """identical rows: member 8 holds exactly 8 delivered keys and needs every one, member 9 overflows; stride 2: the slot
    behind an overflowing one is kept and read by a row of the other cluster"""
    tok, _, _ = D.duplicates(D.SLOT8_N, size, stride)
    check(monkeypatch, capfd, tok, oracle(tok, D.SLOT8_KS), ({"PG_KNN_SYM_CAPL": "8", **FAR},))


@pytest.mark.gpu
def test_the_production_slot_at_the_seam(monkeypatch, capfd):
    """300 identical rows: members 255, 256 (exactly full: all 256 keys packed into the merge's LDS array) and 257 (evicted)"""
    tok, _, _ = D.duplicates(D.SLOT256_N, D.SLOT256_SIZE, 1, start=D.SLOT256_START)
    check(monkeypatch, capfd, tok, oracle(tok, D.SLOT256_KS), (FAR, {}))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["strided256", "contiguous"])
@pytest.mark.parametrize("shape", [D.PIECES_16, D.PIECES_17], ids=["sixteen", "seventeen_clamped"])
def test_sixteen_pieces(monkeypatch, capfd, shape, kind):
    """a block's sixteen lists, one per lane of a row's group in the merge (test_sixteen_pieces_and_the_clamp)"""
    n, piece = shape
    tok, ref = clustered_case(n, kind)
    check(monkeypatch, capfd, tok, {k: ref[k] for k in D.PIECES_KS}, ({"PG_KNN_SYM_PIECE": piece},))


@pytest.mark.gpu
@pytest.mark.parametrize("l", D.TINY_LS)
@pytest.mark.parametrize("n", D.TINY_NS)
def test_tiny_graphs(monkeypatch, capfd, n, l):
    """one block, a last group of the merge with fewer than four rows, N < k + 1: the ranks that do not exist read -1 / 255"""
    tok = D.tiny_case(n, l)
    ref = oracle(tok, D.TINY_KS)
    assert (ref[19][0][:, n - 1:] == -1).all() and (ref[19][1][:, n - 1:] == 255).all()
    check(monkeypatch, capfd, tok, ref, (FAR, {}))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["strided12", "strided64"])
def test_32_row_rectangular_kernel_behind_the_sweep(monkeypatch, capfd, kind):
    """PG_MM_R=1: the sweep in front, the 32-row instance gated behind it.  Limit 0: it runs; out of reach: it never does;
    default: clusters of 12 lose the cap in every row (it runs), clusters of 64 stay"""
    tok, ref = clustered_case(1000, kind)
    envs = [{"PG_MM_R": "1", **extra} for extra in ({"PG_KNN_SYM_EVICT_LIMIT": "0"}, {}, FAR)]
    check(monkeypatch, capfd, tok, {16: ref[16], 19: ref[19]}, envs)


@pytest.mark.gpu
def test_three_runs_are_byte_identical(monkeypatch, capfd):
    """delivery goes through atomics in arbitrary order; the result does not depend on it"""
    from prograph_amd import _native as nat
    tok, ref = clustered_case(3000, "contiguous")
    planes = nat.pack(torch.from_numpy(tok), bits=5)
    runs = [launch(monkeypatch, capfd, planes, planes, 19, "1", FAR) for _ in range(3)]
    assert all(took for _, _, took in runs)
    for idx, dist, _ in runs:
        assert idx.tobytes() == runs[0][0].tobytes() and dist.tobytes() == runs[0][1].tobytes()
    assert np.array_equal(runs[0][0], ref[19][0]) and np.array_equal(runs[0][1], ref[19][1])


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["k20", "bits8", "L70", "guess0", "two_buffers"])
def test_declined_routes(monkeypatch, capfd, route):
    """PG_KNN_SYM=1 and the sweep must not run: k + 1 > PG_MM_KL, 8-bit planes, four chunks (G = 3), no optimistic cap, rows
    and columns in two buffers of equal content.  No planner line, and the oracle's result."""
    from prograph_amd import _native as nat
    from prograph_amd import synth
    l = 70 if route == "L70" else 64
    tok = np.ascontiguousarray(synth.clustered_tokens(1000, l, seed=4100 + l, members=64))
    tok[3] = tok[998]
    tok[500] = D.filler(1, l, 41)[0]
    k = 20 if route == "k20" else 16
    rows = nat.pack(torch.from_numpy(tok), bits=8 if route == "bits8" else 5)
    cols = nat.pack(torch.from_numpy(tok.copy()), bits=5) if route == "two_buffers" else rows
    assert (cols.buf.data_ptr() != rows.buf.data_ptr()) == (route == "two_buffers")
    oidx, odist = oracle(tok, (k,))[k]
    base = {"PG_KNN_GUESS": "0"} if route == "guess0" else {}
    for env in (base, {**base, **FAR}):
        idx, dist, took = launch(monkeypatch, capfd, rows, cols, k, "1", env)
        assert not took, (route, "took the symmetric path")
        assert np.array_equal(idx, oidx) and np.array_equal(dist, odist), route
    if route in ("L70", "bits8"):                            # the same data where the route is open: the line is there
        return
    planes = nat.pack(torch.from_numpy(tok), bits=5)
    assert launch(monkeypatch, capfd, planes, planes, 16, "1", FAR)[2]
