"""
The plan of the symmetric kNN sweep as the device computes it (pg_api.hip: sym_plan_workgroup): a thread's
blocks counted once and kept in a register (up to four a thread, 262 144 rows), a scan of wave scans behind one barrier -
and, behind a probe, the plan's workgroups riding in pg_decide_kernel's launch instead of a launch of their own.

pg_knn_sym_plan_device against the host's pg_knn_sym_plan word for word (the entries, the first pass of every block, the
number of passes) at row counts that give a thread one block, four, five and 256; then the riding plan at the smallest probed
launch and above it, on a workspace poisoned with 0xEE: the forced sweep against the rectangular path byte for byte and
against the C oracle on rows at the start, the middle and the end.
"""
import ctypes

import numpy as np
import pytest
import torch

import knn_sym_testdata as D

pytestmark = pytest.mark.gpu

NS = (1, 64, 65, 129, 3000, 65536, 70001, 200000, 262145, 1 << 24)


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def host_plan(lib, n, slots, piece):
    count = lib.pg_knn_sym_plan(n, slots, piece, 0, None, 0)
    out = np.zeros((count, 4), dtype=np.int32)
    assert lib.pg_knn_sym_plan(n, slots, piece, 0, out.ctypes.data_as(ctypes.c_void_p), count) == count
    return out


@pytest.mark.parametrize("n", NS)
def test_device_plan_equals_host_plan(nat, n):
    """one block a thread (n <= 65 536), four (262 144 rows), five (the counts are recomputed) and 256; few slots (long
    pieces) and many; the guided rule and fixed pieces of 3 (sixteen a block) and 500 super-tiles"""
    lib = nat.lib()
    dev = nat.device()
    nb = (n + 63) // 64
    for slots in (8, 4096):
        for piece in (0, 3, 500):
            want = host_plan(lib, n, slots, piece)
            count = len(want)
            assert np.array_equal(np.unique(want[:, 0]), np.arange(nb))
            start = np.concatenate([np.searchsorted(want[:, 0], np.arange(nb)), [count]]).astype(np.uint32)
            plan = torch.full((count + 8, 4), -7, dtype=torch.int32, device=dev)
            first = torch.full((nb + 1 + 8,), 0x7777, dtype=torch.int32, device=dev)
            got = lib.pg_knn_sym_plan_device(n, slots, piece, 0, nat._ptr(plan), nat._ptr(first), count, nat._stream())
            assert got == count, (n, slots, piece, got, lib.pg_last_error())
            torch.cuda.synchronize()
            plan, first = plan.cpu().numpy(), first.cpu().numpy()
            assert np.array_equal(plan[:count], want), (n, slots, piece)
            assert (plan[count:] == -7).all(), (n, slots, piece, "entries behind the plan")
            assert np.array_equal(first[:nb + 1].view(np.uint32), start), (n, slots, piece)
            assert (first[nb + 1:] == 0x7777).all(), (n, slots, piece, "words behind pieceStart")


def test_a_plan_that_does_not_fit_is_declined(nat):
    """one entry short: an error, and nothing is written"""
    lib = nat.lib()
    count = lib.pg_knn_sym_plan(3000, 4096, 3, 0, None, 0)
    plan = torch.full((count, 4), -7, dtype=torch.int32, device=nat.device())
    first = torch.full((48,), 0x7777, dtype=torch.int32, device=nat.device())
    assert lib.pg_knn_sym_plan_device(3000, 4096, 3, 0, nat._ptr(plan), nat._ptr(first), count - 1, nat._stream()) != count
    torch.cuda.synchronize()
    assert (plan.cpu().numpy() == -7).all() and (first.cpu().numpy() == 0x7777).all()


# ---------------------------------------------------------------------------------------------------------------------
# the plan riding in the probe's decision launch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probed(nat):
    """n -> [tokens, planes, the rectangular path's result]: clusters of 100, the probe's "clustered" verdict"""
    from prograph_amd import synth
    out = {}
    for n in (65536, 70001):
        tok = np.ascontiguousarray(synth.clustered_tokens(n, 64, seed=2100 + n % 97, members=100))
        out[n] = [tok, nat.pack(torch.from_numpy(tok), bits=5), None]
    return out


@pytest.fixture
def poisoned_workspace(nat, monkeypatch):
    """every workspace of a call comes filled with 0xEE: what the plan's workgroups do not write is not zero by chance"""
    for v in ("PG_ENGINE", "PG_ENGINE_MIN_ROWS", "PG_PROBE", "PG_PROBE_S", "PG_PROBE_W", "PG_KNN_GUESS", "PG_GATE_FORCE", "PG_MM_R", "PG_KNN_SYM"):
        monkeypatch.delenv(v, raising=False)
    seen = []

    def poisoned(nrows, dev):
        ws = torch.full((int(nat.lib().pg_workspace_bytes(int(nrows))),), 0xEE, dtype=torch.uint8, device=dev)
        seen.append(ws)
        return ws
    monkeypatch.setattr(nat, "workspace", poisoned)
    return seen


def run(nat, monkeypatch, capfd, planes, env):
    monkeypatch.setenv("PG_DEBUG_PLAN", "1")
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    capfd.readouterr()
    idx, dist = [x.cpu().numpy() for x in nat.knn_graph(planes, planes, 16)]
    err = capfd.readouterr().err
    for key in env:
        monkeypatch.delenv(key)
    return idx, dist, err


def rectangular(nat, monkeypatch, capfd, probed, n):
    """the PG_KNN_SYM=0 result, held to the C oracle on 128 rows at the start, the middle and the end; once per n"""
    tok, planes, ref = probed[n]
    if ref is None:
        idx, dist, err = run(nat, monkeypatch, capfd, planes, {"PG_KNN_SYM": "0"})
        assert "[pg plan sym]" not in err
        from oracle import c_oracle as Co
        for r0 in (0, n // 2, n - 128):
            oidx, odist = Co.knn(tok, 16, row0=r0, nrows=128, fast=True)
            assert np.array_equal(idx[r0:r0 + 128], oidx) and np.array_equal(dist[r0:r0 + 128], odist), (n, r0)
        ref = probed[n][2] = (idx, dist)
    return ref


@pytest.mark.parametrize("n", [65536, 70001])
@pytest.mark.parametrize("route", ["rides", "launched"])
def test_forced_sweep_with_the_plan_in_the_decide_launch(nat, monkeypatch, capfd, probed, poisoned_workspace, n, route):
    """PG_KNN_SYM=1 behind the probe: the plan rides; PG_PROBE=0: the plan kernel is a launch of its own.  The eviction limit
    out of reach: what is compared is the sweep's and the merge's own output, which a wrong plan entry, a wrong first pass
    of a block or a count of delivered keys left at 0xEEEEEEEE would spoil.  Twice in a row, fresh poisoned workspaces."""
    ridx, rdist = rectangular(nat, monkeypatch, capfd, probed, n)
    env = {"PG_KNN_SYM": "1", "PG_KNN_SYM_EVICT_LIMIT": D.OUT_OF_REACH}
    if route == "launched":
        env["PG_PROBE"] = "0"
    for _ in range(2):
        idx, dist, err = run(nat, monkeypatch, capfd, probed[n][1], env)
        assert f"[pg plan sym] rows={n}:" in err, err
        assert ("plan rides in the decide launch" in err) == (route == "rides"), err
        assert idx.tobytes() == ridx.tobytes() and dist.tobytes() == rdist.tobytes(), (n, route)


@pytest.mark.parametrize("n", [65536, 70001])
@pytest.mark.parametrize("force", ["1", "4"])
def test_plan_workgroups_run_while_the_probe_sends_the_launch_elsewhere(nat, monkeypatch, capfd, probed, poisoned_workspace, n, force):
    """the decision is forced to the VALU engine (1) and to the 32-row alternative's word (4): sweep and merge leave at their
    gate, the plan's workgroups ran all the same, the result is the rectangular path's"""
    ridx, rdist = rectangular(nat, monkeypatch, capfd, probed, n)
    idx, dist, err = run(nat, monkeypatch, capfd, probed[n][1], {"PG_KNN_SYM": "1", "PG_GATE_FORCE": force})
    assert f"[pg plan sym] rows={n}:" in err and "plan rides in the decide launch" in err, err
    assert idx.tobytes() == ridx.tobytes() and dist.tobytes() == rdist.tobytes(), (n, force)
