"""
The symmetric kNN sweep without a GPU: the pass plan through its C entry (pg_knn_sym_plan: a host function),
the hot loop's census and the fragment-ring rule of the new kernel on the generated ISA (the tools' --kernel option), and the
kernel's presence in the library.
"""
import ctypes
import heapq
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "_Z20pg_mm_knn_sym_kernel"
SLOTS = 256 * 4 * 4                                          # MI355X: 256 CUs x 4 SIMDs x 4 waves (the instance's occupancy)


def plan(n, slots, piece=0, piece_min=0):
    from prograph_amd import _native
    lib = _native.lib()
    count = lib.pg_knn_sym_plan(n, slots, piece, piece_min, None, 0)
    out = np.zeros((count, 4), dtype=np.int32)
    assert lib.pg_knn_sym_plan(n, slots, piece, piece_min, out.ctypes.data_as(ctypes.c_void_p), count) == count
    return out


def covered_once(n, p):
    """every (row block, super-tile at or beyond the block's own) exactly once; no piece empty; inner boundaries even"""
    nb, nst = (n + 63) // 64, (n + 127) // 128
    assert (p[:, 2] > p[:, 1]).all()
    seen = np.zeros((nb, nst), dtype=np.int32)
    for b, first, end, q in p:
        assert 0 <= b < nb and b // 2 <= first and end <= nst
        seen[b, first:end] += 1
        assert first == b // 2 or first % 2 == 0
    want = np.arange(nst)[None, :] >= (np.arange(nb) // 2)[:, None]
    assert np.array_equal(seen, want.astype(np.int32))
    for b in range(nb):                                      # a block's pieces: consecutive passes, numbered from 0, in column order
        mine = p[p[:, 0] == b]
        assert list(mine[:, 3]) == list(range(len(mine))) and (np.diff(mine[:, 1]) > 0).all()
        assert len(mine) <= 16


@pytest.mark.parametrize("n", [1, 64, 65, 128, 129, 193, 1000, 3000, 70001])
@pytest.mark.parametrize("piece", [0, 3, 4, 12, 500])
def test_plan_covers_the_triangle_exactly_once(n, piece):
    for slots in (8, SLOTS):
        covered_once(n, plan(n, slots, piece))


def test_pieces_the_gpu_tests_count_on():
    p = plan(3000, SLOTS, 12)
    assert (p[:, 0] == 0).sum() == 2                         # 24 super-tiles in pieces of 12
    p = plan(3000, SLOTS, 3)
    assert max((p[:, 0] == b).sum() for b in range(47)) == 8 and (p[:, 0] == 6).sum() == 7   # 21 super-tiles in pieces of 3
    assert (plan(1000, SLOTS, 4)[:, 0] == 0).sum() == 2


@pytest.mark.parametrize("n", [200_000, 131_073, 150_000, 270_000])
@pytest.mark.parametrize("slots", [256 * 4 * 3, SLOTS])
def test_modelled_makespan_within_ten_percent_of_the_mean(n, slots):
    """greedy assignment of the emitted order to `slots` waves, cost = super-tile visits"""
    p = plan(n, slots)
    cost = (p[:, 2] - p[:, 1]).astype(np.int64)
    waves = [0] * slots
    heapq.heapify(waves)
    for c in cost:
        heapq.heappush(waves, heapq.heappop(waves) + int(c))
    mean = cost.sum() / slots
    print(f"n={n} slots={slots}: {len(p)} passes, makespan {max(waves)} = {max(waves) / mean:.3f} x mean")
    assert max(waves) <= 1.10 * mean
    covered_once(n, p)


def test_census_and_ring_rule_of_the_symmetric_kernel():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_scan_loop.py"), "2", "--json", "--kernel", SYM],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(report) == 1
    (name, c), = report.items()
    assert name.startswith(SYM)
    assert c["steps"] == 2 and c["lane_spill"] == 0 and c["scratch"] == 0 and c["heads_inline"], c
    assert c["mfma"] == 8 and c["heads"] == 3 and c["valu"] <= 31, c      # the 64-row instance's step: chains of 3 + 3 + 2
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_ring_asm.py"), "2", "--kernel", SYM],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "G=2: 1 pg_mm_knn_sym_kernel instances, 12 inline fragment loads checked" in out.stdout
    assert "RULE violations: 0" in out.stdout


def test_symbol_is_in_the_library():
    from prograph_amd import _native
    _native.lib()
    blob = open(_native.LIB_PATH, "rb").read()
    assert (SYM + "I13HammingMetricILi2ELi5EEEv9NsqParams").encode() in blob
    assert (SYM + "I13HammingMetricILi1ELi5EEEv9NsqParams").encode() in blob
