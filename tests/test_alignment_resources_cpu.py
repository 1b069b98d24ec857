"""
The register, scratch and LDS budget of every alignment score kernel, from the compiler's own resource remarks: the six
translation units of prograph_amd/csrc/pg_aln*.hip that stand on pg_aln_frame.h (and pg_aln_score.h) are compiled device-only
for gfx950 with the Makefile's flags and -Rpass-analysis=kernel-resource-usage, no GPU needed.  These kernels sit on the
register cliff (164..168 VGPRs of the 168 that three waves per SIMD allow; 194..198 of the 256 that two allow), and the
shared frame puts all modes at risk at once, so for every kernel instance found:

    occupancy      3 waves/SIMD for the kernels up to 128 positions, 2 for the strip-mined ones ("_long_")
    scratch        0 bytes per lane
    LDS per block  at most the figure measured before the frame was shared (profiles/aln_frame_resources.txt) plus 8 bytes,
                   the room of an smin / smax pair

The per-pair kernels on pg_aln_pair.h (the traceback template of pg_aln_trace.hip, two instances; the statistics kernel of
pg_aln_stats.hip, three) are LDS-bound at one wave per SIMD, nowhere near a register cliff: for them scratch 0, the number
of instances, and LDS per block at most the figure measured before they shared a frame
(profiles/aln_pair_frame_resources.txt); their VGPRs are printed, not asserted.

Only the remarks are read, nothing else of the assembly.  Skipped where hipcc is absent.
"""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "prograph_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wno-unused-function", "-Wno-pass-failed"]
# translation unit -> kernel name -> LDS bytes per block before the frame was shared
LDS = {
    "pg_aln": {"pg_aln_dense_kernel": 39072},
    "pg_aln_affine": {"pg_aln_affine_dense_kernel": 39072},
    "pg_aln_local": {"pg_aln_local_dense_kernel": 39076},
    "pg_aln_long": {"pg_aln_long_dense_kernel": 40072},         # the global instance took 40068, the local one 40072
    "pg_aln_semiglobal": {"pg_aln_semiglobal_dense_kernel": 39080, "pg_aln_semiglobal_long_dense_kernel": 40076},
    "pg_aln_fit": {"pg_aln_fit_dense_kernel": 39080, "pg_aln_fit_long_dense_kernel": 40076},
}
LDS_LONG_GLOBAL = 40068
INSTANCES = {"pg_aln_long_dense_kernel": 4}                     # two modes x two output types; every other kernel: two output types
# the per-pair units: kernel name -> template argument -> LDS bytes per block before the frame was shared
PAIR_LDS = {
    "pg_aln_trace": {"pg_aln_trace_kernel": {"Lb0": 78336, "Lb1": 77824}},      # up to 128 positions, the strip loop
    "pg_aln_stats": {"pg_aln_stats_kernel": {"Li32": 39936, "Li64": 74752, "Li128": 144384}},
}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")


def remarks(unit, tmp):
    p = subprocess.run([HIPCC, *FLAGS, "-Rpass-analysis=kernel-resource-usage", "-S", "--cuda-device-only", unit + ".hip", "-o",
                        os.path.join(tmp, unit + ".s")], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    kernels, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            kernels.append(cur)
        else:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return kernels


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("aln_resources"))
    with ThreadPoolExecutor(max_workers=6) as pool:                          # six compiler processes at the most
        return dict(zip(LDS, pool.map(lambda u: remarks(u, tmp), LDS)))


@pytest.mark.parametrize("unit", sorted(LDS))
def test_alignment_kernel_resources(usage, unit):
    found = {k: 0 for k in LDS[unit]}
    for k in usage[unit]:
        base = re.match(r"_Z\d+([a-z0-9_]+?)I", k["name"])
        assert base and base.group(1) in LDS[unit], f"{unit}.hip: a kernel this test does not know: {k['name']}"
        name = base.group(1)
        found[name] += 1
        print(unit, k)
        assert k["Occupancy"] == (2 if "_long_" in name else 3), k
        assert k["ScratchSize"] == 0, k
        lds = LDS_LONG_GLOBAL if "AlnGlobalLong" in k["name"] else LDS[unit][name]
        assert k["LDS"] <= lds + 8, k
    assert found == {k: INSTANCES.get(k, 2) for k in LDS[unit]}, found


@pytest.fixture(scope="module")
def pair_usage(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("aln_pair_resources"))
    with ThreadPoolExecutor(max_workers=2) as pool:
        return dict(zip(PAIR_LDS, pool.map(lambda u: remarks(u, tmp), PAIR_LDS)))


@pytest.mark.parametrize("unit", sorted(PAIR_LDS))
def test_pair_kernel_resources(pair_usage, unit):
    found = []
    for k in pair_usage[unit]:
        base = re.match(r"_Z\d+([a-z0-9_]+?)I(L[bi]\d+)E", k["name"])
        assert base and base.group(2) in PAIR_LDS[unit].get(base.group(1), {}), f"{unit}.hip: a kernel this test does not know: {k['name']}"
        found.append(base.group(2))
        print(unit, k)                                                      # the VGPRs among them: recorded, not asserted
        assert k["ScratchSize"] == 0, k
        assert k["LDS"] <= PAIR_LDS[unit][base.group(1)][base.group(2)], k
    (instances,) = PAIR_LDS[unit].values()
    assert sorted(found) == sorted(instances), found
