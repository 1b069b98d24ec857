"""
The chained filter MFMAs of pg_mm.h, without a GPU: the hot loop's generated ISA for the flagship's group
count (tools/check_scan_loop.py: every MFMA-engine instance of it) and the flag identity of the chained accumulator
(pg_common.h) over every triple of filter results, in a stand-alone host program.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# VALU instructions per super-tile of the loop BEFORE the chain (one OR tree per MFMA), by MFMAs per super-tile: the
# census of the same tool on the parent's pg_mm.h at G = 2 (4: 38 in the short-list kNN instances, 40 in the others)
VALU_BEFORE = {4: 38, 8: 72}


def test_scan_loop_census_of_the_generated_isa():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_scan_loop.py"), "2", "--json"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(report) == 10                                          # eps, symmetric eps, kNN long / short / two blocks; 5 and 8 planes
    for name, c in report.items():
        assert c["steps"] == 2, (name, c)                             # the loop is unrolled by two
        assert c["lane_spill"] == 0 and c["scratch"] == 0, (name, c)
        assert c["heads_inline"], (name, c)
        if "ELi0ELi64ELi1E" in name or "ELi2ELi64ELi1E" in name:
            # eps / symmetric eps: kept on one MFMA per OR tree (pg_mm.h kChain: the chain measured a loss at cfg2) -
            # the parent's step, and not a VALU instruction more than it (40)
            assert c["mfma"] == 4 and c["heads"] == 4 and c["valu"] <= 40, (name, c)
            continue
        assert c["heads"] in (2, 3), (name, c)                        # chains of 3 + 1, or 3 + 3 + 2
        assert c["mfma"] in VALU_BEFORE and c["valu"] < VALU_BEFORE[c["mfma"]], (name, c)
    assert sorted(c["mfma"] for c in report.values()) == [4] * 8 + [8] * 2


def test_flag_identity_over_every_triple_of_filter_results(tmp_path):
    exe = str(tmp_path / "chain_flag_host")
    src = os.path.join(ROOT, "tools", "ubench", "chain_flag_host.hip")
    subprocess.run(["/opt/rocm/bin/hipcc", "--cuda-host-only", "-O2", "-std=c++17", src, "-o", exe], check=True, capture_output=True, timeout=600)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "11697083 triples in [-114, 112]^3: 0 values wrong, 0 flags wrong, 0 negative fields not named" in out.stdout
