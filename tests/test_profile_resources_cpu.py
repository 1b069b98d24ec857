"""
The register, scratch and LDS budget of the profile (PSSM) kernels of prograph_amd/csrc/pg_aln_profile.hip, from the
compiler's own resource remarks, by the method and with the flags of tests/test_alignment_resources_cpu.py: the unit is
compiled device-only for gfx950 with -Rpass-analysis=kernel-resource-usage, no GPU needed.  The kernels run the cell loops of
the token kernels on frames that stage less, so they must hold what those hold:

    occupancy      3 waves/SIMD for the kernels up to 128 positions, 2 for the strip-mined ones ("_long_")
    scratch        0 bytes per lane
    LDS per block  at most the token kernels' own figures: 39 080 (short), 40 076 (long)
    instances      three modes x two output types of either kernel

Only the remarks are read, nothing else of the assembly.  Skipped where hipcc is absent.
"""
import os
import re

import pytest

from test_alignment_resources_cpu import HIPCC, remarks

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc is not installed")

LDS = {"pg_aln_profile_dense_kernel": 39080, "pg_aln_profile_long_dense_kernel": 40076}
MODES = ("AlnLocal", "AlnSemiglobal", "AlnFit")


def test_profile_kernel_resources(tmp_path):
    found = []
    for k in remarks("pg_aln_profile", str(tmp_path)):
        base = re.match(r"_Z\d+([a-z0-9_]+?)I\d+(Aln[A-Za-z]+?)(DF16_|x|i)E", k["name"])
        assert base and base.group(1) in LDS and base.group(2) in MODES, f"a kernel this test does not know: {k['name']}"
        name = base.group(1)
        found.append((name, base.group(2), base.group(3)))
        print(k)
        assert k["Occupancy"] == (2 if "_long_" in name else 3), k
        assert k["ScratchSize"] == 0, k
        assert k["LDS"] <= LDS[name], k
    want = [(name, mode, out) for name in LDS for mode in MODES for out in (("i", "x") if "_long_" in name else ("DF16_", "x"))]
    assert sorted(found) == sorted(want), found
