"""The entries the symmetric kNN sweep delivers, on the CPU: tests/capi_sym_codec/codec_check.cpp includes
prograph_amd/csrc/pg_plan.h directly (plain C++, no HIP header, no library, no device) and checks the codec the sweep and
the merge run - the field widths at caps 1 .. 65, the round trip at every field edge, the key order of the decoded entry,
the groups' log capacities - and knn_plan's decline rule one row below, at and above the row field's limit.  Once as it
is, once as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO, "tests", "capi_sym_codec")


@pytest.mark.parametrize("san", ["", "1"], ids=["plain", "asan_ubsan"])
def test_sym_codec_on_the_host(tmp_path, san):
    subprocess.check_call(["make", "-s", "-C", HERE, f"BUILD={tmp_path}", f"SAN={san}"])
    out = subprocess.run([os.path.join(str(tmp_path), "codec_check")], capture_output=True, text=True, timeout=300)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("codec_check ok:"), out.stdout[-4000:] + out.stderr[-2000:]
