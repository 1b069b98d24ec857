"""The window of delivered keys in the merge of the symmetric kNN sweep, on the CPU:
tests/capi_sym_window/window_check.cpp includes prograph_amd/csrc/pg_plan.h directly (plain C++, no HIP header, no library,
no device) and runs the lane-local step of the merge's rounds - sym_window_pop, sym_window_refill, the text the kernel runs -
on sixteen simulated lanes at window widths 1, 2 and 4, against rounds that move a lane's whole list at every win.  The
distributions a device test cannot steer (arrival order decides which lane holds which key): one lane with the 16, 17 and 20
smallest keys, two lanes in turns, per-lane counts 0, 1, W, W + 1, 2 W, 15 and 16, own keys only, delivered keys only, fewer
keys than k + 1; k + 1 = 2, 17 and 20.  Once as it is, once as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO, "tests", "capi_sym_window")


@pytest.mark.parametrize("san", ["", "1"], ids=["plain", "asan_ubsan"])
def test_sym_window_on_the_host(tmp_path, san):
    subprocess.check_call(["make", "-s", "-C", HERE, f"BUILD={tmp_path}", f"SAN={san}"])
    out = subprocess.run([os.path.join(str(tmp_path), "window_check")], capture_output=True, text=True, timeout=300)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("window_check ok:"), out.stdout[-4000:] + out.stderr[-2000:]
