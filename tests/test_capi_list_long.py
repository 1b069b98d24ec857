"""
The walk of the long list frame on the host (tests/capi_list_long): the chunk / round / group arithmetic
of prograph_amd/csrc/pg_aln_list_long_walk.h, which the kernel frame steers by, in a stand-alone program of its own built with
-fsanitize=address,undefined.  No GPU, no library, no Python code under a sanitizer.
"""
import os
import subprocess

from conftest import REPO


def test_the_walk_visits_every_entry_once_and_keeps_the_barriers_equal():
    capi = os.path.join(REPO, "tests", "capi_list_long")
    subprocess.check_call(["make", "-s", "-C", capi])
    out = subprocess.run([os.path.join(capi, "_build", "walk_check")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "list long walk OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
