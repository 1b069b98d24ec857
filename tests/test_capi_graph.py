"""
The host-and-device routines of the graph operations on the host (tests/capi_graph): the sorting network's
schedule in its wave and workgroup forms at every length 0..130 and at the seams of every tier, the merge ranks, the run combine
and the tie rule of prograph_amd/csrc/pg_graph.h, in a stand-alone program of its own built with -fsanitize=address,undefined.
No GPU, no library, no Python code under a sanitizer.
"""
import os
import subprocess

from conftest import REPO


def test_the_network_sorts_every_length_and_the_merge_follows_the_definition():
    capi = os.path.join(REPO, "tests", "capi_graph")
    subprocess.check_call(["make", "-s", "-C", capi])
    out = subprocess.run([os.path.join(capi, "_build", "graph_check")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "graph routines OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
