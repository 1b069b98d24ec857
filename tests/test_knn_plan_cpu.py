"""The kNN launch planner on the CPU: tests/capi_plan/plan_check.cpp includes prograph_amd/csrc/pg_plan.h directly
(plain C++, no HIP header, no library, no device) and checks the planners against the recorded table
tests/capi_plan/plan_table.txt, the decisions the planner's comments promise (cfg3: 64-row passes, 196 608 rows in plain
passes, 53 row blocks in 16 pieces), the facts the executor in pg_api.hip relies on over a sweep of shapes, and every
knob set alone."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(REPO, "tests", "capi_plan")


def test_knn_plan_on_the_host(tmp_path):
    subprocess.check_call(["make", "-s", "-C", HERE, f"BUILD={tmp_path}"])
    out = subprocess.run([os.path.join(str(tmp_path), "plan_check"), os.path.join(HERE, "plan_table.txt")],
                         capture_output=True, text=True, timeout=300)
    last = out.stdout.strip().splitlines()[-1] if out.stdout.strip() else ""
    assert out.returncode == 0 and last.startswith("plan_check ok:"), out.stdout[-4000:] + out.stderr[-2000:]


def test_plan_header_is_host_only():
    """pg_plan.h includes no HIP header, and pg_api.hip reads the environment through the knob reader alone."""
    plan = open(os.path.join(REPO, "prograph_amd", "csrc", "pg_plan.h")).read()
    assert "#include <hip" not in plan and '#include "pg_' not in plan
    api = open(os.path.join(REPO, "prograph_amd", "csrc", "pg_api.hip")).read()
    assert "getenv" not in api and api.count("pg_knobs_read(") == 1
