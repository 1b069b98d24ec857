"""Two builds of libprograph_hip.so under bench.py, alternated, for several workloads:
tools/chain_scan_ab.py PARENT.so NEW.so [--rounds 3] [--steps 20 --warmup 5] [--workloads cfg3,cfg3b8,cfg2,cfg4slice]
[--outputs cfg3,cfg3b8,cfg3d,cfg2] [--scratch DIR].
Timing: per workload bench.py in child processes (PROGRAPH_HIP_LIB picks the build) in the order parent, new, ..., parent
(2 * rounds + 1 runs); `cfg4slice` is `PG_FORCE_DIST=1 bench.py --workload cfg4`, one GPU's slice of the N = 1M graph.  A gain
counts when the median ms_per_step of the new build is below the parent's by more than three times the largest difference
between two parent runs; a loss when it is above it by more than that difference.  Outputs: `bench.py --dump-outputs` of
both builds per workload, every array compared.  One JSON line (profiles/r12_chain_scan.json, "ab")."""
import argparse, glob, json, os, statistics, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("parent")
ap.add_argument("new")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--workloads", default="cfg3,cfg3b8,cfg2,cfg4slice")
ap.add_argument("--outputs", default="cfg3,cfg3b8,cfg3d,cfg2")
ap.add_argument("--scratch", default=None)
a = ap.parse_args()
libs = {"parent": os.path.abspath(a.parent), "new": os.path.abspath(a.new)}


def bench(which, wl, extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PG_")}
    env["PROGRAPH_HIP_LIB"] = libs[which]
    args = ["--gpus", "1"]
    if wl == "cfg4slice":
        env["PG_FORCE_DIST"] = "1"
        args += ["--workload", "cfg4"]
    elif wl != "cfg3":                                       # cfg3 is bench.py's default workload: the command every pull request is measured by
        args += ["--workload", wl]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + extra, env=env, capture_output=True, text=True, timeout=900)
    if out.returncode:
        raise SystemExit(f"bench.py {wl} ({which}) failed: {out.stderr[-2000:]}")
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


res = {"tool": "chain_scan_ab", "steps": a.steps, "warmup": a.warmup, "ab": {}}
order = ["parent", "new"] * a.rounds + ["parent"]
for wl in [w for w in a.workloads.split(",") if w]:
    runs = []
    for which in order:
        r = bench(which, wl, ["--steps", str(a.steps), "--warmup", str(a.warmup)])
        runs.append({"lib": which, "ms_per_step": r["ms_per_step"]})
        print(f"[{wl} {which}] ms_per_step={r['ms_per_step']}", file=sys.stderr, flush=True)
    par = [r["ms_per_step"] for r in runs if r["lib"] == "parent"]
    new = [r["ms_per_step"] for r in runs if r["lib"] == "new"]
    spread = max(par) - min(par)
    gain = statistics.median(par) - statistics.median(new)
    res["ab"][wl] = {"runs": runs, "parent_median_ms": statistics.median(par), "new_median_ms": statistics.median(new), "gain_ms": gain,
                     "gain_pct": 100.0 * gain / statistics.median(par), "parent_spread_ms": spread, "gain_counts": gain > 3.0 * spread,
                     "slower_than_spread": -gain > spread}
    print(json.dumps({wl: res["ab"][wl]}), file=sys.stderr, flush=True)

import numpy as np
same = {}
with tempfile.TemporaryDirectory(dir=a.scratch) as tmp:
    for wl in [w for w in a.outputs.split(",") if w]:
        for which in ("parent", "new"):
            bench(which, wl, ["--steps", "2", "--warmup", "1", "--dump-outputs", os.path.join(tmp, wl, which)])
        names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(tmp, wl, "parent", "*.npy")))
        same[wl] = {n: bool(np.array_equal(np.load(os.path.join(tmp, wl, "parent", n)), np.load(os.path.join(tmp, wl, "new", n)))) for n in names}
        if not names:
            same[wl] = {"(no arrays)": False}
res["outputs_equal"] = same
res["outputs_all_equal"] = all(v for d in same.values() for v in d.values())
print(json.dumps(res))
