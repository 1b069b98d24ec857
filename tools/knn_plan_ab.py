"""Same plans, same results: tools/knn_plan_ab.py PARENT.so NEW.so [--timeout 180].
Two builds of libprograph_hip.so on the branches of the kNN launch planner (prograph_amd/csrc/pg_plan.h), one case and
one library per child process (PROGRAPH_HIP_LIB picks the build, PG_DEBUG_PLAN=1 makes it say what it planned).  Per case:
the `[pg plan ...]` lines the library wrote and a SHA-256 of idx and of dist; the two libraries' outputs must be equal
line for line.  Stops at the first child that fails.  The full output: profiles/knn_plan_ab.txt."""
import argparse, hashlib, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name, N, L, bits, k, (row0, nrows) or None, knobs
CASES = [
    ("4000 self (VALU engine)", 4000, 64, 5, 16, None, {}),
    ("24000 self (MFMA engine, one round, no split)", 24000, 64, 5, 16, None, {}),
    ("66000 self (probe, split, symmetric candidate)", 66000, 64, 5, 16, None, {}),
    ("200000 self L=64 5-bit (cfg3)", 200000, 64, 5, 16, None, {}),
    ("200000 self L=64 8-bit", 200000, 64, 8, 16, None, {}),
    ("200000 self L=32", 200000, 32, 5, 16, None, {}),
    ("100000 self L=128", 100000, 128, 5, 16, None, {}),
    ("rows 70000..140000 of 200000 (rectangular)", 200000, 64, 5, 16, (70000, 70000), {}),
    ("66000 self k=1", 66000, 64, 5, 1, None, {}),
    ("66000 self k=63", 66000, 64, 5, 63, None, {}),
    ("66000 self k=100 (rounds: floor keys, long lists)", 66000, 64, 5, 100, None, {}),
] + [(f"200000 self {k}={v}", 200000, 64, 5, 16, None, {k: v}) for k, v in (
    ("PG_GATE_FORCE", "1"), ("PG_GATE_FORCE", "2"), ("PG_KNN_SYM", "0"), ("PG_KNN_SYM", "1"), ("PG_MM_R", "1"), ("PG_MM_R", "2"),
    ("PG_MM_SPLIT", "0"), ("PG_MM_EVICT", "0"), ("PG_MM_PIECES_AHEAD", "0"), ("PG_MM_PIECES", "8"), ("PG_PROBE", "0"))]


def child(i):
    sys.path.insert(0, ROOT)
    import torch
    from prograph_amd import _native as nat, synth
    _, n, l, bits, k, rows, _ = CASES[i]
    p = nat.pack(torch.from_numpy(synth.clustered_tokens(n, l)), bits=bits)
    row0, nrows = rows if rows else (0, None)
    idx, dist = nat.knn_graph(p, p, k, row0=row0, nrows=nrows)
    torch.cuda.synchronize()
    for name, t in (("idx", idx), ("dist", dist)):
        print(f"{name} {tuple(t.shape)} sha256={hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--timeout", type=float, default=180.0)
    a = ap.parse_args()
    libs = (("parent", os.path.abspath(a.parent)), ("new", os.path.abspath(a.new)))
    differ = 0
    for i, case in enumerate(CASES):
        outs = {}
        for which, lib in libs:
            env = {k: v for k, v in os.environ.items() if not k.startswith("PG_")}
            env.update(case[6], PROGRAPH_HIP_LIB=lib, PG_DEBUG_PLAN="1")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(i)], env=env, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"case {i} ({case[0]}), {which}: no result after {a.timeout} s - stopped")
            if r.returncode:
                raise SystemExit(f"case {i} ({case[0]}), {which}: exit {r.returncode} - stopped\n{r.stderr[-3000:]}")
            outs[which] = [ln for ln in r.stderr.splitlines() if ln.startswith("[pg plan")] + r.stdout.splitlines()
        same = outs["parent"] == outs["new"]
        differ += not same
        print(f"=== case {i}: {case[0]}: {'equal' if same else 'DIFFERENT'}")
        for ln in outs["new"]:
            print("    " + ln)
        if not same:
            print("  parent:")
            for ln in outs["parent"]:
                print("    " + ln)
        sys.stdout.flush()
    print(f"knn_plan_ab: {len(CASES)} cases, {differ} different" + ("" if differ else ": all equal"))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        sys.exit(main())
