"""
Measurements behind DESIGN.md §4.29 (filter-and-refine alignment graphs, `pg_alignment_list_scores`), on one GPU, by the
method of tools/aln_stats_time.py: every time is a whole call on a host clock, from the call to the end of a device
synchronise, after one warm-up; inputs are seeded; medians of --reps (5) with min / max.

  timing   On the same seeded rows (tools/aln_stats_time.py's: 21 symbols, lengths `--shape` 64 or 125..128, costs 1..4,
           scores -4..16, gap 1, gap_open 11) and the SAME edge list, in one process, for local and global:
             the list kernel      `_native.alignment_list_scores` on packed operands and a device CSR;
             the stats kernel     `_native.alignment_stats` on the same pairs - how these scores were had before;
             the dense kernel     the mode's `pg_alignment_*_dense` (int64 out) on a block of as many pairs.
           Two edge lists: 200 000 rows x 16 edges (a kNN graph's worth; a quarter of every wave's lanes) and 12 500 rows x
           256 edges (the same 3.2 M pairs with full waves).  `wins`: the list kernel's slowest run is faster than the
           stats kernel's fastest.  `list_over_dense_rate`: the list kernel's cell rate as a fraction of the dense kernel's.
  recall   `build_graph(distance=local_alignment(...), k=16, candidates=spectrum(k=3, symbols=20), pool=P)` for P = 64, 256,
           1023 against the exact `build_graph(distance=local_alignment(...), k=16)` on `synth.clustered_tokens(20 000, 64)`:
           the fraction of the exact graph's edges found, both times, and the pool's kNN graph and `rescore` timed apart.  A record,
           not a test.
  resources   (no GPU) the compiler's report of every instance of the list kernel: VGPRs, SGPRs, scratch, LDS, occupancy.
  report   (no GPU) the parts above, which every step leaves as a JSON file under --parts, into profiles/aln_list.txt
           with a short reading.
  --only long   the same steps for `pg_alignment_list_long_scores` (129..2048 positions), into profiles/aln_list_long.txt:
           `timing` on rows of 300..400 positions (--shape 300..400) with the long list kernel, the source of these scores
           before it - `_native.alignment_trace_long_heads`, what `align(..., ops=False)` runs at that width - and the
           mode's `pg_alignment_*_long_dense`; `resources` over pg_aln_list_long.hip; `report` of those two.

Each GPU step is a process of its own; run them under a time limit each, chained so that a failure ends the chain:

    timeout 300 python tools/aln_list_ab.py timing --shape 64 && timeout 420 python tools/aln_list_ab.py timing --shape 125..128 \\
      && timeout 420 python tools/aln_list_ab.py recall && python tools/aln_list_ab.py resources && python tools/aln_list_ab.py report
    timeout 900 python tools/aln_list_ab.py timing --only long --shape 300..400 && python tools/aln_list_ab.py resources --only long \\
      && python tools/aln_list_ab.py report --only long
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.join(HERE, "..")
sys.path.insert(0, REPO)
GAP, GAP_OPEN, A = 1, 11, 21


def tables():
    from aln_ab import random_table
    rng = np.random.default_rng(25)
    C = random_table(rng, A, 4)
    S = random_table(rng, A, 20) - 4
    S[np.arange(A), np.arange(A)] = rng.integers(4, 17, A)
    return C, S


def median_of(run, reps):
    from aln_ab import stats, timed
    run()
    t, out = [], None
    for _ in range(reps):
        out = None
        ms, out = timed(run)
        t.append(ms)
    return stats(t), out


def timing(args):
    import torch
    from aln_ab import varlen
    from prograph_amd import _native
    long = args.only == "long"
    if long != (args.shape == "300..400"):
        raise SystemExit("--only long goes with --shape 300..400, and only with it")
    lo, hi = {"64": (64, 64), "125..128": (125, 128), "300..400": (300, 400)}[args.shape]
    rng = np.random.default_rng(31)
    n = args.rows
    C, S = tables()
    Cd, Sd = _native.sub_cost(C), _native.aln_local_score(S)
    modes = {"local": (_native.ALN_TRACE_LOCAL, Sd, _native.alignment_local_long_dense if long else _native.alignment_local_dense),
             "global": (_native.ALN_TRACE_GLOBAL, Cd, _native.alignment_long_dense if long else _native.alignment_affine_dense)}
    # the three arms: the list kernel, how these scores were had before it, the dense kernel
    operand, list_scores, before = (_native.aln_long_operand, _native.alignment_list_long_scores, _native.alignment_trace_long_heads) \
        if long else (_native.aln_operand, _native.alignment_list_scores, _native.alignment_stats)
    tok, lens = varlen(rng, n, lo, hi, A)
    xo = operand(torch.from_numpy(tok), A)
    res = {"part": "timing", "shape": args.shape, "rows": n, "gap": GAP, "gap_open": GAP_OPEN, "reps": args.reps,
           "device": _native.device_info()}
    for rows, k in ((n, 16), (n // 16, 256)):
        idx = rng.integers(0, n, (rows, k)).astype(np.int32)
        yo = xo if rows == n else operand(torch.from_numpy(tok[:rows]), A)
        indptr = torch.arange(0, rows * k + 1, k, dtype=torch.int64).cuda()
        indices = torch.from_numpy(idx.reshape(-1)).cuda()
        ri = torch.from_numpy(np.repeat(np.arange(rows, dtype=np.int32), k)).cuda()
        cells = int((lens[:rows].astype(np.int64)[:, None] * lens[idx]).sum())
        cols = min(50_000, n)
        drows = max(1, rows * k // cols)
        co = operand(torch.from_numpy(tok[:cols]), A)
        dcells = int(lens[:cols].astype(np.int64).sum() * lens[:drows].astype(np.int64).sum())
        for name, (mode, Td, dense) in modes.items():
            ls, got = median_of(lambda: list_scores(xo, yo, indptr, indices, mode, Td, GAP, GAP_OPEN), args.reps)
            st, head = median_of(lambda: before(xo, xo, ri, indices, mode, Td, GAP, GAP_OPEN), args.reps)
            same = bool(torch.equal(got, head[:, 0].contiguous()))
            del got, head
            ds, out = median_of(lambda: dense(co, xo, Td, GAP, GAP_OPEN, out_bytes=8, rows=(0, drows)), args.reps)
            del out
            rate = lambda s, c: c / (s["median_ms"] * 1e-3)               # noqa: E731
            res[f"{name}_{rows}x{k}"] = {
                "pairs": rows * k, "cells": cells, "same_scores": same, "list": ls, "stats": st,
                "dense": {**ds, "pairs": cols * drows, "cells": dcells},
                "wins": ls["max_ms"] < st["min_ms"], "stats_over_list": st["median_ms"] / ls["median_ms"],
                "list_cell_updates_per_s": rate(ls, cells), "stats_cell_updates_per_s": rate(st, cells),
                "dense_cell_updates_per_s": rate(ds, dcells), "list_over_dense_rate": rate(ls, cells) / rate(ds, dcells)}
            print(name, rows, k, json.dumps(res[f"{name}_{rows}x{k}"]), file=sys.stderr, flush=True)
    return res


def recall(args):
    import pandas as pd
    import torch
    from prograph_amd import Prograph, _native, synth
    from prograph_amd.distance import local_alignment, spectrum
    n, k = args.n, 16
    _, S = tables()
    tok = synth.clustered_tokens(n, 64)
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "rows.csv")
        pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": np.random.default_rng(0).uniform(0, 1, n)}).to_csv(f)
        P = Prograph(file=f)
    assert np.array_equal(P.tokenized, tok)
    op = local_alignment(S, GAP, gap_open=GAP_OPEN)

    def edges(g):
        idx = g.idx.cpu().numpy().astype(np.int64)
        r = np.repeat(np.arange(idx.shape[0], dtype=np.int64), idx.shape[1]).reshape(idx.shape)
        return np.unique((r * n + idx)[idx >= 0])

    def once(run):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, g
    once(lambda: P.build_graph(distance=op, k=k, candidates=spectrum(k=3, symbols=20), pool=64, output="csr"))      # warm-up
    ms, exact = once(lambda: P.build_graph(distance=op, k=k, output="csr"))
    want = edges(exact)
    res = {"part": "recall", "n": n, "positions": 64, "k": k, "gap": GAP, "gap_open": GAP_OPEN, "exact_ms": ms,
           "exact_edges": int(len(want)), "device": _native.device_info(), "pools": {}}
    for pool in (64, 256, 1023):
        ms, g = once(lambda: P.build_graph(distance=op, k=k, candidates=spectrum(k=3, symbols=20), pool=pool, output="csr"))
        found = len(np.intersect1d(edges(g), want, assume_unique=True))
        pool_ms, cand = once(lambda: P.build_graph(k=pool, distance=spectrum(k=3, symbols=20), output="csr"))      # the call's two parts
        rescore_ms, _ = once(lambda: P.rescore(cand, op, k=k))
        del cand
        res["pools"][str(pool)] = {"ms": ms, "pool_graph_ms": pool_ms, "rescore_ms": rescore_ms, "found": int(found),
                                   "recall": found / len(want)}
        print(pool, json.dumps(res["pools"][str(pool)]), file=sys.stderr, flush=True)
    return res


def resources(args):
    """hipcc's -Rpass-analysis=kernel-resource-usage over the file that holds the list instances."""
    src = os.path.join(REPO, "prograph_amd", "csrc")
    out = {"part": "resources", "kernels": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for f in ("pg_aln_list_long.hip" if args.only == "long" else "pg_aln_list.hip",):
            log = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wno-pass-failed",
                                  "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(src, f), "-o", os.path.join(tmp, "o.o")],
                                 capture_output=True, text=True, check=True).stderr
            name = None
            for line in log.splitlines():
                m = re.search(r"remark: +([A-Za-z ]+?)(?: \[[^\]]*\])?: +(\S+)", line)
                if not m:
                    continue
                key, val = m.group(1).strip(), m.group(2)
                if key == "Function Name":
                    name = re.sub(r"^_Z\d+", "", val)
                    name = name[:name.index("kernel") + 6]
                    out["kernels"].setdefault(name, {})
                elif name and key in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size"):
                    out["kernels"][name][key] = int(val)
    out["kernels"] = {k_: v for k_, v in out["kernels"].items() if "list" in k_}
    return out


def report_long(args):
    """profiles/aln_list_long.txt: the compiler's report, the timing at 300..400 positions, the route condition."""
    parts = {}
    for name in sorted(os.listdir(args.parts)):
        if name.startswith("aln_list_long_") and name.endswith(".json"):
            with open(os.path.join(args.parts, name)) as f:
                parts[name[14:-5]] = json.loads(f.read())
    lines = ["pg_alignment_list_long_scores (DESIGN.md 4.29): tools/aln_list_ab.py --only long.  A reading first, then every part as "
             "one JSON line.", ""]
    if "resources" in parts:
        lines.append("Compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), every instance of the long list frame:")
        for k_, v in parts["resources"]["kernels"].items():
            lines.append(f"  {k_:38s} VGPRs {v.get('VGPRs')}  AGPRs {v.get('AGPRs')}  SGPRs {v.get('TotalSGPRs')}  scratch "
                         f"{v.get('ScratchSize')} B/lane  LDS {v.get('LDS Size')} B  occupancy {v.get('Occupancy')} waves/SIMD")
        lines.append("")
    p = parts.get("timing_300..400")
    if p:
        lines.append(f"Timing, lengths {p['shape']}, {p['rows']} rows, gap {p['gap']} / gap_open {p['gap_open']}, median [min .. max] ms of "
                     f"{p['reps']} whole calls: (a) the long list kernel, (b) alignment_trace_long_heads - the scores of "
                     "align(..., ops=False) before it -, (c) the long dense kernel on as many pairs:")
        for case, v in p.items():
            if not isinstance(v, dict) or "list" not in v:
                continue
            f3 = lambda s: f"{s['median_ms']:.3f} [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]"       # noqa: E731
            lines.append(f"  {case:18s} (a) list {f3(v['list'])}   (b) trace {f3(v['stats'])}   (c) dense {f3(v['dense'])}")
            lines.append(f"  {'':18s} (a) slowest < (b) fastest: {v['wins']}   (b) / (a) {v['stats_over_list']:.1f}x   "
                         f"list {v['list_cell_updates_per_s']:.3e} cells/s = {v['list_over_dense_rate']:.3f} of dense "
                         f"{v['dense_cell_updates_per_s']:.3e}   same scores: {v['same_scores']}")
        wins = [v["wins"] for v in p.values() if isinstance(v, dict) and "list" in v]
        lines += ["", f"Route condition ((a)'s slowest run faster than (b)'s fastest, on both shapes, both modes): {all(wins)}.", "",
                  "Reading.  A workgroup serves one row at a time, its four waves one 64-entry chunk each, so a 16-edge list runs",
                  "16 of the workgroup's 256 lanes and three waves idle: the fraction of the dense rate there is the lane use, a",
                  "little over 1/16, not a cost of the gather.  At 256 edges a row every lane works, and the gather and the per-row",
                  "staging stay hidden behind the cell loop.  (c) runs 1568 (column tile, row group) items on 512 resident",
                  "workgroups - three full rounds and a thin fourth -, so a ratio a little above 1 says that the list frame is no",
                  "slower than the dense one, and no more than that.", ""]
    lines += [json.dumps(v) for v in parts.values()]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:-len(parts)] if parts else lines))


def report(args):
    if args.only == "long":
        return report_long(args)
    parts = {}
    for name in sorted(os.listdir(args.parts)):
        if name.startswith("aln_list_") and not name.startswith("aln_list_long_") and name.endswith(".json"):
            with open(os.path.join(args.parts, name)) as f:
                parts[name[9:-5]] = json.loads(f.read())
    lines = ["pg_alignment_list_scores (DESIGN.md 4.29): tools/aln_list_ab.py.  A reading first, then every part as one JSON line.", ""]
    if "resources" in parts:
        lines.append("Compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), every instance of the list frame:")
        for k_, v in parts["resources"]["kernels"].items():
            lines.append(f"  {k_:34s} VGPRs {v.get('VGPRs')}  AGPRs {v.get('AGPRs')}  SGPRs {v.get('TotalSGPRs')}  scratch "
                         f"{v.get('ScratchSize')} B/lane  LDS {v.get('LDS Size')} B  occupancy {v.get('Occupancy')} waves/SIMD")
        lines.append("")
    for key in ("timing_64", "timing_125..128"):
        if key not in parts:
            continue
        p = parts[key]
        lines.append(f"Timing, lengths {p['shape']}, {p['rows']} rows, median [min .. max] ms of {p['reps']}:")
        for case, v in p.items():
            if not isinstance(v, dict) or "list" not in v:
                continue
            f3 = lambda s: f"{s['median_ms']:.3f} [{s['min_ms']:.3f} .. {s['max_ms']:.3f}]"       # noqa: E731
            lines.append(f"  {case:18s} list {f3(v['list'])}   stats {f3(v['stats'])}   dense {f3(v['dense'])}")
            lines.append(f"  {'':18s} list slowest < stats fastest: {v['wins']}   stats / list {v['stats_over_list']:.1f}x   "
                         f"list {v['list_cell_updates_per_s']:.3e} cells/s = {v['list_over_dense_rate']:.3f} of dense "
                         f"{v['dense_cell_updates_per_s']:.3e}   same scores: {v['same_scores']}")
        lines.append("")
    if any(k_.startswith("timing") for k_ in parts):
        lines += ["Reading.  A wave serves one row at a time, so a 16-edge list runs 16 of a wave's 64 lanes: its fraction of the dense",
                  "rate is the lane use, a little over 1/4, not a cost of the gather.  At 256 edges a row every lane works, and the",
                  "fraction there is what the gather costs: the uncoalesced operand loads stay hidden behind the cell loop.", ""]
    if "recall" in parts:
        p = parts["recall"]
        lines.append(f"Recall of build_graph(local_alignment, k={p['k']}, candidates=spectrum(k=3, symbols=20), pool=P) against the exact "
                     f"graph, synth.clustered_tokens({p['n']}, {p['positions']}); exact: {p['exact_ms']:.0f} ms, {p['exact_edges']} edges:")
        for pool, v in p["pools"].items():
            lines.append(f"  pool {pool:>4s}   recall {v['recall']:.4f}   ({v['found']} edges)   {v['ms']:.0f} ms, of which the pool's kNN graph "
                         f"{v['pool_graph_ms']:.0f} ms and rescore {v['rescore_ms']:.1f} ms when called apart")
        lines += ["Reading.  The clusters have 256 members with many equal scores, so a pool below the cluster size cannot hold a row's",
                  "exact neighbours.  Beyond it the recall stays below 1 because the two routes leave out different things: the exact one",
                  "drops rank 0, whatever it is, this one drops the row itself.  Where a row of lower index scores as much against row",
                  "r as r itself (duplicates and near-duplicates: 93 of the first 300 rows of this data), the exact graph keeps the",
                  "edge (r, r) and loses r's best neighbour; the rescored graph has it the other way round - about one edge a row.",
                  "The time is the whole call, and nearly all of it is the pool's own kNN graph (the spectrum sweep in rounds of 64",
                  "ranks): scoring and selecting the pool is the small part.", ""]
    lines += [json.dumps(v) for v in parts.values()]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:-len(parts)] if parts else lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("step", choices=("timing", "recall", "resources", "report"))
    ap.add_argument("--shape", choices=("64", "125..128", "300..400"), default="64")
    ap.add_argument("--only", choices=("long",), default=None)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default=os.path.join(tempfile.gettempdir(), "aln_list_parts"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "aln_list_long.txt" if args.only == "long" else "aln_list.txt")
    if args.step == "report":
        return report(args)
    res = {"timing": timing, "recall": recall, "resources": resources}[args.step](args)
    os.makedirs(args.parts, exist_ok=True)
    tag = f"timing_{args.shape}" if args.step == "timing" else args.step
    line = json.dumps(res)
    with open(os.path.join(args.parts, f"aln_list_{'long_' if args.only == 'long' else ''}{tag}.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
