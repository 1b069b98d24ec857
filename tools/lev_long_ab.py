"""
Timings behind DESIGN.md §4.22 (Levenshtein beyond 128 positions), on one GPU, with the method of tools/lev_graph_ab.py:
every time is a whole call on a host clock, from the call to the end of a device synchronise, after a warm-up; arms
alternate; inputs are seeded; medians with min / max.

  dense     rows of 300..400 tokens (clusters of 50 around a parent, 5 % substitutions), 4096 x 20 000 pairs:
            (a) `levenshtein_long_dense`, fp16 out - the new kernel;
            (b) `alignment_long_dense` with 1 - I, gap 1, int32 out - the parent commit's best device route;
            the two matrices are compared for equality.
  torch     (c) `_torch_levenshtein` on --torch-rows (256) of the rows against the 20 000 - what the parent commit runs
            for this very call; the row count stands next to the figure, nothing is extrapolated.
  graph     (d) `build_graph(k=16, distance=levenshtein)` at N = 20 000 with lengths 200..400 on the kernel; and at
            N = --fallback-n (2000) both on the kernel and with `lev_long_ready` false (the generic loop around the torch
            expression, as on the parent commit) - the fallback at N = 20 000 would take a hundred times as long.

Prints one JSON line; progress goes to stderr.

    python tools/lev_long_ab.py [--reps 9] [--only dense,torch,graph] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from prograph_amd import Prograph, _native  # noqa: E402
from prograph_amd.distance import alignment, levenshtein  # noqa: E402
from prograph_amd.distance.levenshtein import _torch_levenshtein  # noqa: E402

ALPHABET = "ACDEFGHIKLMNPQRSTVWY"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "runs": len(v)}


def alternate(fns, reps, log):
    for f in fns.values():
        f()                                                                    # warm-up (code objects loaded)
    times, outs = {k: [] for k in fns}, {}
    for _ in range(reps):
        for key, f in fns.items():
            t, outs[key] = timed(f)
            times[key].append(t)
    res = {k: stats(v) for k, v in times.items()}
    print(log, json.dumps(res), file=sys.stderr, flush=True)
    return res, outs


def rows(n, lmin, lmax, seed):
    """(n, lmax) uint8 tokens 1..20, lengths uniform in lmin..lmax, clusters of 50 rows around one parent."""
    rng = np.random.default_rng(seed)
    T = np.zeros((n, lmax), dtype=np.uint8)
    lens = rng.integers(lmin, lmax + 1, n)
    for c0 in range(0, n, 50):
        parent = rng.integers(1, 21, lmax)
        for r in range(c0, min(n, c0 + 50)):
            row = parent[:lens[r]].copy()
            hit = rng.random(lens[r]) < 0.05
            row[hit] = rng.integers(1, 21, int(hit.sum()))
            T[r, :lens[r]] = row
    return T, lens


def prograph(tok, directory):
    lut = np.array([""] + list(ALPHABET))
    seqs = ["".join(lut[r[r > 0]]) for r in tok]
    f = os.path.join(directory, f"rows{len(tok)}.pkl")
    pd.DataFrame({"Sequence": seqs, "Fitness": np.linspace(0, 1, len(tok))}).to_pickle(f)
    return Prograph(file=f, seed_seq=seqs[0], amino_acids=ALPHABET)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--torch-rows", type=int, default=256)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--graph-reps", type=int, default=3)
    ap.add_argument("--fallback-n", type=int, default=2000)
    ap.add_argument("--valu-per-step", type=float, default=64.0, help="VALU instructions per text position and block in the ISA")
    ap.add_argument("--only", default="dense,torch,graph")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _native.device()
    out = {"device": _native.device_info()["arch"], "reps": args.reps}
    only = args.only.split(",")
    n, m = args.n, args.rows

    if "dense" in only or "torch" in only:
        tok_host, lens = rows(n, 300, 400, 1)
        tok = torch.as_tensor(tok_host, device=dev)
    if "dense" in only:
        lo = _native.lev_long_operand(tok)
        assert lo.valid()
        dist = alignment(1 - np.eye(32, dtype=np.int64), 1)
        ao = _native.aln_long_operand(tok, dist.symbols)
        cost = dist.device_cost()
        fns = {"a_levenshtein_long_dense_f16": lambda: _native.levenshtein_long_dense(lo, lo, out_bytes=2, rows=(0, m)),
               "b_alignment_long_dense_i32": lambda: _native.alignment_long_dense(ao, ao, cost, dist._gap, dist._open, out_bytes=4, rows=(0, m))}
        res, outs = alternate(fns, args.reps, "dense")
        a, b = outs["a_levenshtein_long_dense_f16"], outs["b_alignment_long_dense_i32"]
        ms = res["a_levenshtein_long_dense_f16"]["median_ms"]
        # text positions x pattern blocks a wave runs (its longest pattern), summed over the pairs' waves x 64 lanes
        wave_blocks = np.array([-(-int(lens[c:c + 64].max()) // 128) for c in range(0, n, 64)])
        steps = float(lens[:m].astype(np.int64).sum()) * float(wave_blocks.sum()) * 64
        peak = 256 * 4 * 32 * 2.4e9
        res.update(n=n, rows=m, lengths=[int(lens.min()), int(lens.max())], equal=bool(torch.equal(a.to(torch.int32), b)),
                   pairs_per_s=m * n / (ms * 1e-3), valu_per_step=args.valu_per_step,
                   valu_share_of_peak=steps * args.valu_per_step / (ms * 1e-3) / peak,
                   speedup_a_over_b=res["b_alignment_long_dense_i32"]["median_ms"] / ms)
        out["dense"] = res
        del outs, a, b, ao
        torch.cuda.empty_cache()
    if "torch" in only:
        tr = args.torch_rows
        times = []
        for _ in range(args.torch_reps + 1):
            t, d = timed(lambda: _torch_levenshtein(tok, tok[:tr]))
            times.append(t)
        res = stats(times[1:])
        if "dense" in only:
            res["equal_to_the_kernel"] = bool(torch.equal(d, _native.levenshtein_long_dense(lo, lo, out_bytes=8, rows=(0, tr))))
        res.update(rows=tr, n=n, pairs_per_s=tr * n / (res["median_ms"] * 1e-3))
        print("torch", json.dumps(res), file=sys.stderr, flush=True)
        out["c_torch_levenshtein"] = res
        del d
        torch.cuda.empty_cache()
    if "graph" in only:
        with tempfile.TemporaryDirectory() as tmp:
            tok_g, lens_g = rows(n, 200, 400, 2)
            P = prograph(tok_g, tmp)
            res, outs = alternate({"native": lambda: P.build_graph(k=16, distance=levenshtein, output="csr")}, args.graph_reps, "graph")
            res.update(n=n, k=16, lengths=[int(lens_g.min()), int(lens_g.max())])
            out["d_build_graph_k16"] = res
            del outs
            fn = args.fallback_n
            Ps = prograph(tok_g[:fn], tmp)
            t_nat, g = [], None
            for _ in range(args.graph_reps + 1):
                t, g = timed(lambda: Ps.build_graph(k=16, distance=levenshtein, output="csr"))
                t_nat.append(t)
            ready = _native.lev_long_ready
            _native.lev_long_ready = lambda: False
            try:
                t_fb, tuples = timed(lambda: Ps.build_graph(k=16, distance=levenshtein))
            finally:
                _native.lev_long_ready = ready
            same = all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(g.to_tuples(), tuples))
            out["d_small"] = {"n": fn, "k": 16, "native": stats(t_nat[1:]), "fallback_generic_loop": {"ms": t_fb, "runs": 1},
                              "identical": bool(same)}
            print("graph small", json.dumps(out["d_small"]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
