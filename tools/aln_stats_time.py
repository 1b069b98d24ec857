"""
Timings behind DESIGN.md §4.25 (alignment statistics, `pg_alignment_stats`), on one GPU, by the method of
tools/aln_trace_time.py: every time is a whole call on a host clock, from the call to the end of a device synchronise,
after one warm-up; inputs are seeded and random; medians of --reps (5) with min / max.

  The workload is a kNN graph's worth of edges: a `KNNGraph` of --rows (200 000) x --k (16) edges (row, random column) over a
  `Prograph` of rows of 125..128 tokens and one of rows of exactly 64, 21 symbols, under each of the four modes (gap 1,
  gap_open 11; costs 1..4, scores -4..16).  Per mode and shape, on the SAME edges:

    `Prograph.align(G)`              the traceback route as it stands (edge lists, upload and packing of the dataset, the
                                     index check, `pg_alignment_trace` in launches that fit 256 MiB of direction bits,
                                     head and ops) - the yardstick;
    `Prograph.align(G, ops=False)`   the same call on `pg_alignment_stats`: no workspace, no ops;
    both kernels alone               `_native.alignment_trace` and `_native.alignment_stats` on packed operands and device
                                     index lists (the index check included), which leaves the host work of
                                     `Prograph.align` out of the ratio;
    the forward-only ceiling         the mode's `pg_alignment_*_dense` call (int64 out) over an equal number of pairs of the
                                     same rows: 50 000 columns against rows * k / 50 000 rows.

  The seven fields of the two routes are compared on the device; `same_fields` must be true.

Prints one JSON line; progress goes to stderr.  Writes profiles/aln_stats.txt unless --out is given.

    python tools/aln_stats_time.py [--rows 200000] [--k 16] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from prograph_amd import Prograph, _native, synth  # noqa: E402
from prograph_amd.distance import alignment, fit_alignment, local_alignment, semiglobal_alignment  # noqa: E402
from prograph_amd.graph import KNNGraph  # noqa: E402
from aln_ab import random_table, stats, timed, varlen  # noqa: E402

MODES = (("global", _native.ALN_TRACE_GLOBAL), ("local", _native.ALN_TRACE_LOCAL), ("semiglobal", _native.ALN_TRACE_SEMIGLOBAL),
         ("fit", _native.ALN_TRACE_FIT))
FIELDS = ("score", "x_begin", "x_end", "y_begin", "y_end", "n_ops", "identities")


def median_of(run, reps):
    """One warm-up, then `reps` timed calls; the last result is handed back, earlier ones are freed before the next call."""
    run()
    t, out = [], None
    for _ in range(reps):
        out = None
        ms, out = timed(run)
        t.append(ms)
    return stats(t), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "aln_stats.txt")
    rng = np.random.default_rng(25)
    a, gap, gap_open, n, k = 21, 1, 11, args.rows, args.k
    C = random_table(rng, a, 4)
    S = random_table(rng, a, 20) - 4
    S[np.arange(a), np.arange(a)] = rng.integers(4, 17, a)
    Cd, Sd = _native.sub_cost(C), _native.aln_local_score(S)
    ops = {"global": (alignment(C, gap, gap_open=gap_open), Cd,
                      lambda xo, yo, rows: _native.alignment_affine_dense(xo, yo, Cd, gap, gap_open, out_bytes=8, rows=rows)),
           "local": (local_alignment(S, gap, gap_open=gap_open), Sd,
                     lambda xo, yo, rows: _native.alignment_local_dense(xo, yo, Sd, gap, gap_open, out_bytes=8, rows=rows)),
           "semiglobal": (semiglobal_alignment(S, gap, gap_open=gap_open), Sd,
                          lambda xo, yo, rows: _native.alignment_semiglobal_dense(xo, yo, Sd, gap, gap_open, out_bytes=8, rows=rows)),
           "fit": (fit_alignment(S, gap, gap_open=gap_open), Sd,
                   lambda xo, yo, rows: _native.alignment_fit_dense(xo, yo, Sd, gap, gap_open, out_bytes=8, rows=rows))}
    res = {"rows": n, "k": k, "gap": gap, "gap_open": gap_open, "reps": args.reps, "device": _native.device_info()}
    for shape, (lo, hi) in (("125..128", (125, 128)), ("64", (64, 64))):
        tok, lens = varlen(rng, n, lo, hi, a)
        with tempfile.TemporaryDirectory() as tmp:
            f = os.path.join(tmp, "rows.csv")
            pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": rng.uniform(0, 1, n)}).to_csv(f)
            P = Prograph(file=f)
        assert np.array_equal(P.tokenized, tok)
        idx = rng.integers(0, n, (n, k)).astype(np.int32)
        G = KNNGraph(torch.from_numpy(idx).cuda(), torch.zeros((n, k), dtype=torch.int16, device="cuda"), n)
        xi, yi = np.repeat(np.arange(n, dtype=np.int32), k), idx.reshape(-1)
        xid, yid = torch.from_numpy(xi).cuda(), torch.from_numpy(yi).cuda()
        cells = int((lens[xi].astype(np.int64) * lens[yi]).sum())
        xo = _native.aln_operand(torch.from_numpy(tok), a)
        cols = min(50_000, n)
        drows = max(1, len(xi) // cols)
        co = _native.aln_operand(torch.from_numpy(tok[:cols]), a)
        dcells = int(lens[:cols].astype(np.int64).sum() * lens[:drows].astype(np.int64).sum())
        for name, mode in MODES:
            op, Td, dense = ops[name]
            ax, ay = (yid, xid) if name == "fit" else (xid, yid)             # fit: the tracer's x is the edge's column
            full_st, full = median_of(lambda: P.align(G, distance=op), args.reps)
            want = torch.stack([getattr(full, f_) for f_ in FIELDS], 1)
            ops_bytes = full.ops.numel()
            del full
            stat_st, got = median_of(lambda: P.align(G, distance=op, ops=False), args.reps)
            same = bool(got.ops is None and torch.equal(torch.stack([getattr(got, f_) for f_ in FIELDS], 1), want))
            del got, want
            ktrace, out = median_of(lambda: _native.alignment_trace(xo, xo, ax, ay, mode, Td, gap, gap_open), args.reps)
            del out
            kstats, out = median_of(lambda: _native.alignment_stats(xo, xo, ax, ay, mode, Td, gap, gap_open), args.reps)
            del out
            ds, out = median_of(lambda: dense(co, xo, (0, drows)), args.reps)
            del out
            per = lambda st: (st["median_ms"] / cells) / (ds["median_ms"] / dcells)
            res[f"{name}_{shape}"] = {
                "pairs": len(xi), "cells": cells, "same_fields": same, "ops_bytes": ops_bytes, "head_bytes": 32 * len(xi),
                "align": full_st, "align_ops_false": stat_st, "align_over_ops_false": full_st["median_ms"] / stat_st["median_ms"],
                "kernel_trace": ktrace, "kernel_stats": kstats, "kernel_trace_over_stats": ktrace["median_ms"] / kstats["median_ms"],
                "stats_cell_updates_per_s": cells / (kstats["median_ms"] * 1e-3),
                "forward_only_dense": {**ds, "pairs": cols * drows, "cells": dcells,
                                       "cell_updates_per_s": dcells / (ds["median_ms"] * 1e-3)},
                "trace_over_forward_per_cell": per(ktrace), "stats_over_forward_per_cell": per(kstats)}
            print(name, shape, json.dumps(res[f"{name}_{shape}"]), file=sys.stderr, flush=True)
        del P, G, xo, co
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
