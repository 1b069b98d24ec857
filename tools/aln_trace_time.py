"""
Timings behind DESIGN.md §4.20 (alignment tracebacks, `pg_alignment_trace`), on one GPU, by the method of tools/aln_ab.py:
every time is a whole call on a host clock, from the call to the end of a device synchronise, after a warm-up; inputs are
seeded and random; medians with min / max.

  The workload is a kNN graph's worth of edges: --rows (200 000) x --k (16) pairs (row, random column) over rows of 125..128
  tokens and over rows of exactly 64, 21 symbols, under each of the three modes (gap 1, gap_open 11; costs 1..4, scores
  -4..16).  Per mode and shape: `_native.alignment_trace` on packed operands (the host index check and the split into
  launches included) - time, pairs/s, cell updates/s (sum of len x * len y); the same edges through the host expression
  (`alignments.host_trace`) on the first --host-edges (1 000) of them, compared field for field; and, as the forward-only
  ceiling, the mode's `pg_alignment_*_dense` call (int64 out) over an equal number of pairs of the same rows: 50 000 columns
  against rows * k / 50 000 rows.

  --long (`pg_alignment_trace_long`): `Prograph.align` over the k = 16 graph (built once, under the
  local operator) of --long-rows (20 000) rows of 300..400 tokens, under each of the three modes - the whole call: edge
  lists, the upload and packing of the dataset, the index check, the launches; pairs/s and cell updates/s; the parent
  route, `alignments.host_trace`, on the first --long-host-edges (500) of the same edges, compared field for field; and
  the mode's `pg_alignment_*_long_dense` call over an equal number of pairs (every row against k rows) as the
  forward-only ceiling.  Writes profiles/aln_trace_long.txt unless --out is given.

Prints one JSON line; progress goes to stderr.  Writes profiles/aln_trace.txt unless --out is given.

    python tools/aln_trace_time.py [--rows 200000] [--k 16] [--reps 5] [--host-edges 1000] [--out FILE]
    python tools/aln_trace_time.py --long [--long-rows 20000] [--k 16] [--reps 5] [--long-host-edges 500] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from prograph_amd import _native, alignments  # noqa: E402
from aln_ab import random_table, stats, timed, varlen  # noqa: E402

MODES = (("global", _native.ALN_TRACE_GLOBAL), ("local", _native.ALN_TRACE_LOCAL), ("semiglobal", _native.ALN_TRACE_SEMIGLOBAL))
FIELDS = ("score", "x_begin", "x_end", "y_begin", "y_end", "n_ops", "identities")


def long_arm(args):
    import tempfile
    import pandas as pd
    from prograph_amd import Prograph, synth
    from prograph_amd.distance import alignment, local_alignment, semiglobal_alignment
    rng = np.random.default_rng(21)
    a, gap, gap_open, n, k = 21, 1, 11, args.long_rows, args.k
    C = random_table(rng, a, 4)
    S = random_table(rng, a, 20) - 4
    S[np.arange(a), np.arange(a)] = rng.integers(4, 17, a)
    tok, lens = varlen(rng, n, 300, 400, a)
    tok[0, :400] = np.where(tok[0, :400] == 0, 1, tok[0, :400])            # one row of the full width
    lens[0] = 400
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "long.csv")
        pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": rng.uniform(0, 1, n)}).to_csv(f)
        P = Prograph(file=f)
    assert np.array_equal(P.tokenized, tok)
    ops = {"global": (alignment(C, gap, gap_open=gap_open), C, _native.sub_cost(C), _native.alignment_long_dense),
           "local": (local_alignment(S, gap, gap_open=gap_open), S, _native.aln_local_score(S), _native.alignment_local_long_dense),
           "semiglobal": (semiglobal_alignment(S, gap, gap_open=gap_open), S, _native.aln_local_score(S),
                          _native.alignment_semiglobal_long_dense)}
    build_ms, G = timed(lambda: P.build_graph(k=k, distance=ops["local"][0], output="csr"))
    xi = np.repeat(np.arange(n, dtype=np.int64), k)
    yi = G.idx.cpu().numpy().reshape(-1).astype(np.int64)
    cells = int((lens[xi].astype(np.int64) * lens[yi]).sum())
    xo = _native.aln_long_operand(torch.from_numpy(tok), a)
    dcells = int(lens.astype(np.int64).sum() * lens[:k].astype(np.int64).sum())
    res = {"rows": n, "k": k, "lengths": [300, 400], "gap": gap, "gap_open": gap_open, "device": _native.device_info(),
           "graph_build_local_ms": build_ms, "wave_share_bytes": _native.aln_trace_long_wave_bytes(400, 400)}
    for name, mode in MODES:
        op, T, Td, dense = ops[name]
        run = lambda: P.align(G, distance=op)
        run()
        t, out = [], None
        for _ in range(args.reps):
            out = None
            ms, out = timed(run)
            t.append(ms)
        st = stats(t)
        m = min(args.long_host_edges, len(xi))
        t0 = time.perf_counter()
        *fields, hops = alignments.host_trace(mode, T, gap, gap_open, tok, tok, xi[:m], yi[:m])
        host_s = time.perf_counter() - t0
        same = bool(all(np.array_equal(h, getattr(out, f)[:m].cpu().numpy()) for f, h in zip(FIELDS, fields))
                    and np.array_equal(hops, out.ops[:m].cpu().numpy()))
        del out
        dense(xo, xo, Td, gap, gap_open, out_bytes=8, rows=(0, k))
        ds = stats([timed(lambda: dense(xo, xo, Td, gap, gap_open, out_bytes=8, rows=(0, k)))[0] for _ in range(args.reps)])
        res[name] = {
            "align": st, "pairs": len(xi), "cells": cells, "pairs_per_s": len(xi) / (st["median_ms"] * 1e-3),
            "cell_updates_per_s": cells / (st["median_ms"] * 1e-3),
            "host_expression": {"edges": m, "seconds": host_s, "pairs_per_s": m / host_s, "same_as_kernel": same},
            "speedup_over_host_expression": (len(xi) / (st["median_ms"] * 1e-3)) / (m / host_s),
            "forward_only_long_dense": {**ds, "pairs": n * k, "cells": dcells, "cell_updates_per_s": dcells / (ds["median_ms"] * 1e-3)},
            "align_over_forward_per_cell": (st["median_ms"] / cells) / (ds["median_ms"] / dcells)}
        print(name, json.dumps(res[name]), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--long-rows", type=int, default=20_000)
    ap.add_argument("--long-host-edges", type=int, default=500)
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-edges", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                "aln_trace_long.txt" if args.long else "aln_trace.txt")
    if args.long:
        line = json.dumps(long_arm(args))
        print(line)
        with open(args.out, "w") as f:
            f.write(line + "\n")
        return
    rng = np.random.default_rng(20)
    a, gap, gap_open = 21, 1, 11
    C = random_table(rng, a, 4)
    S = random_table(rng, a, 20) - 4
    S[np.arange(a), np.arange(a)] = rng.integers(4, 17, a)
    tables = {"global": (C, _native.sub_cost(C)), "local": (S, _native.aln_local_score(S)), "semiglobal": (S, _native.aln_local_score(S))}
    dense = {"global": lambda xo, yo, t, rows: _native.alignment_affine_dense(xo, yo, t, gap, gap_open, out_bytes=8, rows=rows),
             "local": lambda xo, yo, t, rows: _native.alignment_local_dense(xo, yo, t, gap, gap_open, out_bytes=8, rows=rows),
             "semiglobal": lambda xo, yo, t, rows: _native.alignment_semiglobal_dense(xo, yo, t, gap, gap_open, out_bytes=8, rows=rows)}
    res = {"rows": args.rows, "k": args.k, "gap": gap, "gap_open": gap_open, "device": _native.device_info()}
    for shape, (lo, hi) in (("125..128", (125, 128)), ("64", (64, 64))):
        tok, lens = varlen(rng, args.rows, lo, hi, a)
        xo = _native.aln_operand(torch.from_numpy(tok), a)
        xi = np.repeat(np.arange(args.rows, dtype=np.int32), args.k)
        yi = rng.integers(0, args.rows, len(xi)).astype(np.int32)
        xid, yid = torch.from_numpy(xi).cuda(), torch.from_numpy(yi).cuda()
        cells = int((lens[xi].astype(np.int64) * lens[yi]).sum())
        cols = min(50_000, args.rows)
        drows = max(1, len(xi) // cols)
        co = _native.aln_operand(torch.from_numpy(tok[:cols]), a)
        dcells = int(lens[:cols].astype(np.int64).sum() * lens[:drows].astype(np.int64).sum())
        for name, mode in MODES:
            T, Td = tables[name]
            run = lambda: _native.alignment_trace(xo, xo, xid, yid, mode, Td, gap, gap_open)
            run()
            t, out = [], None
            for _ in range(args.reps):
                out = None
                ms, out = timed(run)
                t.append(ms)
            st = stats(t)
            head, ops = out
            n = min(args.host_edges, len(xi))
            t0 = time.perf_counter()
            *fields, hops = alignments.host_trace(mode, T, gap, gap_open, tok, tok, xi[:n], yi[:n])
            host_s = time.perf_counter() - t0
            same = bool(np.array_equal(np.stack(fields, 1), head[:n, :7].cpu().numpy()) and np.array_equal(hops, ops[:n].cpu().numpy()))
            del out, head, ops
            dense[name](co, xo, Td, (0, drows))
            dt = [timed(lambda: dense[name](co, xo, Td, (0, drows)))[0] for _ in range(args.reps)]
            ds = stats(dt)
            res[f"{name}_{shape}"] = {
                "trace": st, "pairs": len(xi), "cells": cells, "pairs_per_s": len(xi) / (st["median_ms"] * 1e-3),
                "cell_updates_per_s": cells / (st["median_ms"] * 1e-3),
                "host_expression": {"edges": n, "seconds": host_s, "pairs_per_s": n / host_s, "same_as_kernel": same},
                "forward_only_dense": {**ds, "pairs": cols * drows, "cells": dcells,
                                       "cell_updates_per_s": dcells / (ds["median_ms"] * 1e-3)},
                "trace_over_forward_per_cell": (st["median_ms"] / cells) / (ds["median_ms"] / dcells)}
            print(name, shape, json.dumps(res[f"{name}_{shape}"]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
