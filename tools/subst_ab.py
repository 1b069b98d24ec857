"""
Timings behind DESIGN.md §4.14 (substitution-matrix distance), on one GPU.  Every time is a whole call on a host clock,
from the call to the end of a device synchronise, after a warm-up; arms alternate; inputs are seeded and random (not
constant: the bank conflicts of the image read depend on the symbols); medians with min / max.  A dense kernel call
takes about a millisecond, so a timed window of the dense part is --inner calls in a row (the torch expression: a tenth
as many) and the figures are per call.

  dense   pg_substitution_dense, 8192 rows x N = 50 000, L = 64, 21 symbols, fp16 output: time, pairs/s, and the share of
          the LDS bound - one byte of the image per pair and position, 256 B/clk/CU, so 256 / L pairs/clk/CU - at
          256 CUs x 2.4 GHz.  Beside it, in the same run: `pg_hamming_dense` at the same shape (context), and the blocked
          torch expression of the operator, Ct[Y[:, None, :], X[None, :, :]].sum(-1), on --torch-rows rows of the same
          operands - what a callable handed to the generic loop costs per pair, the thing to beat.
  graph   build_graph(k = 16) at N = 50 000, L = 32: `_build_graph_substitution` against `_build_graph_generic` given a
          callable that evaluates the torch expression (--generic-reps runs: it takes seconds); graphs compared.
  pmc     one dense call and nothing else: the program of a `rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE` run
          (counters only); `--sum FILE` then prints the two counters of pg_sub_dense_kernel from its
          counter_collection CSV.

Prints one JSON line; progress goes to stderr.  PROGRAPH_HIP_LIB selects another build of the library (the image
variant -DPG_SUB_SPLIT).

    python tools/subst_ab.py [--reps 9] [--only dense,graph] [--out FILE]
"""
import argparse
import collections
import csv
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from prograph_amd import Prograph, _native  # noqa: E402
from prograph_amd.distance import substitution  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "runs": len(v)}


def repeated(f, inner):
    def run():
        for _ in range(inner - 1):
            f()
        return f()
    return run


def alternate(fns, reps, log, inner=None):
    inner = inner or {}
    for f in fns.values():
        f()                                                                    # warm-up (code objects loaded)
    times, outs = {k: [] for k in fns}, {}
    for _ in range(reps):
        for key, f in fns.items():
            outs[key] = None
            t, outs[key] = timed(repeated(f, inner.get(key, 1)))
            times[key].append(t / inner.get(key, 1))
    res = {k: stats(v) for k, v in times.items()}
    print(log, json.dumps(res), file=sys.stderr, flush=True)
    return res, outs


def random_table(rng, a, hi):
    C = np.triu(rng.integers(1, hi + 1, (a, a)), 1)
    return C + C.T


def counters(path):
    acc = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        if "pg_sub_dense_kernel" in r["Kernel_Name"]:
            acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
    out = {k: sum(v) / len(v) for k, v in acc.items()}
    if out.get("SQ_LDS_IDX_ACTIVE"):
        out["conflict_share"] = out.get("SQ_LDS_BANK_CONFLICT", 0.0) / out["SQ_LDS_IDX_ACTIVE"]
    out["launches"] = max((len(v) for v in acc.values()), default=0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--generic-reps", type=int, default=1)
    ap.add_argument("--inner", type=int, default=200, help="dense kernel calls per timed window")
    ap.add_argument("--n", type=int, default=50_000)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--l", type=int, default=64)
    ap.add_argument("--torch-rows", type=int, default=256)
    ap.add_argument("--n-graph", type=int, default=50_000)
    ap.add_argument("--only", default="dense,graph")
    ap.add_argument("--sum", default=None, help="a rocprofv3 counter_collection CSV: print the counters of the dense kernel")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.sum:
        print(json.dumps(counters(args.sum)))
        return
    dev = _native.device()
    out = {"device": _native.device_info()["arch"], "reps": args.reps, "library": os.path.basename(_native.LIB_PATH)}
    only = args.only.split(",")
    rng = np.random.default_rng(1)
    a = 21

    if "dense" in only or "pmc" in only:
        n, m, l = args.n, args.rows, args.l
        C = random_table(rng, a, 2048 // l)
        dist = substitution(C)
        tok = torch.from_numpy(rng.integers(1, a, (n, l), dtype=np.uint8)).to(dev)
        xo = _native.sub_operand(tok, a)
        cost = dist.device_cost()
        assert xo.valid()
        sub = lambda: _native.substitution_dense(xo, xo, cost, out_bytes=2, rows=(0, m))     # noqa: E731
        if "pmc" in only:
            sub()
            torch.cuda.synchronize()
            print(json.dumps({"pmc": "one dense call", "n": n, "rows": m, "l": l}))
            return
        xp = _native.pack(tok, bits=5)
        yp = _native.pack(tok[:m], bits=5)
        tr = args.torch_rows
        fns = {"substitution_dense_f16": sub,
               "hamming_dense_f16": lambda: _native.hamming_dense(xp, yp, out_bytes=2),
               "torch_expression": lambda: dist._torch_expression(tok, tok[:tr])}
        inner = {"substitution_dense_f16": args.inner, "hamming_dense_f16": args.inner, "torch_expression": max(1, args.inner // 10)}
        res, outs = alternate(fns, args.reps, "dense", inner)
        res["calls_per_window"] = inner
        same = bool(torch.equal(outs["substitution_dense_f16"][:tr].to(torch.int64), outs["torch_expression"]))
        ms = res["substitution_dense_f16"]["median_ms"]
        pairs = m * n / (ms * 1e-3)
        torch_pairs = tr * n / (res["torch_expression"]["median_ms"] * 1e-3)
        bound = 256.0 / l * 256 * 2.4e9                                        # pairs/s: 256 B/clk/CU, l bytes per pair
        res.update(n=n, rows=m, l=l, symbols=a, pairs_per_s=pairs, pairs_per_clk_per_cu=pairs / (256 * 2.4e9),
                   lds_bound_pairs_per_s=bound, share_of_lds_bound=pairs / bound, torch_rows=tr, torch_pairs_per_s=torch_pairs,
                   speedup_over_torch_expression=pairs / torch_pairs,
                   hamming_pairs_per_s=m * n / (res["hamming_dense_f16"]["median_ms"] * 1e-3), first_rows_equal_torch=same)
        out["dense"] = res
        del outs, xo, xp, yp, tok
        torch.cuda.empty_cache()

    if "graph" in only:
        n, l = args.n_graph, 32
        C = random_table(rng, a, 2048 // l)
        dist = substitution(C)
        tok = rng.integers(1, a, (n, l))
        tok[1::2, 3:] = tok[0::2, 3:][:len(tok[1::2])]                         # near pairs, so that ranks are not all ties of noise
        pg = Prograph.__new__(Prograph)                                        # the graph builder alone: no file
        pg.tokenized = tok
        pg.graph = pd.DataFrame({"Tokenized": list(tok)})

        def callable_distance(X, Y, similarity=False):                         # what a user of the generic loop writes
            d = dist._torch_expression(X.to(torch.uint8), Y.to(torch.uint8))
            return 1 / (1 + d) if similarity else d

        native = lambda: pg._build_graph_substitution(None, None, 16, False, "Tokenized", None, dist)     # noqa: E731
        res, outs = alternate({"native_k16": native}, args.reps, "graph")
        G = outs["native_k16"]
        times = []
        for _ in range(args.generic_reps):
            t, tuples = timed(lambda: pg._build_graph_generic(None, 8, None, 16, False, "Tokenized", callable_distance, None))
            times.append(t)
        res["generic_loop_callable_k16"] = stats(times)
        gi = np.array([i for i, _ in tuples])
        gw = np.array([w for _, w in tuples])
        res.update(n=n, l=l, k=16, identical=bool(np.array_equal(G.idx.cpu().numpy(), gi) and np.array_equal(G.dist.cpu().numpy(), gw)),
                   speedup=res["generic_loop_callable_k16"]["median_ms"] / res["native_k16"]["median_ms"])
        out["graph"] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
