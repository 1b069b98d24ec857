"""
kNN graphs beyond 63 neighbours: the round path against the generic batch loop in one process (HIP events, warm-up,
the two versions alternated).

  rounds   build_graph(representation="Embedded", distance=cosine / minkowski, k) - pg_*_knn with first = 1, k = 63,
           then one pg_*_knn_round sweep per 64 more ranks, ceil((k + 1) / 64) fused sweeps in all
  generic  the same call with the operator wrapped in a lambda (`distance=lambda X, Y, similarity=False: ...`), which
           build_graph does not recognise: the reference's loop, 8 rows per batch, torch.sort over all N columns
           and a host copy per batch

Both return the reference's list of (indices, weights) tuples; the outputs must be identical (indices, weight bits
and dtypes) on every shape.  `rounds_csr_ms` also times the round path with output="csr" (no per-row host objects).
Shapes: cos / mink x D in {64, 1280} x k in {64, 100, 256} at N = 50 000, bench.py's embedding data.
Prints one JSON line (per shape the median / min / max ms of each version); progress goes to stderr.

    python tools/knn_rounds_ab.py [--reps 3] [--metrics cos,mink] [--dims 64,1280] [--ks 64,100,256] [--out FILE]
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
from prograph_amd import Prograph, _native, synth  # noqa: E402
from prograph_amd.distance import cosine, minkowski  # noqa: E402

METRICS = {"cos": cosine, "mink": minkowski}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def identical(a, b):
    if len(a) != len(b):
        return False
    return all(np.array_equal(ai, bi) and aw.dtype == bw.dtype and np.array_equal(aw.view(np.uint8), bw.view(np.uint8))
               for (ai, aw), (bi, bw) in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=50_000)
    ap.add_argument("--metrics", default="cos,mink")
    ap.add_argument("--dims", default="64,1280")
    ap.add_argument("--ks", default="64,100,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _native.device()
    n = a.n
    res = {"tool": "knn_rounds_ab", "reps": a.reps, "N": n, "device": _native.device_info(), "shapes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "ab.csv")
        pd.DataFrame({"Sequence": synth.tokens_to_strings(synth.clustered_tokens(n, 8, seed=3)),
                      "Fitness": np.zeros(n)}).to_csv(f)
        pg = Prograph(file=f)
    for d in (int(x) for x in a.dims.split(",")):
        g = torch.Generator(device="cpu").manual_seed(20260104)                  # bench.py's embedding data
        X = torch.randn((n, d), generator=g, dtype=torch.float32).to(torch.float16)
        pg.graph["Embedded"] = list(X.float().numpy())
        for mname in a.metrics.split(","):
            dist = METRICS[mname]
            wrapped = (lambda dd: lambda X, Y, similarity=False: dd(X, Y, similarity=similarity))(dist)
            for k in (int(x) for x in a.ks.split(",")):
                fns = {"rounds": lambda: pg.build_graph(representation="Embedded", k=k, distance=dist),
                       "generic": lambda: pg.build_graph(representation="Embedded", k=k, distance=wrapped)}
                t = {"rounds": [], "generic": []}
                t_wall = time.perf_counter()
                outs = {v: timed(fns[v])[1] for v in fns}                         # warm-up, and the outputs compared
                same = identical(outs["rounds"], outs["generic"])
                del outs
                for r in range(a.reps):
                    for v in (("rounds", "generic") if r % 2 == 0 else ("generic", "rounds")):
                        t[v].append(timed(fns[v])[0])
                csr = [timed(lambda: pg.build_graph(representation="Embedded", k=k, distance=dist, output="csr"))[0]
                       for _ in range(a.reps)]
                rec = {"metric": mname, "D": d, "k": k, "sweeps": (k + 1 + 63) // 64, "identical": bool(same),
                       "wall_s": round(time.perf_counter() - t_wall, 2)}
                for v in t:
                    rec[v] = {"median_ms": float(np.median(t[v])), "min_ms": float(np.min(t[v])),
                              "max_ms": float(np.max(t[v])), "all_ms": [round(x, 2) for x in t[v]]}
                rec["rounds_csr_ms"] = {"median_ms": float(np.median(csr)), "all_ms": [round(x, 2) for x in csr]}
                rec["generic_over_rounds"] = rec["generic"]["median_ms"] / rec["rounds"]["median_ms"]
                name = f"{mname}{d}_k{k}"
                res["shapes"][name] = rec
                print(f"# {name}: rounds {rec['rounds']['median_ms']:.1f} ms (csr {rec['rounds_csr_ms']['median_ms']:.1f}), "
                      f"generic {rec['generic']['median_ms']:.1f} ms (x{rec['generic_over_rounds']:.1f}), identical={same}",
                      file=sys.stderr, flush=True)
        del X
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    return 0 if all(r["identical"] for r in res["shapes"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
