"""
Staged vs fused Minkowski graphs in one process (HIP events, warm-up, the two versions alternated).

  staged  per block of rows (<= 256 MB of fp16 distances, as Prograph._build_graph_minkowski walked them before
          the fused kernels): pg_pack_f16 of the block + pg_minkowski_dense + pg_f16_knn / pg_f16_eps_* - device
          work only (the former per-block host copies are NOT charged to it)
  fused   pg_minkowski_knn, or pg_minkowski_eps_slots + scan + compaction (+ the restricted sweep) with its one sync

Shapes: mink64 / mink1280 (N = 50 000, k = 16, bench.py's data) and eps64 (N = 50 000, D = 64, the threshold
that gives closest to 16 neighbours per row).  Every repetition also checks that both versions give identical arrays.
Prints one JSON line: per shape the median / min / max ms of each version and the ratio of the medians.

    python tools/mink_fused_ab.py [--reps 7] [--shapes mink64,mink1280,eps64] [--out profiles/mink_fused_ab.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from prograph_amd import _native  # noqa: E402

SHAPES = {"mink64": (50_000, 64, "knn"), "mink1280": (50_000, 1280, "knn"), "eps64": (50_000, 64, "eps")}


def staged(X, xp, mode, k, eps):
    n = X.shape[0]
    rows = max(64, min(n, (1 << 27) // n))
    parts = []
    for r0 in range(0, n, rows):
        block = _native.minkowski_dense(xp, _native.pack_f16(X[r0:r0 + rows]))
        parts.append(_native.f16_knn(block, k, first=1) if mode == "knn" else _native.f16_eps(block, _native.CMP_LE, eps))
    if mode == "knn":
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    base, ptrs = 0, [torch.zeros(1, dtype=torch.int64, device=X.device)]
    for p in parts:
        ptrs.append(p[0][1:] + base)
        base += int(p[0][-1])
    return torch.cat(ptrs), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts])


def fused(X, xp, mode, k, eps):
    if mode == "knn":
        return _native.minkowski_knn(xp, xp, k, first=1)
    return _native.minkowski_eps(xp, xp, _native.CMP_LE, eps)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def same(a, b):
    return all(x.dtype == y.dtype and torch.equal(x.view(torch.int16) if x.dtype == torch.float16 else x,
                                                 y.view(torch.int16) if y.dtype == torch.float16 else y) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="mink64,mink1280,eps64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = _native.device()
    res = {"tool": "mink_fused_ab", "reps": a.reps, "device": _native.device_info(), "shapes": {}}
    for name in a.shapes.split(","):
        n, d, mode = SHAPES[name]
        g = torch.Generator(device="cpu").manual_seed(20260104)                 # bench.py's mink data
        X = torch.randn((n, d), generator=g, dtype=torch.float32).to(torch.float16).to(dev)
        xp = _native.pack_f16(X)
        k, eps = 16, None
        if mode == "eps":        # the quantile of the 16th-neighbour distance that gives closest to 16 neighbours per row
            d16 = _native.minkowski_knn(xp, xp, 16, first=1)[1][:, 15].float()
            cand = [float(np.float16(d16.quantile(q).item())) for q in (0.5, 0.35, 0.25, 0.15, 0.1, 0.05)]
            eps = min(cand, key=lambda e: abs(int(fused(X, xp, mode, k, e)[0][-1]) / n - 16))
        reps = a.reps if d <= 64 else max(3, a.reps // 2)
        t = {"staged": [], "fused": []}
        ok = True
        for v in ("staged", "fused"):                                           # warm-up
            timed(lambda: (staged if v == "staged" else fused)(X, xp, mode, k, eps))
        t_wall = time.perf_counter()
        for r in range(reps):
            order = ("staged", "fused") if r % 2 == 0 else ("fused", "staged")
            outs = {}
            for v in order:
                ms, outs[v] = timed(lambda: (staged if v == "staged" else fused)(X, xp, mode, k, eps))
                t[v].append(ms)
            ok = ok and same(outs["staged"], outs["fused"])
            del outs
        rec = {"N": n, "D": d, "mode": mode, "k": k if mode == "knn" else None, "eps": eps, "identical": bool(ok),
               "wall_s": round(time.perf_counter() - t_wall, 2)}
        if mode == "eps":
            rec["nnz"] = int(fused(X, xp, mode, k, eps)[0][-1])
        for v in ("staged", "fused"):
            rec[v] = {"median_ms": float(np.median(t[v])), "min_ms": float(np.min(t[v])), "max_ms": float(np.max(t[v])),
                      "all_ms": [round(x, 3) for x in t[v]]}
        rec["fused_over_staged"] = rec["fused"]["median_ms"] / rec["staged"]["median_ms"]
        res["shapes"][name] = rec
        print(f"# {name}: staged {rec['staged']['median_ms']:.2f} ms, fused {rec['fused']['median_ms']:.2f} ms "
              f"(x{rec['fused_over_staged']:.3f}), identical={ok}", file=sys.stderr, flush=True)
        del X, xp
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["identical"] for r in res["shapes"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
