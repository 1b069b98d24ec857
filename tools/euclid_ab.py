"""
Native Euclidean graphs beside the two embedding metrics the library already had, in one process (HIP events,
warm-up, the three versions alternated).

  euclidean  pg_cosine_prep + pg_euclidean_knn (ranks 1..k), or pg_cosine_prep + pg_euclidean_eps_slots + scan +
             compaction (+ the restricted sweep) - what build_graph(distance=euclidean) runs
  cosine     the same kernels with the cosine epilogue (pg_cosine_knn / pg_cosine_eps_*): the yardstick for "costs
             what cosine costs"
  minkowski  pg_pack_f16 + pg_minkowski_knn / pg_minkowski_eps_*: the fused fp16 emulation of the reference (DESIGN.md
             §4.5), re-run beside the other two

Shapes: knn64 / knn1280 (N = 50 000, k = 16, bench.py's embedding data) and eps64 / eps1280 (per metric the threshold
that gives closest to 16 neighbours per row; Minkowski takes the Euclidean one, rounded to fp16; the rows beyond the
default slot capacity of 256, which cost a second sweep, are counted per metric).  No version is
checked against another here - they are different contracts (tests/test_euclidean_gpu.py pins the Euclidean one); the
share of Euclidean kNN rows whose neighbour SET equals Minkowski's is recorded for orientation only.
The matrix-core floor is 2 N^2 D FLOP at 2.5 PF dense F16.
Prints one JSON line: per shape the median / min / max ms of each version and the share of the floor.

    python tools/euclid_ab.py [--reps 7] [--shapes knn64,knn1280,eps64,eps1280] [--out profiles/euclid_ab.json]
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

SHAPES = {"knn64": (50_000, 64, "knn"), "knn1280": (50_000, 1280, "knn"),
          "eps64": (50_000, 64, "eps"), "eps1280": (50_000, 1280, "eps")}
VERSIONS = ("euclidean", "cosine", "minkowski")
PEAK_F16 = 2.5e15


def run(version, X, mode, k, eps):
    if version == "minkowski":
        xp = _native.pack_f16(X)
        if mode == "knn":
            return _native.minkowski_knn(xp, xp, k, first=1)
        return _native.minkowski_eps(xp, xp, _native.CMP_LE, eps)
    xc = _native.cosine_prep(X)
    if mode == "knn":
        return getattr(_native, version + "_knn")(xc, xc, k, first=1)
    return getattr(_native, version + "_eps")(xc, xc, _native.CMP_LE, eps)


def calibrate(version, X, k):
    """The quantile of the 16th-neighbour value that gives closest to 16 neighbours per row."""
    d16 = run(version, X, "knn", 16, None)[1][:, 15].float()
    cand = [float(d16.quantile(q).item()) for q in (0.5, 0.35, 0.25, 0.15, 0.1, 0.05)]
    return min(cand, key=lambda e: abs(int(run(version, X, "eps", k, e)[0][-1]) / X.shape[0] - 16))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="knn64,knn1280,eps64,eps1280")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = _native.device()
    res = {"tool": "euclid_ab", "reps": a.reps, "device": _native.device_info(), "peak_f16_flops": PEAK_F16, "shapes": {}}
    for name in a.shapes.split(","):
        n, d, mode = SHAPES[name]
        g = torch.Generator(device="cpu").manual_seed(20260104)                 # bench.py's embedding data
        X = torch.randn((n, d), generator=g, dtype=torch.float32).to(torch.float16).to(dev)
        k = 16
        eps = dict.fromkeys(VERSIONS)
        if mode == "eps":
            eps["euclidean"], eps["cosine"] = calibrate("euclidean", X, k), calibrate("cosine", X, k)
            eps["minkowski"] = eps["euclidean"]
        reps = a.reps if d <= 64 else max(3, a.reps // 2)
        fns = {v: (lambda v=v: run(v, X, mode, k, eps[v])) for v in VERSIONS}
        t = {v: [] for v in VERSIONS}
        for v in VERSIONS:                                                       # warm-up
            timed(fns[v])
        t_wall = time.perf_counter()
        info = {}
        for r in range(reps):
            order = VERSIONS[r % 3:] + VERSIONS[:r % 3]
            outs = {}
            for v in order:
                ms, outs[v] = timed(fns[v])
                t[v].append(ms)
            if r == 0 and mode == "knn":
                e, m = torch.sort(outs["euclidean"][0], dim=1)[0], torch.sort(outs["minkowski"][0], dim=1)[0]
                info["rows_with_minkowski_neighbour_set"] = float((e == m).all(1).float().mean())
            elif r == 0:
                info["nnz_per_row"] = {v: int(outs[v][0][-1]) / n for v in VERSIONS}
                # rows beyond the slot capacity cost a second, restricted sweep (a wave per 32 of them over all columns)
                info["rows_over_cap_256"] = {v: int((torch.diff(outs[v][0]) > 256).sum()) for v in VERSIONS}
                info["largest_row"] = {v: int(torch.diff(outs[v][0]).max()) for v in VERSIONS}
            del outs
        floor_ms = 2.0 * n * n * d / PEAK_F16 * 1e3
        rec = {"N": n, "D": d, "mode": mode, "k": k if mode == "knn" else None, "eps": eps if mode == "eps" else None, **info,
               "wall_s": round(time.perf_counter() - t_wall, 2), "mfma_floor_ms": floor_ms}
        for v in VERSIONS:
            rec[v] = {"median_ms": float(np.median(t[v])), "min_ms": float(np.min(t[v])), "max_ms": float(np.max(t[v])),
                      "all_ms": [round(x, 3) for x in t[v]]}
        rec["euclidean_over_cosine"] = rec["euclidean"]["median_ms"] / rec["cosine"]["median_ms"]
        rec["euclidean_over_minkowski"] = rec["euclidean"]["median_ms"] / rec["minkowski"]["median_ms"]
        rec["floor_share"] = floor_ms / rec["euclidean"]["median_ms"]
        res["shapes"][name] = rec
        print(f"# {name}: euclidean {rec['euclidean']['median_ms']:.2f} ms, cosine {rec['cosine']['median_ms']:.2f} ms "
              f"(x{rec['euclidean_over_cosine']:.3f}), minkowski {rec['minkowski']['median_ms']:.2f} ms, "
              f"floor share {rec['floor_share']:.3f} {info}", file=sys.stderr, flush=True)
        del X
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
