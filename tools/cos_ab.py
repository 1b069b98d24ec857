"""
Native cosine graphs against a torch baseline in one process (HIP events, warm-up, the two versions alternated).

  native  pg_cosine_prep + pg_cosine_knn (ranks 1..k), or pg_cosine_prep + pg_cosine_eps_slots + scan + compaction
          (+ the restricted sweep) with its one sync - what build_graph(distance=cosine) runs
  torch   rows normalised in fp32, then per block of rows torch.mm against all normalised rows (fp32 GEMM),
          d = 1 - s, and topk(k + 1) with rank 0 dropped / the threshold `(d <= eps) & (d > 0)` to a CSR

Shapes: cos64 / cos1280 (N = 50 000, kNN k = 16, bench.py's embedding data) and eps64 / eps1280 (the threshold that
gives closest to 16 neighbours per row).  Agreement is checked on every shape: kNN rank by rank the sorted distances
of the two versions within 2 (D 2^-24 + 2^-21); eps the rows whose neighbour counts differ may only differ by pairs
within twice that bound of eps or of 0 (the baseline's self pairs come out a few ulp above 0).
The matrix-core floor is 2 N^2 D FLOP at 2.5 PF dense F16.
Prints one JSON line: per shape the median / min / max ms of each version and the share of the floor.

    python tools/cos_ab.py [--reps 7] [--shapes cos64,cos1280,eps64,eps1280] [--out profiles/cos_ab.json]
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

SHAPES = {"cos64": (50_000, 64, "knn"), "cos1280": (50_000, 1280, "knn"),
          "eps64": (50_000, 64, "eps"), "eps1280": (50_000, 1280, "eps")}
PEAK_F16 = 2.5e15


def native(X, mode, k, eps):
    xc = _native.cosine_prep(X)
    if mode == "knn":
        return _native.cosine_knn(xc, xc, k, first=1)
    return _native.cosine_eps(xc, xc, _native.CMP_LE, eps)


def baseline(X, mode, k, eps, rows=4096):
    Xf = X.float()
    Xn = Xf / torch.linalg.vector_norm(Xf, dim=1, keepdim=True)
    parts = []
    for r0 in range(0, X.shape[0], rows):
        d = 1 - torch.mm(Xn[r0:r0 + rows], Xn.T)
        if mode == "knn":
            v, i = torch.topk(d, k + 1, dim=1, largest=False, sorted=True)
            parts.append((i[:, 1:], v[:, 1:]))
        else:
            hit = (d <= eps) & (d > 0)
            parts.append((hit.sum(1), torch.nonzero(hit)[:, 1].to(torch.int32), d[hit]))
    if mode == "knn":
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    counts = torch.cat([p[0] for p in parts])
    indptr = torch.zeros(X.shape[0] + 1, dtype=torch.int64, device=X.device)
    indptr[1:] = torch.cumsum(counts, 0)
    return indptr, torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def agree(a, b, mode, eps, bound):
    """kNN: sorted distances rank by rank within 2 * bound.  eps: every differing pair lies within 2 * bound of eps or 0."""
    if mode == "knn":
        wa, wb = torch.sort(a[1].float(), dim=1)[0], torch.sort(b[1].float(), dim=1)[0]
        return float((wa - wb).abs().max()) <= 2 * bound, {"max_rank_diff": float((wa - wb).abs().max())}
    def keyed(g):
        ip, ix, w = (t.cpu().numpy() for t in g)
        rows = np.repeat(np.arange(len(ip) - 1, dtype=np.int64), np.diff(ip))
        return rows * (1 << 32) + ix.astype(np.int64), w.astype(np.float64)
    ka, wa = keyed(a)
    kb, wb = keyed(b)
    only_a, only_b = np.setdiff1d(ka, kb), np.setdiff1d(kb, ka)
    w = np.concatenate([wa[np.searchsorted(ka, only_a)], wb[np.searchsorted(kb, only_b)]])
    ambiguous = (np.abs(w - eps) <= 2 * bound) | (w <= 2 * bound)      # at eps, or a self pair (the d > 0 rule)
    return bool(ambiguous.all()), {"pairs_differing": int(len(w)), "nnz_native": int(len(ka)), "nnz_torch": int(len(kb))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="cos64,cos1280,eps64,eps1280")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = _native.device()
    res = {"tool": "cos_ab", "reps": a.reps, "device": _native.device_info(), "peak_f16_flops": PEAK_F16, "shapes": {}}
    for name in a.shapes.split(","):
        n, d, mode = SHAPES[name]
        g = torch.Generator(device="cpu").manual_seed(20260104)                 # bench.py's embedding data
        X = torch.randn((n, d), generator=g, dtype=torch.float32).to(torch.float16).to(dev)
        bound = d * 2.0 ** -24 + 2.0 ** -21
        k, eps = 16, None
        if mode == "eps":        # the quantile of the 16th-neighbour distance that gives closest to 16 neighbours per row
            d16 = native(X, "knn", 16, None)[1][:, 15]
            cand = [float(d16.quantile(q).item()) for q in (0.5, 0.35, 0.25, 0.15, 0.1, 0.05)]
            eps = min(cand, key=lambda e: abs(int(native(X, mode, k, e)[0][-1]) / n - 16))
        reps = a.reps if d <= 64 else max(3, a.reps // 2)
        fns = {"native": lambda: native(X, mode, k, eps), "torch": lambda: baseline(X, mode, k, eps)}
        t = {"native": [], "torch": []}
        for v in fns:                                                            # warm-up
            timed(fns[v])
        t_wall = time.perf_counter()
        ok, info = True, {}
        for r in range(reps):
            order = ("native", "torch") if r % 2 == 0 else ("torch", "native")
            outs = {}
            for v in order:
                ms, outs[v] = timed(fns[v])
                t[v].append(ms)
            if r == 0:
                ok, info = agree(outs["native"], outs["torch"], mode, eps, bound)
            del outs
        floor_ms = 2.0 * n * n * d / PEAK_F16 * 1e3
        rec = {"N": n, "D": d, "mode": mode, "k": k if mode == "knn" else None, "eps": eps, "agree": bool(ok), **info,
               "wall_s": round(time.perf_counter() - t_wall, 2), "mfma_floor_ms": floor_ms}
        for v in t:
            rec[v] = {"median_ms": float(np.median(t[v])), "min_ms": float(np.min(t[v])), "max_ms": float(np.max(t[v])),
                      "all_ms": [round(x, 3) for x in t[v]]}
        rec["native_over_torch"] = rec["native"]["median_ms"] / rec["torch"]["median_ms"]
        rec["floor_share"] = floor_ms / rec["native"]["median_ms"]
        res["shapes"][name] = rec
        print(f"# {name}: native {rec['native']['median_ms']:.2f} ms, torch {rec['torch']['median_ms']:.2f} ms "
              f"(x{rec['native_over_torch']:.3f}), floor share {rec['floor_share']:.3f}, agree={ok} {info}",
              file=sys.stderr, flush=True)
        del X
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["agree"] for r in res["shapes"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
