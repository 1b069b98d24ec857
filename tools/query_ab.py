"""
kNN of queries against a dataset (Prograph.search): the fused query kernel against the staged path and the torch generic
loop, alternated in one process (HIP events, warm-up), outputs compared.

  Hamming (N = 200 000, L = 64, k = 16, Q in {1, 100, 10 000}; clustered tokens, half of the queries dataset rows)
    fused    _native.query_knn: pg_query_knn_hamming (column pieces + merge)
    staged   pg_hamming_dense into a (Q, N) fp16 block, then pg_f16_knn with first = 0
    torch    the generic loop: the hamming operator's (Q, N) int64 block, torch.sort(stable=True), ranks 0..k-1
  Minkowski (N = 50 000, D in {64, 1280}, k = 16, Q in {1, 1 000}; bench.py's embedding data)
    fused    pg_minkowski_knn with first = 0 (16 queries per workgroup)
    staged   pg_minkowski_dense + pg_f16_knn with first = 0 (what search() takes below 4096 queries)
    torch    the generic loop: the minkowski operator + torch.sort(stable=True)

Indices and weights must be identical across the three.  Prints one JSON line (per shape the median / min / max ms of
each version); progress goes to stderr.

    python tools/query_ab.py [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from prograph_amd import _native, synth  # noqa: E402
from prograph_amd.distance import hamming, minkowski  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def generic(op, X, Y, k):
    rows = max(1, min(Y.shape[0], (1 << 26) // X.shape[0]))
    idx, w = [], []
    for r0 in range(0, Y.shape[0], rows):
        s = torch.sort(op(X, Y[r0:r0 + rows]), dim=1, stable=True)
        idx.append(s[1][:, :k])
        w.append(s[0][:, :k])
    return torch.cat(idx), torch.cat(w)


def staged_f16(block_fn, q, n, k):
    rows = max(1, min(q, (1 << 27) // n))
    parts = [_native.f16_knn(block_fn(r0, min(q, r0 + rows)), k, first=0) for r0 in range(0, q, rows)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


def same(outs):
    ref_i, ref_w = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy().astype(np.float64)
    return all(np.array_equal(i.cpu().numpy(), ref_i) and np.array_equal(w.cpu().numpy().astype(np.float64), ref_w)
               for i, w in outs[1:])


def run(name, fns, reps):
    for f in fns.values():
        f()                                                                    # warm-up (and code objects loaded)
    times = {k: [] for k in fns}
    outs = {}
    for _ in range(reps):
        for key, f in fns.items():                                             # alternated
            t, outs[key] = timed(f)
            times[key].append(t)
    res = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in times.items()}
    res["identical"] = same(list(outs.values()))
    print(name, json.dumps(res), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _native.device()
    out = {"device": _native.device_info()["arch"], "reps": args.reps, "k": 16, "shapes": {}}
    k = 16

    n, l = 200_000, 64
    X = synth.clustered_tokens(n, l, seed=11)
    dp = _native.pack(torch.as_tensor(X), bits=5)
    Xd = torch.as_tensor(X, device=dev)
    rng = np.random.default_rng(3)
    for q in (1, 100, 10_000):
        Y = rng.integers(1, 21, size=(q, l)).astype(np.uint8)
        Y[: q // 2] = X[rng.integers(0, n, size=q // 2)]
        Yd = torch.as_tensor(Y, device=dev)
        fns = {
            "fused": lambda: _native.query_knn(_native.pack(Yd, bits=5), dp, k),
            "staged": lambda: staged_f16(lambda a, b: _native.hamming_dense(dp, _native.pack(Yd[a:b], bits=5), out_bytes=2),
                                         q, n, k),
            "torch": lambda: generic(hamming, Xd, Yd, k),
        }
        out["shapes"][f"hamming_n{n}_l{l}_q{q}"] = run(f"hamming q={q}", fns, args.reps)

    n = 50_000
    for d in (64, 1280):
        E = torch.as_tensor(np.random.default_rng(d).standard_normal((n, d)), dtype=torch.float16, device=dev)
        xp = _native.pack_f16(E)
        for q in (1, 1000):
            Y = E[torch.as_tensor(rng.integers(0, n, size=q), device=dev)] + torch.randn((q, d), device=dev, dtype=torch.float16) * 0.1
            fns = {
                "fused": lambda: _native.minkowski_knn(xp, _native.pack_f16(Y), k, first=0),
                "staged": lambda: staged_f16(lambda a, b: _native.minkowski_dense(xp, _native.pack_f16(Y[a:b])), q, n, k),
                "torch": lambda: generic(minkowski, E, Y, k),
            }
            out["shapes"][f"minkowski_n{n}_d{d}_q{q}"] = run(f"minkowski d={d} q={q}", fns, args.reps)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
