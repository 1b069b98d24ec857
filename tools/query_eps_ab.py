"""
Radius (eps) search of queries against a dataset (Prograph.search(eps=)): the fused query kernel pair against the staged
path and the torch generic loop, alternated in one process after a warm-up, outputs compared for identity.  Each time is
the whole call on a host clock, from the call to the end of a device synchronise, so the one host sync of every version
(nnz) is inside it.

  Hamming (N = 200 000, L = 64, eps = 2, comp = le, Q in {1, 100, 10 000}; clustered tokens, a quarter of the queries
  copies of dataset rows, a quarter dataset rows with 1-3 substitutions, the rest random)
    fused    _native.query_eps: pg_query_eps_count, scan, pg_query_eps_fill (column pieces, two sweeps)
    staged   pg_hamming_dense into a (Q, N) fp16 block, then pg_f16_eps_* with keep-zero
    torch    the generic loop: the hamming operator's (Q, N) block, torch.where(d <= eps)
  Minkowski (N = 50 000, D in {64, 1280}, eps = 0.2 sqrt(D), Q in {1, 1 000}; bench.py's embedding data, queries = rows
  plus noise of 0.1 per coordinate)
    fused    pg_minkowski_eps_* with keep-zero (16 queries per workgroup)
    staged   pg_minkowski_dense + pg_f16_eps_* with keep-zero (what search() takes below 4096 queries)

indptr, indices and weights must be identical across the versions.  Prints one JSON line (per shape the median / min /
max ms of each version and nnz); progress goes to stderr.

    python tools/query_eps_ab.py [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from prograph_amd import _native, synth  # noqa: E402
from prograph_amd.distance import hamming  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def cat_csr(parts):
    if len(parts) == 1:
        return parts[0]
    base, ptrs = 0, [parts[0][0][:1]]
    for indptr, _, _ in parts:
        ptrs.append(indptr[1:] + base)
        base += int(indptr[-1].item())
    return torch.cat(ptrs), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts])


def generic(op, X, Y, eps):
    rows = max(1, min(Y.shape[0], (1 << 26) // X.shape[0]))
    parts = []
    for r0 in range(0, Y.shape[0], rows):
        d = op(X, Y[r0:r0 + rows])
        loc = torch.where(d <= eps)
        indptr = torch.zeros(d.shape[0] + 1, dtype=torch.int64, device=d.device)
        indptr[1:] = torch.cumsum(torch.bincount(loc[0], minlength=d.shape[0]), 0)
        parts.append((indptr, loc[1].to(torch.int32), d[loc]))
    return cat_csr(parts)


def staged_f16(block_fn, q, n, eps):
    rows = max(1, min(q, (1 << 27) // n))
    return cat_csr([_native.f16_eps(block_fn(r0, min(q, r0 + rows)), _native.CMP_LE, eps, keep_zero=True)
                    for r0 in range(0, q, rows)])


def same(outs):
    ref = [t.cpu().numpy().astype(np.float64) for t in outs[0]]
    return all(all(np.array_equal(t.cpu().numpy().astype(np.float64), r) for t, r in zip(o, ref)) for o in outs[1:])


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
    res["nnz"] = int(next(iter(outs.values()))[1].numel())
    print(name, json.dumps(res), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _native.device()
    out = {"device": _native.device_info()["arch"], "reps": args.reps, "shapes": {}}

    n, l, eps = 200_000, 64, 2
    X = synth.clustered_tokens(n, l, seed=11)
    dp = _native.pack(torch.as_tensor(X), bits=5)
    Xd = torch.as_tensor(X, device=dev)
    rng = np.random.default_rng(3)
    for q in (1, 100, 10_000):
        Y = rng.integers(1, 21, size=(q, l)).astype(np.uint8)
        Y[: q // 2] = X[rng.integers(0, n, size=q // 2)]
        for i in range(q // 4):                                                 # 1-3 substitutions
            pos = rng.choice(l, size=int(rng.integers(1, 4)), replace=False)
            Y[i, pos] = rng.integers(1, 21, size=len(pos))
        Yd = torch.as_tensor(Y, device=dev)
        fns = {
            "fused": lambda: _native.query_eps(_native.pack(Yd, bits=5), dp, _native.CMP_LE, eps),
            "staged": lambda: staged_f16(lambda a, b: _native.hamming_dense(dp, _native.pack(Yd[a:b], bits=5), out_bytes=2),
                                         q, n, eps),
            "torch": lambda: generic(hamming, Xd, Yd, eps),
        }
        out["shapes"][f"hamming_n{n}_l{l}_q{q}"] = run(f"hamming q={q}", fns, args.reps)

    n = 50_000
    for d in (64, 1280):
        E = torch.as_tensor(np.random.default_rng(d).standard_normal((n, d)), dtype=torch.float16, device=dev)
        xp = _native.pack_f16(E)
        e = 0.2 * float(np.sqrt(d))
        for q in (1, 1000):
            Y = E[torch.as_tensor(rng.integers(0, n, size=q), device=dev)] + torch.randn((q, d), device=dev, dtype=torch.float16) * 0.1
            fns = {
                "fused": lambda: _native.minkowski_eps(xp, _native.pack_f16(Y), _native.CMP_LE, e, keep_zero=True),
                "staged": lambda: staged_f16(lambda a, b: _native.minkowski_dense(xp, _native.pack_f16(Y[a:b])), q, n, e),
            }
            out["shapes"][f"minkowski_n{n}_d{d}_q{q}"] = run(f"minkowski d={d} q={q}", fns, args.reps)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
