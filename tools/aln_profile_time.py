"""
The timing behind DESIGN.md §4.28 (profile queries), on one GPU: `pg_alignment_profile_dense` in local mode against
`pg_alignment_local_dense` on the SAME operands - Q (64) sequence profiles of 128 positions, P[j][a] = S[y_j][a], against N
(20 000) rows of 128 positions, int64 out - so that both kernels run the same cell loop over the same cells and only the
fill of the query profile differs (global reads instead of an LDS gather).  The local kernel is the one the token operators
run; this feature does not change it.

Every time is a window of --inner (5) calls on a host clock that ends in a device synchronise, after a warm-up of both
entries; the two alternate for --reps (10) windows; medians with min / max, and the ratio of the medians.  The two outputs
must be equal.  Prints one JSON line; writes profiles/aln_profile_dense.txt unless --out is given.

    python tools/aln_profile_time.py [--q 64] [--n 20000] [--reps 10] [--inner 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from prograph_amd import _native  # noqa: E402
from prograph_amd.distance import profile_alignment  # noqa: E402
from aln_ab import random_table, stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--q", type=int, default=64)
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "aln_profile_dense.txt")
    rng = np.random.default_rng(28)
    a, gap, gap_open, width = 21, 1, 11, 128
    S = random_table(rng, a, 20) - 4
    S[np.arange(a), np.arange(a)] = rng.integers(4, 17, a)
    X = rng.integers(1, a, (args.n, width), dtype=np.uint8)                   # every row 128 positions long
    Y = rng.integers(1, a, (args.q, width), dtype=np.uint8)
    xo, yo = _native.aln_operand(torch.from_numpy(X), a), _native.aln_operand(torch.from_numpy(Y), a)
    po = _native.profile_operand([profile_alignment.from_sequence(y, S) for y in Y])
    Sd = _native.aln_local_score(S)
    arms = {"local_dense": lambda: _native.alignment_local_dense(xo, yo, Sd, gap, gap_open, out_bytes=8),
            "profile_dense": lambda: _native.alignment_profile_dense("local", xo, po, gap, gap_open, out_bytes=8)}
    outs = {k: f() for k, f in arms.items()}                                 # the warm-up
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["local_dense"], outs["profile_dense"]))
    times = {k: [] for k in arms}
    for _ in range(args.reps):
        for k, f in arms.items():
            ms, _ = timed(lambda: [f() for _ in range(args.inner)][-1])
            times[k].append(ms / args.inner)
    cells = args.q * args.n * width * width
    res = {"q": args.q, "n": args.n, "positions": width, "gap": gap, "gap_open": gap_open, "reps": args.reps, "inner": args.inner,
           "device": _native.device_info(), "same_output": same, "cells": cells}
    for k, v in times.items():
        res[k] = {**stats(v), "cell_updates_per_s": cells / (float(np.median(v)) * 1e-3)}
    res["profile_over_local"] = res["profile_dense"]["median_ms"] / res["local_dense"]["median_ms"]
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
