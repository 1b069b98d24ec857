"""
Whole-call times of the graph operations (pg_graph.hip) beside the route a user had without them.

    python tools/graph_ops_time.py [--out profiles/graph_ops.txt] [--small]

Every figure is a host clock from the call to the end of a device synchronise: one warm-up, then the median of 5 with min..max.
No GPU: the script fails (a CPU run says nothing about these times).

  graphs    the cfg3 kNN graph (N = 200 000, L = 64, k = 16) and the cfg2 eps graph (N = 50 000, L = 32, d <= 2) of bench.py
  device    `transpose()`, `symmetrize("union")`, `symmetrize("mutual")` on the device containers, results checked against the
            host route's once (same pattern; the weights where no entry repeats)
  host      what a user had before: `g.host()` -> scipy.sparse -> `A.T.tocsr()`, `A.maximum(A.T)` or `A.minimum(A.T)` -> three
            tensors back on the device.  scipy treats a missing entry as 0, so maximum is the union and minimum the mutual graph
            of positive weights - the pattern the user wants, though the union's weights are max, not min.
  tiers     `sorted()` of synthetic graphs of about 2^20 entries in rows of ONE length each: the time per key of the sort's tiers
            (PG_GRAPH_T1 = 64: one wave, PG_GRAPH_T2 = 4096: LDS of one workgroup, beyond: global memory with LDS runs),
            and one hub row of 2^20 entries, which a single workgroup sorts
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from prograph_amd import _native, synth                                   # noqa: E402
from prograph_amd.graph import CSRGraph, KNNGraph                         # noqa: E402


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts), out


def host_route(g, op):
    from scipy import sparse
    indptr, idx, w = g.as_csr().host() if isinstance(g, KNNGraph) else g.host()
    A = sparse.csr_matrix((w.astype(np.float32), idx, indptr), shape=(g.nrows, g.ncols))
    B = {"transpose": lambda: A.T.tocsr(), "union": lambda: A.maximum(A.T), "mutual": lambda: A.minimum(A.T)}[op]()
    B = sparse.csr_matrix(B)
    B.sort_indices()
    dev = g.indptr.device if isinstance(g, CSRGraph) else g.idx.device
    return (torch.from_numpy(B.indptr.astype(np.int64)).to(dev), torch.from_numpy(B.indices.astype(np.int32)).to(dev),
            torch.from_numpy(B.data).to(dev))


def device_route(g, op):
    s = g.transpose() if op == "transpose" else g.symmetrize(op, combine="max" if op == "union" else "min")
    return s.indptr, s.indices, s.weights


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="a tenth of the sizes: a rehearsal")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    dev = _native.device()
    shrink = 10 if a.small else 1
    lines = [f"graph operations, whole calls, ms: median of 5 (min..max) after one warm-up; {_native.device_info()['arch']}"]

    graphs = {}
    tok = torch.from_numpy(synth.clustered_tokens(200_000 // shrink, 64, members=256)).to(dev)
    planes = _native.pack(tok, bits=5)
    graphs["cfg3 kNN 200000 x 16"] = KNNGraph(*_native.knn_graph(planes, planes, 16), planes.n)
    tok = torch.from_numpy(synth.clustered_tokens(50_000 // shrink, 32, members=256)).to(dev)
    planes = _native.pack(tok, bits=5)
    graphs["cfg2 eps d<=2 N=50000"] = CSRGraph(*_native.eps_graph(planes, planes, _native.CMP_LE, 2, cap=256), planes.n)

    lines.append(f"{'graph':24s} {'nnz':>9s} {'operation':10s} {'device':>24s} {'host route':>28s} {'host/device':>11s} {'nnz out':>9s}")
    for name, g in graphs.items():
        c = g.as_csr() if isinstance(g, KNNGraph) else g
        nnz, zeros = c.nnz, int((c.weights == 0).sum())                      # scipy drops a zero weight: no entry to it
        for op in ("transpose", "union", "mutual"):
            d = timed(lambda: device_route(g, op))
            h = timed(lambda: host_route(g, op))
            same = all(torch.equal(x, y) for x, y in zip(d[3][:2], h[3][:2])) and torch.equal(d[3][2].to(torch.float32), h[3][2])
            lines.append(f"{name:24s} {nnz:9d} {op:10s} {d[0]:9.3f} ({d[1]:.3f}..{d[2]:.3f}) {h[0]:11.3f} ({h[1]:.3f}..{h[2]:.3f}) "
                         f"{h[0] / d[0]:10.1f}x {d[3][1].numel():9d}{'' if same else f'  results differ ({zeros} zero weights)'}")

    lines.append("")
    lines.append("sorted() of rows of one length, about 2^20 keys in all (whole call: keys, sort, scan, one host read, fill)")
    lines.append(f"{'row length':>10s} {'rows':>8s} {'tier':>6s} {'ms':>24s} {'ns/key':>8s}")
    total = (1 << 20) // shrink
    rng = np.random.default_rng(0)
    for length in (16, 64, 65, 256, 1024, 4096, 4097, 16384, 65536, 262144, total):
        rows = max(total // length, 1)
        indptr = torch.arange(0, rows * length + 1, length, dtype=torch.int64, device=dev)
        indices = torch.from_numpy(rng.integers(0, 1 << 20, rows * length).astype(np.int32)).to(dev)
        g = CSRGraph(indptr, indices, torch.zeros(rows * length, dtype=torch.uint8, device=dev), 1 << 20)
        t = timed(lambda: g.sorted())
        s = t[3]
        key = s.indices.to(torch.int64) + (1 << 20) * torch.repeat_interleave(torch.arange(rows, device=dev), length)
        assert bool((key[1:] >= key[:-1]).all()) and s.nnz == rows * length
        tier = 1 if length <= 64 else 2 if length <= 4096 else 3
        lines.append(f"{length:10d} {rows:8d} {tier:6d} {t[0]:10.3f} ({t[1]:.3f}..{t[2]:.3f}) {t[0] * 1e6 / (rows * length):8.2f}")

    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
