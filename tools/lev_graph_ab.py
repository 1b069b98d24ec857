"""
Timings behind DESIGN.md §4.12 (Levenshtein graphs), on one GPU.  Every time is a whole call on a host clock, from the
call to the end of a device synchronise, after a warm-up; arms alternate; inputs are seeded; medians with min / max.

  eps     N = 200 000, lengths 96..128 (bench cfg5's data): the fused epsilon graph, eps = 8, comp = le
          (`_native.levenshtein_eps` with its operand staging) against the banded kNN step of cfg5
          (`_native.levenshtein_knn(k=8, band=8)`, the code the parent commit has).  Both run the same bag filter and the
          same pair-once distance pass; the graph then counts, scans, syncs for the CSR size and fills, the kNN
          selects.  `stages` times the graph's parts with a synchronise after each, so the added launches are on
          record.  A sample of rows is compared: every in-band kNN entry with d > 0 is in the graph's row.
  dense   pg_levenshtein_dense, 8192 rows x N = 50 000, full-length rows (125..128), fp16 output: time, pairs/s, VALU
          lane-operations/s from the ISA's instruction count per text position (--valu-per-char) against the chip's
          256 CUs x 4 SIMD x 32 lanes x 2.4 GHz; beside it the host baseline, the C oracle's `lev_knn(band=128)` on
          `--cpu-rows` rows (OpenMP, all cores it finds).
  knn     N = 50 000 of the same data with 1 % unrelated rows mixed in, k = 16: the hybrid (banded first pass, dense
          kernel for the rows it leaves) against dense only (PG_LEV_ROUTE=dense); graphs compared for identity.

Prints one JSON line; progress goes to stderr.

    python tools/lev_graph_ab.py [--reps 9] [--knn-reps 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from prograph_amd import Prograph, _native, synth  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "runs": len(v)}


def alternate(fns, reps, log):
    for f in fns.values():
        f()                                                                    # warm-up (code objects loaded)
    times, outs = {k: [] for k in fns}, {}
    for _ in range(reps):
        for key, f in fns.items():
            t, outs[key] = timed(f)
            times[key].append(t)
    res = {k: stats(v) for k, v in times.items()}
    print(log, json.dumps(res), file=sys.stderr, flush=True)
    return res, outs


def eps_stages(tok, thr, cap, reps):
    """The entries `_native.levenshtein_eps` calls, with a synchronise after each part."""
    L, p, s = _native.lib(), _native._ptr, _native._stream
    parts = {k: [] for k in ("operand", "filter", "pairs", "count_scan_sync", "fill")}
    for _ in range(reps + 1):
        t, op = timed(lambda: _native.lev_operand(tok))
        n, dev = op.n, tok.device
        up, lo, kept = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
        si, sa = (torch.empty(n * cap, dtype=torch.int32, device=dev) for _ in range(2))
        sw = torch.empty(n * cap, dtype=torch.uint8, device=dev)
        indptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
        scratch = torch.empty(int(L.pg_scan_scratch_bytes(n)), dtype=torch.uint8, device=dev)
        tf, mx = timed(lambda: (_native._check(L.pg_lev_candidates_sym(p(op.prof), op.planes.npad, n, thr, cap, p(si), p(sw), p(sa),
                                                                       p(up), p(lo), s()), "filter"), int((up + lo).max()))[1])
        assert mx <= cap
        tp, _ = timed(lambda: _native._check(L.pg_lev_eps_pairs(p(op.tokens), n, op.l, op.tokens.stride(0), p(op.planes.buf),
                                                                op.planes.npad, p(op.lens), thr, cap, p(si), p(sw), p(sa), p(up),
                                                                p(lo), s()), "pairs"))
        tc, nnz = timed(lambda: (_native._check(L.pg_lev_eps_count(n, cap, _native.CMP_LE, thr, p(sw), p(up), p(lo), p(kept), s()), "count"),
                                 _native._check(L.pg_exclusive_scan(p(kept), n, p(indptr), p(scratch), s()), "scan"),
                                 int(indptr[-1].item()))[2])
        ix = torch.empty(nnz, dtype=torch.int32, device=dev)
        w = torch.empty(nnz, dtype=torch.uint8, device=dev)
        tl, _ = timed(lambda: _native._check(L.pg_lev_eps_fill(n, cap, _native.CMP_LE, thr, p(si), p(sw), p(up), p(lo), p(indptr),
                                                               p(ix), p(w), s()), "fill"))
        for k, v in zip(parts, (t, tf, tp, tc, tl)):
            parts[k].append(v)
    return {k: stats(v[1:]) for k, v in parts.items()}, nnz


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--knn-reps", type=int, default=3)
    ap.add_argument("--n-eps", type=int, default=200_000)
    ap.add_argument("--n-dense", type=int, default=50_000)
    ap.add_argument("--rows-dense", type=int, default=8192)
    ap.add_argument("--n-knn", type=int, default=50_000)
    ap.add_argument("--cpu-rows", type=int, default=64)
    ap.add_argument("--valu-per-char", type=float, default=62.0, help="VALU instructions per text position in the dense loop's ISA")
    ap.add_argument("--only", default="eps,dense,knn")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _native.device()
    out = {"device": _native.device_info()["arch"], "reps": args.reps}
    only = args.only.split(",")

    if "eps" in only:
        n = args.n_eps
        tok_host, _ = synth.clustered_varlen_tokens(n, Lmax=128, Lmin=96)
        tok = torch.as_tensor(tok_host, device=dev)
        fns = {"knn_k8_band8": lambda: _native.levenshtein_knn(tok, 8, band=8, cap=512),
               "eps8_graph": lambda: _native.levenshtein_eps(_native.lev_operand(tok), _native.CMP_LE, 8, cap=512)}
        res, outs = alternate(fns, args.reps, "eps")
        (kidx, kd), (indptr, indices, w) = outs["knn_k8_band8"], outs["eps8_graph"]
        ip, ix, ki, kdd = indptr.cpu().numpy(), indices.cpu().numpy(), kidx.cpu().numpy(), kd.cpu().numpy()
        ww = w.cpu().numpy()
        ok = True
        for r in np.random.default_rng(0).integers(0, n, 2000):
            row = dict(zip(ix[ip[r]:ip[r + 1]].tolist(), ww[ip[r]:ip[r + 1]].tolist()))
            ok &= all(row.get(int(c)) == int(d) for c, d in zip(ki[r], kdd[r]) if 0 < d <= 8)
        res.update(nnz=int(ix.size), knn_entries_found_in_graph=bool(ok), n=n)
        res["stages_synchronised"], _ = eps_stages(tok, 8, 512, args.reps)
        out["eps"] = res
        del tok, outs, kidx, kd, indptr, indices, w
        torch.cuda.empty_cache()

    if "dense" in only:
        n, m = args.n_dense, args.rows_dense
        tok_host, lens = synth.clustered_varlen_tokens(n, Lmax=128, Lmin=128)
        op = _native.lev_operand(torch.as_tensor(tok_host, device=dev))
        assert op.valid()
        res, outs = alternate({"dense_f16": lambda: _native.levenshtein_dense(op, op, out_bytes=2, rows=(0, m))}, args.reps, "dense")
        ms = res["dense_f16"]["median_ms"]
        chars = float(lens[:m].astype(np.int64).sum()) * n                     # text positions x pairs
        peak = 256 * 4 * 32 * 2.4e9
        t0 = time.perf_counter()
        from oracle import c_oracle as C
        ci, cd = C.lev_knn(tok_host, 8, band=128, row0=0, nrows=args.cpu_rows)
        cpu_s = time.perf_counter() - t0
        blk = outs["dense_f16"][:args.cpu_rows].to(torch.float32)
        s = torch.sort(blk, dim=1, stable=True)
        same = bool(np.array_equal(s[1][:, 1:9].cpu().numpy(), ci) and np.array_equal(s[0][:, 1:9].cpu().numpy().astype(np.uint8), cd))
        res.update(n=n, rows=m, pairs_per_s=m * n / (ms * 1e-3), valu_lane_ops_per_s=chars * args.valu_per_char / (ms * 1e-3),
                   valu_share_of_peak=chars * args.valu_per_char / (ms * 1e-3) / peak, valu_per_char=args.valu_per_char,
                   cpu_oracle={"rows": args.cpu_rows, "seconds": cpu_s, "pairs_per_s": args.cpu_rows * n / cpu_s,
                               "threads": os.cpu_count() if not os.environ.get("OMP_NUM_THREADS") else int(os.environ["OMP_NUM_THREADS"])},
                   first_rows_equal_the_oracle=same)
        out["dense"] = res
        del op, outs, blk, s
        torch.cuda.empty_cache()

    if "knn" in only:
        n = args.n_knn
        tok_host, _ = synth.clustered_varlen_tokens(n, Lmax=128, Lmin=96)
        rng = np.random.default_rng(5)
        for r in rng.choice(n, n // 100, replace=False):
            l = int(rng.integers(96, 129))
            tok_host[r] = 0
            tok_host[r, :l] = rng.integers(1, 21, l)
        pg = Prograph.__new__(Prograph)                                        # the graph builder alone: no file, no frame
        pg.tokenized = tok_host.astype(np.int64)

        def build(route):
            os.environ["PG_LEV_ROUTE"] = route
            try:
                return pg._build_graph_levenshtein(None, None, 16, False, "Tokenized", None)
            finally:
                del os.environ["PG_LEV_ROUTE"]
        res, outs = alternate({"hybrid": lambda: build(""), "dense_only": lambda: build("dense")}, args.knn_reps, "knn")
        h, d = outs["hybrid"], outs["dense_only"]
        res.update(n=n, k=16, identical=bool(torch.equal(h.idx, d.idx) and torch.equal(h.dist, d.dist)),
                   rows_left_to_dense=int((h.dist[:, 15] > 8).sum().item()))
        out["knn"] = res
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
