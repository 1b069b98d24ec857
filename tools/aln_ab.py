"""
Timings behind DESIGN.md §4.15 .. §4.19 (gapped alignment distance, linear and affine gap penalties; local and semi-global
alignment scores), on one GPU.  Every time is a whole call on a host clock,
from the call to the end of a device synchronise, after a warm-up; arms alternate; inputs are seeded and random;
medians with min / max.

  dense   pg_alignment_dense, 8192 rows x N = 50 000, fp16 output, 21 symbols, at two shapes: rows of 125..128 tokens
          (the shape pg_levenshtein_dense was measured at) and rows of exactly 64.  Time, pairs/s, cell updates/s
          (pairs x len x x len y) and the share of the VALU issue rate: the unrolled body of one outer step is
          VALU_PER_STEP[chunks] instructions in the ISA (523 for 8 chunks of 16 cells, 4.09 per cell), a wave runs one
          outer step per position of its longest X row, and 256 CUs x 4 SIMDs x 2.4 GHz instructions/s is the rate.
          Beside it, in the same run, as context: `pg_levenshtein_dense` (bit-parallel) and `pg_substitution_dense`
          (no recurrence) at the same shapes, and the blocked torch expression of the operator on --torch-rows rows.
  graph   build_graph(k = 16) at N = --n-graph with lengths 48..64: `_build_graph_alignment` against
          `_build_graph_generic` with the operator (--generic-reps runs: it takes long); graphs compared.
  affine  §4.16: `pg_alignment_affine_dense` (gap_open 11) beside `pg_alignment_dense` at the two dense shapes - time, the
          ratio of the two in the same run, cell updates/s, share of the VALU issue rate from AFFINE_VALU_PER_STEP.
  affine_graph  build_graph(k = 16) at N = --n-graph, lengths 48..64, with alignment(C, 5, gap_open=7): native against
          the generic loop with the operator; graphs compared.
  local   §4.17: `pg_alignment_local_dense` (a score table of -4..16 / -4..32, gap 1, gap_open 11) beside
          `pg_alignment_affine_dense` at the two dense shapes - time, the ratio of the two in the same run, cell updates/s,
          share of the VALU issue rate from LOCAL_VALU_PER_STEP; the first rows compared with the operator's torch
          expression.
  long    §4.18: `pg_alignment_long_dense` (gap 1, gap_open 11) at 4096 x 20 000 int32 on rows of 300..400 tokens, beside
          the operator's blocked torch expression on --torch-rows of the rows; the first rows compared.
  long_graph  build_graph(k = 16) at N = 20 000, lengths 200..400: the long route against the generic loop with the
          operator (`aln_long_ready` False); graphs compared.  Both write profiles/aln_long_ab.txt unless --out is given.
  semiglobal  §4.19: `pg_alignment_semiglobal_dense` beside `pg_alignment_local_dense` under the same score table (as
          `local`: -4..16 / -4..32, gap 1, gap_open 11) at the two dense shapes - time, the ratio of the two in the same
          run, the ratio SEMIGLOBAL_VALU_PER_STEP / LOCAL_VALU_PER_STEP it should sit near; the first rows compared with
          the operator's torch expression.
  semiglobal_long  `pg_alignment_semiglobal_long_dense` beside `pg_alignment_local_long_dense` at `long`'s shape (4096 x
          20 000 int32, rows of 300..400 tokens); the first rows compared with the operator's torch expression.  Both write
          profiles/aln_semiglobal_ab.txt unless --out is given.
  fit     §4.23: `pg_alignment_fit_dense` beside the unchanged `pg_alignment_semiglobal_dense` under the same score table at
          `semiglobal`'s two dense shapes - time and the ratio of the two in the same run (the loop body is the same; one fold
          after the loop fewer: a ratio near 1); the first rows compared with the operator's torch expression.
  fit_long  `pg_alignment_fit_long_dense` beside `pg_alignment_semiglobal_long_dense` at `long`'s shape.  Both write
          profiles/aln_fit_ab.txt unless --out is given.
  pmc     one dense call and nothing else: the program of a counters-only `rocprofv3 --pmc` run.

Prints one JSON line; progress goes to stderr.

    python tools/aln_ab.py [--reps 5] [--only dense,graph,affine,affine_graph,local,long,long_graph,semiglobal,semiglobal_long,fit,fit_long] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from prograph_amd import Prograph, _native  # noqa: E402
from prograph_amd.distance import alignment, fit_alignment, local_alignment, semiglobal_alignment  # noqa: E402

# VALU instructions of one outer step (one X symbol against 16 * chunks cells) in the gfx950 ISA of pg_aln_dense_kernel.
# Counted by hand from the compiler's assembly (`--save-temps`; the table is in profiles/aln_dense.txt).  Nothing keeps it
# in step with the kernel: after any change to csrc/pg_aln.hip, csrc/pg_aln_frame.h, their build flags or the compiler, count
# again and update both places, or `share_of_valu_issue` below is wrong without a sign of it.
VALU_PER_STEP = {1: 69, 2: 134, 3: 199, 4: 264, 5: 329, 6: 394, 7: 459, 8: 523}
# The same for pg_aln_affine_dense_kernel (profiles/aln_affine_dense.txt; here every v_* of the loop is counted), kept by
# hand in the same way.
AFFINE_VALU_PER_STEP = {1: 131, 2: 260, 3: 389, 4: 518, 5: 647, 6: 775, 7: 905, 8: 1033}
# The same for pg_aln_local_dense_kernel (profiles/aln_local_dense.txt), kept by hand in the same way.
LOCAL_VALU_PER_STEP = {1: 153, 2: 305, 3: 458, 4: 611, 5: 764, 6: 917, 7: 1070, 8: 1222}
# The same for pg_aln_semiglobal_dense_kernel (profiles/aln_semiglobal_dense.txt), kept by hand in the same way.
SEMIGLOBAL_VALU_PER_STEP = {1: 179, 2: 324, 3: 470, 4: 616, 5: 762, 6: 908, 7: 1054, 8: 1198}
ISSUE_RATE = 256 * 4 * 2.4e9


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "runs": len(v)}


def alternate(fns, reps, log, skip_after=None):
    """Medians of alternating windows; an arm named in `skip_after` is timed only that many times (the slow ones)."""
    skip_after = skip_after or {}
    for f in fns.values():
        f()                                                                    # warm-up (code objects loaded)
    times, outs = {k: [] for k in fns}, {}
    for r in range(reps):
        for key, f in fns.items():
            if r >= skip_after.get(key, reps):
                continue
            outs[key] = None
            t, outs[key] = timed(f)
            times[key].append(t)
    res = {k: stats(v) for k, v in times.items()}
    print(log, json.dumps(res), file=sys.stderr, flush=True)
    return res, outs


def random_table(rng, a, hi):
    C = np.triu(rng.integers(1, hi + 1, (a, a)), 1)
    return C + C.T


def varlen(rng, n, lo, hi, a):
    """(n, hi) uint8 rows of tokens 1..a-1 with lengths lo..hi, zero right-padded."""
    tok = rng.integers(1, a, (n, hi), dtype=np.uint8)
    lens = rng.integers(lo, hi + 1, n)
    tok[np.arange(hi)[None, :] >= lens[:, None]] = 0
    return tok, lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--generic-reps", type=int, default=1)
    ap.add_argument("--n", type=int, default=50_000)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--torch-rows", type=int, default=256)
    ap.add_argument("--n-graph", type=int, default=50_000)
    ap.add_argument("--only", default="dense,graph,affine,affine_graph")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = _native.device()
    out = {"device": _native.device_info()["arch"], "reps": args.reps, "library": os.path.basename(_native.LIB_PATH)}
    only = args.only.split(",")
    rng = np.random.default_rng(1)
    a = 21

    if "dense" in only or "pmc" in only:
        n, m, tr = args.n, args.rows, args.torch_rows
        for name, lo, hi in (("l125_128", 125, 128), ("l64", 64, 64)):
            C = random_table(rng, a, 2048 // hi)
            dist = alignment(C, 2048 // hi)
            host, lens = varlen(rng, n, lo, hi, a)
            tok = torch.from_numpy(host).to(dev)
            xo = _native.aln_operand(tok, a)
            cost = dist.device_cost()
            assert xo.valid()
            aln = lambda: _native.alignment_dense(xo, xo, cost, dist.gap, out_bytes=2, rows=(0, m))     # noqa: E731
            if "pmc" in only:
                aln()
                torch.cuda.synchronize()
                print(json.dumps({"pmc": "one dense call", "n": n, "rows": m, "shape": name}))
                return
            lo_ = _native.lev_operand(tok)
            so = _native.sub_operand(tok, a)
            fns = {"alignment_dense_f16": aln,
                   "levenshtein_dense_f16": lambda: _native.levenshtein_dense(lo_, lo_, out_bytes=2, rows=(0, m)),
                   "substitution_dense_f16": lambda: _native.substitution_dense(so, so, cost, out_bytes=2, rows=(0, m)),
                   "torch_expression": lambda: dist._torch_expression(tok, tok[:tr])}
            res, outs = alternate(fns, args.reps, name, skip_after={"torch_expression": args.torch_reps})
            same = bool(torch.equal(outs["alignment_dense_f16"][:tr].to(torch.int64), outs["torch_expression"]))
            ms = res["alignment_dense_f16"]["median_ms"]
            pairs = m * n / (ms * 1e-3)
            cells = float(lens[:m].astype(np.float64).sum() * lens.astype(np.float64).sum()) / (ms * 1e-3)
            # per wave: one outer step per position of its longest row, the body of the Y row's chunk count
            wave_max = np.pad(lens, (0, -len(lens) % 64)).reshape(-1, 64).max(axis=1).astype(np.float64).sum()
            body = np.array([VALU_PER_STEP[max(1, (int(l) + 15) // 16)] for l in lens[:m]], dtype=np.float64).sum()
            valu = wave_max * body / (ms * 1e-3)
            torch_pairs = tr * n / (res["torch_expression"]["median_ms"] * 1e-3)
            res.update(n=n, rows=m, lengths=[lo, hi], symbols=a, gap=dist.gap, pairs_per_s=pairs, cell_updates_per_s=cells,
                       valu_instructions_per_s=valu, share_of_valu_issue=valu / ISSUE_RATE, torch_rows=tr,
                       torch_pairs_per_s=torch_pairs, speedup_over_torch_expression=pairs / torch_pairs,
                       levenshtein_pairs_per_s=m * n / (res["levenshtein_dense_f16"]["median_ms"] * 1e-3),
                       substitution_pairs_per_s=m * n / (res["substitution_dense_f16"]["median_ms"] * 1e-3),
                       first_rows_equal_torch=same)
            out["dense_" + name] = res
            del outs, xo, lo_, so, tok, fns
            torch.cuda.empty_cache()

    if "graph" in only:
        n = args.n_graph
        C = random_table(rng, a, 12)
        dist = alignment(C, 5)
        tok, lens = varlen(rng, n, 48, 64, a)
        tok[1::2, 3:] = tok[0::2, 3:][:len(tok[1::2])]                         # near pairs, so that ranks are not all ties of noise
        tok = tok.astype(np.int64)
        pg = Prograph.__new__(Prograph)                                        # the graph builder alone: no file
        pg.tokenized = tok
        pg.graph = pd.DataFrame({"Tokenized": list(tok)})
        native = lambda: pg._build_graph_alignment(None, None, 16, False, "Tokenized", None, dist)     # noqa: E731
        res, outs = alternate({"native_k16": native}, args.reps, "graph")
        G = outs["native_k16"]
        times = []
        for _ in range(args.generic_reps):
            t, tuples = timed(lambda: pg._build_graph_generic(None, 8, None, 16, False, "Tokenized", dist, None))
            times.append(t)
        res["generic_loop_operator_k16"] = stats(times)
        gi = np.array([i for i, _ in tuples])
        gw = np.array([w for _, w in tuples])
        res.update(n=n, lengths=[48, 64], k=16, gap=5,
                   identical=bool(np.array_equal(G.idx.cpu().numpy(), gi) and np.array_equal(G.dist.cpu().numpy(), gw)),
                   speedup=res["generic_loop_operator_k16"]["median_ms"] / res["native_k16"]["median_ms"])
        out["graph"] = res
    if "affine" in only:
        n, m = args.n, args.rows
        rng = np.random.default_rng(2)
        for name, lo, hi in (("l125_128", 125, 128), ("l64", 64, 64)):
            top = (2048 - 11) // hi
            C = random_table(rng, a, top)
            dist = alignment(C, top, gap_open=11)
            host, lens = varlen(rng, n, lo, hi, a)
            tok = torch.from_numpy(host).to(dev)
            xo = _native.aln_operand(tok, a)
            cost = dist.device_cost()
            assert xo.valid()
            fns = {"alignment_affine_dense_f16": lambda: _native.alignment_affine_dense(xo, xo, cost, dist.gap, dist.gap_open,
                                                                                        out_bytes=2, rows=(0, m)),
                   "alignment_dense_f16": lambda: _native.alignment_dense(xo, xo, cost, dist.gap, out_bytes=2, rows=(0, m))}
            res, outs = alternate(fns, args.reps, "affine " + name)
            zero = _native.alignment_affine_dense(xo, xo, cost, dist.gap, 0, out_bytes=2, rows=(0, min(m, 256)))
            same = bool(torch.equal(zero, outs["alignment_dense_f16"][:256]))
            ms = res["alignment_affine_dense_f16"]["median_ms"]
            cells = float(lens[:m].astype(np.float64).sum() * lens.astype(np.float64).sum()) / (ms * 1e-3)
            wave_max = np.pad(lens, (0, -len(lens) % 64)).reshape(-1, 64).max(axis=1).astype(np.float64).sum()
            body = np.array([AFFINE_VALU_PER_STEP[max(1, (int(l) + 15) // 16)] for l in lens[:m]], dtype=np.float64).sum()
            valu = wave_max * body / (ms * 1e-3)
            res.update(n=n, rows=m, lengths=[lo, hi], symbols=a, gap=dist.gap, gap_open=dist.gap_open,
                       pairs_per_s=m * n / (ms * 1e-3), cell_updates_per_s=cells, valu_instructions_per_s=valu,
                       share_of_valu_issue=valu / ISSUE_RATE,
                       ratio_to_linear=ms / res["alignment_dense_f16"]["median_ms"], gap_open_zero_equals_linear=same)
            out["affine_" + name] = res
            del outs, xo, tok, fns, zero
            torch.cuda.empty_cache()

    if "affine_graph" in only:
        n = args.n_graph
        rng = np.random.default_rng(3)
        C = random_table(rng, a, 12)
        dist = alignment(C, 5, gap_open=7)
        tok, lens = varlen(rng, n, 48, 64, a)
        tok[1::2, 3:] = tok[0::2, 3:][:len(tok[1::2])]
        tok = tok.astype(np.int64)
        pg = Prograph.__new__(Prograph)
        pg.tokenized = tok
        pg.graph = pd.DataFrame({"Tokenized": list(tok)})
        native = lambda: pg._build_graph_alignment(None, None, 16, False, "Tokenized", None, dist)     # noqa: E731
        res, outs = alternate({"native_k16": native}, args.reps, "affine graph")
        G = outs["native_k16"]
        times = []
        for _ in range(args.generic_reps):
            t, tuples = timed(lambda: pg._build_graph_generic(None, 8, None, 16, False, "Tokenized", dist, None))
            times.append(t)
        res["generic_loop_operator_k16"] = stats(times)
        gi = np.array([i for i, _ in tuples])
        gw = np.array([w for _, w in tuples])
        res.update(n=n, lengths=[48, 64], k=16, gap=5, gap_open=7,
                   identical=bool(np.array_equal(G.idx.cpu().numpy(), gi) and np.array_equal(G.dist.cpu().numpy(), gw)),
                   speedup=res["generic_loop_operator_k16"]["median_ms"] / res["native_k16"]["median_ms"])
        out["affine_graph"] = res
    if "local" in only:
        n, m, tr = args.n, args.rows, args.torch_rows
        rng = np.random.default_rng(4)
        for name, lo, hi in (("l125_128", 125, 128), ("l64", 64, 64)):
            top = 2048 // hi                                                   # width * max(S) = 2048: the fp16 bound
            S = np.triu(rng.integers(-4, 1, (a, a)), 1)
            S = S + S.T + np.diag(rng.integers(top // 2, top + 1, a))
            S[1, 1] = top
            score = local_alignment(S, 1, gap_open=11)
            C = random_table(rng, a, (2048 - 11) // hi)
            dist = alignment(C, 1, gap_open=11)
            host, lens = varlen(rng, n, lo, hi, a)
            tok = torch.from_numpy(host).to(dev)
            xo = _native.aln_operand(tok, a)
            table, cost = score.device_score(), dist.device_cost()
            assert xo.valid()
            fns = {"alignment_local_dense_f16": lambda: _native.alignment_local_dense(xo, xo, table, score.gap, score.gap_open,
                                                                                      out_bytes=2, rows=(0, m)),
                   "alignment_affine_dense_f16": lambda: _native.alignment_affine_dense(xo, xo, cost, dist.gap, dist.gap_open,
                                                                                        out_bytes=2, rows=(0, m))}
            res, outs = alternate(fns, args.reps, "local " + name)
            same = bool(torch.equal(outs["alignment_local_dense_f16"][:tr].to(torch.int64), score._torch_expression(tok, tok[:tr])))
            ms = res["alignment_local_dense_f16"]["median_ms"]
            cells = float(lens[:m].astype(np.float64).sum() * lens.astype(np.float64).sum()) / (ms * 1e-3)
            wave_max = np.pad(lens, (0, -len(lens) % 64)).reshape(-1, 64).max(axis=1).astype(np.float64).sum()
            body = np.array([LOCAL_VALU_PER_STEP[max(1, (int(l) + 15) // 16)] for l in lens[:m]], dtype=np.float64).sum()
            valu = wave_max * body / (ms * 1e-3)
            res.update(n=n, rows=m, lengths=[lo, hi], symbols=a, gap=score.gap, gap_open=score.gap_open, max_score=score.max_score,
                       pairs_per_s=m * n / (ms * 1e-3), cell_updates_per_s=cells, valu_instructions_per_s=valu,
                       share_of_valu_issue=valu / ISSUE_RATE,
                       ratio_to_affine=ms / res["alignment_affine_dense_f16"]["median_ms"],
                       expected_ratio_from_instruction_counts=LOCAL_VALU_PER_STEP[8] / AFFINE_VALU_PER_STEP[8],
                       torch_rows=tr, first_rows_equal_torch=same)
            out["local_" + name] = res
            del outs, xo, tok, fns
            torch.cuda.empty_cache()
    if "long" in only:
        # pg_alignment_long_dense at 4096 x 20 000 int32 on rows of 300..400 tokens, beside the blocked torch expression on
        # 256 of the rows
        n, m, tr = 20_000, 4096, args.torch_rows
        rng = np.random.default_rng(5)
        C = random_table(rng, a, 12)
        dist = alignment(C, 1, gap_open=11)
        host, lens = varlen(rng, n, 300, 400, a)
        tok = torch.from_numpy(host).to(dev)
        xo = _native.aln_long_operand(tok, a)
        cost = dist.device_cost()
        assert xo.valid() and _native.aln_long_fits(400, dist.max_cost, dist.gap, dist.gap_open)
        fns = {"alignment_long_dense_i32": lambda: _native.alignment_long_dense(xo, xo, cost, dist.gap, dist.gap_open, out_bytes=4,
                                                                                rows=(0, m)),
               "torch_expression_256_rows": lambda: dist._torch_expression(tok, tok[:tr])}
        res, outs = alternate(fns, args.reps, "long", skip_after={"torch_expression_256_rows": args.torch_reps})
        ms = res["alignment_long_dense_i32"]["median_ms"]
        res.update(n=n, rows=m, lengths=[300, 400], symbols=a, gap=dist.gap, gap_open=dist.gap_open, torch_rows=tr,
                   pairs_per_s=m * n / (ms * 1e-3),
                   cell_updates_per_s=float(lens[:m].astype(np.float64).sum() * lens.astype(np.float64).sum()) / (ms * 1e-3),
                   first_rows_equal_torch=bool(torch.equal(outs["alignment_long_dense_i32"][:tr].to(torch.int64),
                                                           outs["torch_expression_256_rows"])),
                   speedup_per_row=(res["torch_expression_256_rows"]["median_ms"] / tr) / (ms / m))
        out["long"] = res
        del outs, xo, tok, fns
        torch.cuda.empty_cache()
    if "long_graph" in only:
        # build_graph(k=16) at N = 20 000 with lengths 200..400: the long route, and the generic loop with the operator's
        # torch expression (aln_long_ready False)
        import tempfile
        from prograph_amd import synth             # not Prograph or pd again: a local import makes them locals of main() for every mode
        rng = np.random.default_rng(6)
        host, _ = varlen(rng, 20_000, 200, 400, a)
        with tempfile.TemporaryDirectory() as tmp:
            f = os.path.join(tmp, "long.csv")
            pd.DataFrame({"Sequence": synth.tokens_to_strings(host), "Fitness": rng.uniform(0, 1, len(host))}).to_csv(f)
            P = Prograph(file=f)
        dist = alignment(random_table(rng, a, 12), 1, gap_open=11)
        ready = _native.aln_long_ready

        def generic():
            _native.aln_long_ready = lambda: False
            try:
                return P.build_graph(k=16, distance=dist, output="csr")
            finally:
                _native.aln_long_ready = ready
        res, outs = alternate({"native_k16": lambda: P.build_graph(k=16, distance=dist, output="csr"), "generic_loop_operator_k16": generic},
                              args.reps, "long_graph", skip_after={"generic_loop_operator_k16": args.generic_reps})
        G, H = outs["native_k16"], outs["generic_loop_operator_k16"]
        res.update(n=20_000, lengths=[200, 400], k=16, gap=1, gap_open=11,
                   identical=bool(torch.equal(G.idx, H.idx) and torch.equal(G.dist.to(torch.int64), H.dist.to(torch.int64))),
                   speedup=res["generic_loop_operator_k16"]["median_ms"] / res["native_k16"]["median_ms"])
        out["long_graph"] = res
    if "semiglobal" in only:
        n, m, tr = args.n, args.rows, args.torch_rows
        rng = np.random.default_rng(7)
        for name, lo, hi in (("l125_128", 125, 128), ("l64", 64, 64)):
            top = 2048 // hi                                                   # width * max(S) = 2048: the fp16 bound
            S = np.triu(rng.integers(-4, 1, (a, a)), 1)
            S = S + S.T + np.diag(rng.integers(top // 2, top + 1, a))
            S[1, 1] = top
            score, local = semiglobal_alignment(S, 1, gap_open=11), local_alignment(S, 1, gap_open=11)
            host, lens = varlen(rng, n, lo, hi, a)
            tok = torch.from_numpy(host).to(dev)
            xo = _native.aln_operand(tok, a)
            table = score.device_score()
            assert xo.valid()
            fns = {"alignment_semiglobal_dense_f16": lambda: score._native_dense(xo, xo, 2, rows=(0, m)),
                   "alignment_local_dense_f16": lambda: _native.alignment_local_dense(xo, xo, table, local.gap, local.gap_open,
                                                                                      out_bytes=2, rows=(0, m))}
            res, outs = alternate(fns, args.reps, "semiglobal " + name)
            same = bool(torch.equal(outs["alignment_semiglobal_dense_f16"][:tr].to(torch.int64), score._torch_expression(tok, tok[:tr])))
            ms = res["alignment_semiglobal_dense_f16"]["median_ms"]
            cells = float(lens[:m].astype(np.float64).sum() * lens.astype(np.float64).sum()) / (ms * 1e-3)
            wave_max = np.pad(lens, (0, -len(lens) % 64)).reshape(-1, 64).max(axis=1).astype(np.float64).sum()
            chunks = [max(1, (int(l) + 15) // 16) for l in lens[:m]]
            body = np.array([SEMIGLOBAL_VALU_PER_STEP[c] for c in chunks], dtype=np.float64).sum()
            valu = wave_max * body / (ms * 1e-3)
            res.update(n=n, rows=m, lengths=[lo, hi], symbols=a, gap=score.gap, gap_open=score.gap_open, max_score=score.max_score,
                       pairs_per_s=m * n / (ms * 1e-3), cell_updates_per_s=cells, valu_instructions_per_s=valu,
                       share_of_valu_issue=valu / ISSUE_RATE,
                       ratio_to_local=ms / res["alignment_local_dense_f16"]["median_ms"],
                       expected_ratio_from_instruction_counts=body / np.array([LOCAL_VALU_PER_STEP[c] for c in chunks],
                                                                              dtype=np.float64).sum(),
                       torch_rows=tr, first_rows_equal_torch=same)
            out["semiglobal_" + name] = res
            del outs, xo, tok, fns
            torch.cuda.empty_cache()
    if "semiglobal_long" in only:
        n, m, tr = 20_000, 4096, args.torch_rows
        rng = np.random.default_rng(8)
        S = np.triu(rng.integers(-4, 1, (a, a)), 1)
        S = S + S.T + np.diag(rng.integers(4, 12, a))
        score, local = semiglobal_alignment(S, 1, gap_open=11), local_alignment(S, 1, gap_open=11)
        host, lens = varlen(rng, n, 300, 400, a)
        tok = torch.from_numpy(host).to(dev)
        xo = _native.aln_long_operand(tok, a)
        table = score.device_score()
        assert xo.valid() and score._long_fits(400, 400) and local._long_fits(400, 400)
        fns = {"alignment_semiglobal_long_dense_i32": lambda: score._native_long_dense(xo, xo, 4, rows=(0, m)),
               "alignment_local_long_dense_i32": lambda: _native.alignment_local_long_dense(xo, xo, table, local.gap, local.gap_open,
                                                                                            out_bytes=4, rows=(0, m))}
        res, outs = alternate(fns, args.reps, "semiglobal_long")
        ms = res["alignment_semiglobal_long_dense_i32"]["median_ms"]
        res.update(n=n, rows=m, lengths=[300, 400], symbols=a, gap=score.gap, gap_open=score.gap_open, max_score=score.max_score,
                   torch_rows=tr, pairs_per_s=m * n / (ms * 1e-3),
                   cell_updates_per_s=float(lens[:m].astype(np.float64).sum() * lens.astype(np.float64).sum()) / (ms * 1e-3),
                   ratio_to_local=ms / res["alignment_local_long_dense_i32"]["median_ms"],
                   first_rows_equal_torch=bool(torch.equal(outs["alignment_semiglobal_long_dense_i32"][:tr].to(torch.int64),
                                                           score._torch_expression(tok, tok[:tr]))))
        out["semiglobal_long"] = res
        del outs, xo, tok, fns
        torch.cuda.empty_cache()
    if "fit" in only:
        n, m, tr = args.n, args.rows, args.torch_rows
        rng = np.random.default_rng(7)
        for name, lo, hi in (("l125_128", 125, 128), ("l64", 64, 64)):
            top = (2048 - 11 - hi) // hi                                       # shifted scores stay fp16-exact: K + width * max(S) <= 2048
            S = np.triu(rng.integers(-4, 1, (a, a)), 1)
            S = S + S.T + np.diag(rng.integers(top // 2, top + 1, a))
            S[1, 1] = top
            score, semi = fit_alignment(S, 1, gap_open=11), semiglobal_alignment(S, 1, gap_open=11)
            host, lens = varlen(rng, n, lo, hi, a)
            tok = torch.from_numpy(host).to(dev)
            xo = _native.aln_operand(tok, a)
            K = score._select_bias(xo.l)
            assert xo.valid() and score._f16_route(xo.l, xo.l)
            fns = {"alignment_fit_dense_f16": lambda: score._native_dense(xo, xo, 2, rows=(0, m), bias=K),
                   "alignment_semiglobal_dense_f16": lambda: semi._native_dense(xo, xo, 2, rows=(0, m))}
            res, outs = alternate(fns, args.reps, "fit " + name)
            same = bool(torch.equal(outs["alignment_fit_dense_f16"][:tr].to(torch.int64) - K, score._torch_expression(tok, tok[:tr])))
            ms = res["alignment_fit_dense_f16"]["median_ms"]
            res.update(n=n, rows=m, lengths=[lo, hi], symbols=a, gap=score.gap, gap_open=score.gap_open, max_score=score.max_score,
                       bias=K, pairs_per_s=m * n / (ms * 1e-3),
                       cell_updates_per_s=float(lens[:m].astype(np.float64).sum() * lens.astype(np.float64).sum()) / (ms * 1e-3),
                       ratio_to_semiglobal=ms / res["alignment_semiglobal_dense_f16"]["median_ms"],
                       torch_rows=tr, first_rows_equal_torch=same)
            out["fit_" + name] = res
            del outs, xo, tok, fns
            torch.cuda.empty_cache()
    if "fit_long" in only:
        n, m, tr = 20_000, 4096, args.torch_rows
        rng = np.random.default_rng(8)
        S = np.triu(rng.integers(-4, 1, (a, a)), 1)
        S = S + S.T + np.diag(rng.integers(4, 12, a))
        score, semi = fit_alignment(S, 1, gap_open=11), semiglobal_alignment(S, 1, gap_open=11)
        host, lens = varlen(rng, n, 300, 400, a)
        tok = torch.from_numpy(host).to(dev)
        xo = _native.aln_long_operand(tok, a)
        assert xo.valid() and score._long_fits(400, 400) and semi._long_fits(400, 400)
        fns = {"alignment_fit_long_dense_i32": lambda: score._native_long_dense(xo, xo, 4, rows=(0, m)),
               "alignment_semiglobal_long_dense_i32": lambda: semi._native_long_dense(xo, xo, 4, rows=(0, m))}
        res, outs = alternate(fns, args.reps, "fit_long")
        ms = res["alignment_fit_long_dense_i32"]["median_ms"]
        res.update(n=n, rows=m, lengths=[300, 400], symbols=a, gap=score.gap, gap_open=score.gap_open, max_score=score.max_score,
                   torch_rows=tr, pairs_per_s=m * n / (ms * 1e-3),
                   cell_updates_per_s=float(lens[:m].astype(np.float64).sum() * lens.astype(np.float64).sum()) / (ms * 1e-3),
                   ratio_to_semiglobal=ms / res["alignment_semiglobal_long_dense_i32"]["median_ms"],
                   first_rows_equal_torch=bool(torch.equal(outs["alignment_fit_long_dense_i32"][:tr].to(torch.int64),
                                                           score._torch_expression(tok, tok[:tr]))))
        out["fit_long"] = res
        del outs, xo, tok, fns
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if args.out is None and ("fit" in only or "fit_long" in only):
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "aln_fit_ab.txt")
    if args.out is None and ("semiglobal" in only or "semiglobal_long" in only):
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "aln_semiglobal_ab.txt")
    if args.out is None and ("long" in only or "long_graph" in only):
        args.out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "aln_long_ab.txt")
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
