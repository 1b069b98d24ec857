"""
Digests of what `build_graph(..., output="csr")` and `search(..., output="csr")` return on every staged route ("dense
block -> selection kernel"): one line per case with the container's type, each array's dtype and shape
and a SHA-256 of its bytes.  Two trees compute the same graphs iff their outputs are equal line for line; a case that
raises prints the exception instead.  The public API only, fixed seeds, every case once with `Prograph._BLOCK_ELEMS` as
it is and once so small that a graph and a search are cut into at least three blocks.

  python tools/route_digest.py [--only SUBSTRING] [--out FILE] [--summary FILE]
  python tools/route_digest.py --summarise FILE    the summary of a full output written earlier with --out; nothing runs

The summary (what profiles/route_digest.txt keeps of a run, the full output being 300 kB) has one line per route and
block setting: the number of its cases, how many of them raised, and a SHA-256 over its full lines.  Where two
summaries differ, `--only ROUTE` prints that route's cases.
  python tools/route_digest.py --fake      the CPU stand-ins of tests/fake_*.py instead of the kernels (no GPU; the
                                           Minkowski cases, which have no stand-in, are left out, the long widths shrink)
"""
import argparse
import contextlib
import hashlib
import io
import operator
import os
import shutil
import sys
import tempfile

import numpy as np
import pandas as pd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

from prograph_amd import Prograph, synth                                    # noqa: E402
from prograph_amd.distance import (alignment, fit_alignment, hamming, levenshtein, local_alignment, minkowski,      # noqa: E402
                                   semiglobal_alignment, substitution)

OPS = (("le", operator.le), ("lt", operator.lt), ("eq", operator.eq), ("ge", operator.ge))
LINES = []


def emit(line):
    LINES.append(line)
    print(line, flush=True)


def digest(name, fn):
    try:
        g = fn()
    except Exception as e:                                                  # an error is a behaviour too
        emit(f"{name} | {type(e).__name__}: {e}")
        return None
    names = ("indptr", "indices", "weights") if hasattr(g, "indptr") else ("idx", "dist")
    parts = [type(g).__name__ + (f" first={g.first}" if hasattr(g, "first") else "") + f" ncols={g.ncols} sim={g.similarity}"]
    for a in names:
        t = getattr(g, a).detach().cpu().contiguous()
        parts.append(f"{a} {str(t.dtype).replace('torch.', '')}{list(t.shape)} {hashlib.sha256(t.numpy().tobytes()).hexdigest()}")
    emit(f"{name} | " + " | ".join(parts))
    return g


def summary(lines):
    """One line per route and block setting (the first two words of a case's name), in the order of their first case."""
    groups = {}
    for line in lines:
        groups.setdefault(" ".join(line.split(" ", 2)[:2]), []).append(line)
    raised = lambda g: sum(not c.split(" | ")[1].startswith(("KNNGraph", "CSRGraph")) for c in g)     # noqa: E731
    out = [f"{key} | {len(g)} cases | {raised(g)} raised | {hashlib.sha256(chr(10).join(g).encode()).hexdigest()}"
           for key, g in groups.items()]
    return out + [f"all | {len(lines)} cases | {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()}"]


def cost_table(rng, a, top):
    C = np.triu(rng.integers(0, top + 1, (a, a)), 1)
    C[0, a - 1] = top
    return C + C.T


def score_table(rng, a, lo, hi, diag):
    S = np.triu(rng.integers(lo, hi + 1, (a, a)), 1)
    S = S + S.T
    S[np.arange(a), np.arange(a)] = rng.choice(np.asarray(diag), a)
    return S


def dataset(tmp, name, tok):
    f = os.path.join(tmp, name + ".csv")
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    with contextlib.redirect_stdout(io.StringIO()):
        P = Prograph(file=f)
    return P


def queries(tok, q, seed):
    """q rows of the dataset, two in three of them changed in a few places, one shortened."""
    rng = np.random.default_rng(seed)
    T = np.array(tok[rng.permutation(len(tok))[:q]], dtype=np.int64)
    for r in range(0, q, 3):
        l = int((T[r] > 0).sum())
        at = rng.integers(0, l, 3)
        T[r, at] = 1 + (T[r, at] + rng.integers(0, 19, 3)) % 20
    for r in range(1, q, 3):
        l = int((T[r] > 0).sum())
        T[r, max(1, l - 4):] = 0
    return T


def route(tag, P, Q, distance, representation="Tokenized", graph=True, lev=False, strings=True):
    """Every variant of one route: graph and search, k and eps."""
    kw = dict(distance=distance, representation=representation, output="csr")
    n = len(P)
    some = [7, 3, 50, 51, 90, 2, 110, 64, 65, 12, 13, 14, 99, 100, 1, 0, 33, 34, 35, 128]
    base = digest(f"{tag} search k=5", lambda: P.search(Q, k=5, **kw))
    if base is None or not hasattr(base, "dist"):
        e = 3.0
    else:
        e = float(np.median(base.dist[:, -1].float().cpu().numpy()))
    e_int, e_frac = (float(int(e)), int(e) + 0.5) if float(e).is_integer() or e > 4 else (e, e * 1.5)
    if graph:
        for k in (5, 70):
            digest(f"{tag} graph k={k}", lambda: P.build_graph(k=k, **kw))
        digest(f"{tag} graph k=12 of 9 rows", lambda: P.build_graph(k=12, idxs=list(range(9)), **kw))
        digest(f"{tag} graph k=5 of 1 row", lambda: P.build_graph(k=5, idxs=[3], **kw))
        digest(f"{tag} graph k=5 idxs list", lambda: P.build_graph(k=5, idxs=some, **kw))
        digest(f"{tag} graph k=5 similarity", lambda: P.build_graph(k=5, similarity=True, **kw))
        for name, comp in OPS:
            for eps in (e_int, e_frac):
                digest(f"{tag} graph eps={eps} {name}", lambda: P.build_graph(eps=eps, comp=comp, **kw))
        digest(f"{tag} graph eps={e_int} idxs list", lambda: P.build_graph(eps=e_int, idxs=some, **kw))
        digest(f"{tag} graph eps={e_int} similarity", lambda: P.build_graph(eps=e_int, similarity=True, **kw))
        if lev:
            digest(f"{tag} graph eps=0.5 le", lambda: P.build_graph(eps=0.5, **kw))
            digest(f"{tag} graph eps=1 lt", lambda: P.build_graph(eps=1, comp=operator.lt, **kw))
    digest(f"{tag} search k=70", lambda: P.search(Q, k=70, **kw))
    digest(f"{tag} search k={n + 10}", lambda: P.search(Q, k=n + 10, **kw))
    digest(f"{tag} search k=5 similarity", lambda: P.search(Q, k=5, similarity=True, **kw))
    for name, comp in OPS:
        for eps in (e_int, e_frac):
            digest(f"{tag} search eps={eps} {name}", lambda: P.search(Q, eps=eps, comp=comp, **kw))
    digest(f"{tag} search eps=0", lambda: P.search(Q, eps=0, **kw))
    digest(f"{tag} search eps=1e9", lambda: P.search(Q, eps=1e9, **kw))
    digest(f"{tag} search eps=1e9 ge", lambda: P.search(Q, eps=1e9, comp=operator.ge, **kw))
    digest(f"{tag} search eps={e_int} similarity", lambda: P.search(Q, eps=e_int, similarity=True, **kw))
    if strings:
        S = synth.tokens_to_strings(Q[:9])
        digest(f"{tag} search strings k=5", lambda: P.search(S, k=5, **kw))
        digest(f"{tag} search strings eps={e_int}", lambda: P.search(S, eps=e_int, **kw))
        digest(f"{tag} search one string k=5", lambda: P.search(S[0], k=5, **kw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fake", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--summary", default=None)
    ap.add_argument("--summarise", default=None)
    args = ap.parse_args()
    if args.summarise:
        print("\n".join(summary(open(args.summarise).read().splitlines())))
        return
    long_w = 200
    if args.fake:
        import pytest
        import fake_fit_native, fake_lev_long_native, fake_semiglobal_native, fake_sub_native      # noqa: E401
        mp = pytest.MonkeyPatch()
        for m in (fake_sub_native, fake_lev_long_native, fake_semiglobal_native, fake_fit_native):
            m.install(mp)
        long_w = 136

    rng = np.random.default_rng(11)
    C = cost_table(rng, 21, 9)
    S = score_table(rng, 21, -4, 1, np.arange(2, 6))
    tmp = tempfile.mkdtemp()
    tok300 = synth.clustered_tokens(300, 300, seed=5, members=20)
    tok300[77] = tok300[5]
    tok20, _ = synth.clustered_varlen_tokens(150, Lmax=20, Lmin=12, seed=5, members=10)
    tok20 = tok20.copy()
    tok20[7] = tok20[8]
    tokL, _ = synth.clustered_varlen_tokens(130, Lmax=long_w, Lmin=long_w - 50, seed=9, members=10)
    tokL = tokL.copy()
    tokL[0, :] = 1 + np.arange(long_w) % 20                                  # one row of the full width
    tokL[7] = tokL[8]
    P300, P20, PL = dataset(tmp, "h300", tok300), dataset(tmp, "s20", tok20), dataset(tmp, "long", tokL)
    P20.embedding([np.random.default_rng(100 + i).normal(0, 1, 24).astype(np.float16) for i in range(len(P20))], "e")
    Q300, Q20, QL = queries(tok300, 150, 1), queries(tok20, 9, 2), queries(tokL, 9, 3)
    QE = np.stack([np.random.default_rng(500 + i).normal(0, 1, 24).astype(np.float16) for i in range(9)])
    QE[0] = np.asarray(P20("e_embedded")[4])

    routes = [
        ("hamming300", P300, lambda t: route(t, P300, Q300, hamming)),
        ("levenshtein20", P20, lambda t: route(t, P20, Q20, levenshtein, lev=True)),
        ("levenshtein_long", PL, lambda t: route(t, PL, QL, levenshtein, lev=True)),
        ("substitution20", P20, lambda t: route(t, P20, Q20, substitution(C))),
        ("alignment20_linear", P20, lambda t: route(t, P20, Q20, alignment(C, 2))),
        ("alignment20_affine", P20, lambda t: route(t, P20, Q20, alignment(C, 2, gap_open=3))),
        ("alignment_long", PL, lambda t: route(t, PL, QL, alignment(C, 2, gap_open=3))),
        ("local20", P20, lambda t: route(t, P20, Q20, local_alignment(S, 3, gap_open=2))),
        ("local_long", PL, lambda t: route(t, PL, QL, local_alignment(S, 3, gap_open=2))),
        ("semiglobal20", P20, lambda t: route(t, P20, Q20, semiglobal_alignment(S, 3, gap_open=2))),
        ("semiglobal_long", PL, lambda t: route(t, PL, QL, semiglobal_alignment(S, 3, gap_open=2))),
        ("fit20", P20, lambda t: route(t, P20, Q20, fit_alignment(S, 3, gap_open=2))),
        ("fit_long", PL, lambda t: route(t, PL, QL, fit_alignment(S, 3, gap_open=2))),
    ]
    if not args.fake:
        routes.append(("minkowski_few_queries", P20,
                       lambda t: route(t, P20, QE, minkowski, representation="e_embedded", graph=False, strings=False)))
    default = Prograph._BLOCK_ELEMS
    for whole in (True, False):
        for tag, P, run in routes:
            if args.only and args.only not in tag:
                continue
            # room for three rows of distances to the dataset: 64-row blocks for a graph (the floor) and for the long
            # Hamming queries, 3 queries at a time (1 for int32 blocks) for every other search
            Prograph._BLOCK_ELEMS = default if whole else 3 * len(P)
            run(f"{'whole' if whole else 'blocks'} {tag}")
    Prograph._BLOCK_ELEMS = default
    shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    if args.summary:
        with open(args.summary, "w") as f:
            f.write("\n".join(summary(LINES)) + "\n")


if __name__ == "__main__":
    main()
