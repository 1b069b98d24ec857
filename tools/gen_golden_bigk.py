#!/usr/bin/env python3
"""
Reference goldens for Minkowski kNN graphs beyond 63 neighbours -> tests/golden/minkowski_f16_bigk.npz.

Runs the real reference's `build_graph(representation="Embedded", distance=minkowski, k=...)` on the CPU through
oracle/gen_golden.py's harness (its `quiet`, the stable-sort `proxy` and `make_csv`), on the seeded d2 / d64
embeddings that oracle/gen_golden.py wrote to tests/golden/minkowski_f16.npz.  Test infrastructure: it needs the
reference checkout, so it runs only where that exists; the tests read the .npz alone.

    d2   (300 x 2, dense with ties):  k = 100, 299; k = 400 clamps to 299 and is asserted equal to it, not stored
    d64  (1000 x 64):                 k = 100, with and without similarity
Indices int32, weights the reference's fp16 (the file stays under 1 MB).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_bigk.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np                                          # noqa: E402

from oracle import gen_golden as G                          # noqa: E402

CASES = {"d2": [(100, False), (299, False), (400, False)], "d64": [(100, False), (100, True)]}


def main():
    from prograph.distance import minkowski as ref_mink
    src = np.load(os.path.join(G.OUT, "minkowski_f16.npz"))
    out = {}
    G.proxy.stable = True
    with tempfile.TemporaryDirectory() as tmp:
        for name, cases in CASES.items():
            emb = src[f"{name}_emb"]
            n = emb.shape[0]
            tok = G.synth.clustered_tokens(n, 8, seed=G.synth.DEFAULT_SEED + 7)
            pg = G.quiet(G.Prograph, file=G.make_csv(tmp, "bigk_" + name, tok, 5))
            pg.graph["Embedded"] = list(emb)
            for k, sim in cases:
                L = G.quiet(pg.build_graph, representation="Embedded", k=k, similarity=sim, distance=ref_mink)
                key = f"{name}_knn{k}" + ("_sim" if sim else "")
                if k >= n:
                    want = f"{name}_knn{n - 1}"
                    assert np.array_equal(np.stack([x[0] for x in L]), out[want + "_idx"])
                    assert np.array_equal(np.stack([x[1] for x in L]).view(np.int16), out[want + "_w"].view(np.int16))
                    continue
                out[key + "_idx"] = np.stack([x[0] for x in L]).astype(np.int32)
                out[key + "_w"] = np.stack([x[1] for x in L]).astype(np.float16)
    G.proxy.stable = False
    path = os.path.join(G.OUT, "minkowski_f16_bigk.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
