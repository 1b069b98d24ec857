"""
Times of the k-mer spectrum route on one device: medians of 5 after a warm-up, on the host clock to the
end of a synchronise.

  1. `pg_spectrum_profile` alone against the torch expression of `spectrum.embed` (`_torch_profiles`) on the same device
     tensor - the only yardstick that exists for it.
  2. `build_graph(distance=spectrum(...), k=16, output="csr")` whole against `build_graph(representation=<the same
     profiles stored with pg.embedding>, distance=cosine, k=16, output="csr")`: the second call is the route of stored
     embeddings, the difference is what the new route adds.

    python tools/spectrum_time.py [--n 50000] [--lmin 64] [--lmax 128] [--k 3] [--dims 0 1024] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prograph_amd import Prograph, _native            # noqa: E402
from prograph_amd.distance import cosine, spectrum    # noqa: E402
from prograph_amd.synth import AMINO                  # noqa: E402


def median_ms(fn, reps=5):
    fn()                                              # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--lmin", type=int, default=64)
    ap.add_argument("--lmax", type=int, default=128)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--dims", type=int, nargs="+", default=[0, 1024])
    ap.add_argument("--graph-k", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    rng = np.random.default_rng(1)
    tok = np.zeros((args.n, args.lmax), dtype=np.uint8)
    lens = rng.integers(args.lmin, args.lmax + 1, args.n)
    for r in range(args.n):
        tok[r, :lens[r]] = rng.integers(1, 21, lens[r])
    lut = np.array([""] + list(AMINO))
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "spectrum_time.csv")
        pd.DataFrame({"Sequence": ["".join(lut[r[r > 0]]) for r in tok], "Fitness": rng.uniform(0, 1, args.n)}).to_csv(f)
        pg = Prograph(file=f)
    dev = _native.device()
    tok_dev = torch.from_numpy(tok).to(dev)
    info = _native.device_info()
    lines = [f"k-mer spectrum on {info['arch']} ({info['cus']} CUs): N = {args.n}, lengths {args.lmin}..{args.lmax}, 20 symbols, k = {args.k}",
             "medians of 5 after a warm-up, host clock to the end of a synchronise", ""]
    lines.append("1. profiles: pg_spectrum_profile against the torch expression of embed on the same device tensor")
    lines.append(f"{'D':>8} {'kernel ms':>10} {'torch ms':>10} {'ratio':>7} {'profile MB':>11}")
    stored = {}
    for dims in args.dims:
        op = spectrum(k=args.k, symbols=20, dims=dims or None)
        got, flags = _native.spectrum_profile(tok_dev, op.k, op.symbols, op.dims)
        ref = op._torch_profiles(tok_dev)
        assert int(flags.item()) == 0 and torch.equal(got, ref)
        t_kernel = median_ms(lambda: _native.spectrum_profile(tok_dev, op.k, op.symbols, op.dims))
        t_torch = median_ms(lambda: op._torch_profiles(tok_dev))
        lines.append(f"{op.D:>8} {t_kernel:>10.3f} {t_torch:>10.3f} {t_torch / t_kernel:>7.1f} {args.n * op.D * 2 / 1e6:>11.1f}")
        stored[dims] = (op, got.cpu().numpy().astype(np.float32), t_kernel)
    lines += ["", f"2. build_graph(k={args.graph_k}, output=\"csr\"): the spectrum route against the same profiles stored with pg.embedding under cosine",
              f"{'D':>8} {'spectrum ms':>12} {'stored ms':>10} {'profile pass ms':>16} {'share':>6} {'staged MB':>10}"]
    for dims in args.dims:
        op, prof, t_kernel = stored[dims]
        name = f"p{dims}"
        pg.embedding(list(prof), name)
        a = pg.build_graph(distance=op, k=args.graph_k, output="csr")
        b = pg.build_graph(representation=f"{name}_embedded", distance=cosine, k=args.graph_k, output="csr")
        assert torch.equal(a.idx, b.idx) and torch.equal(a.dist, b.dist)
        t_new = median_ms(lambda: pg.build_graph(distance=op, k=args.graph_k, output="csr"))
        t_old = median_ms(lambda: pg.build_graph(representation=f"{name}_embedded", distance=cosine, k=args.graph_k, output="csr"))
        lines.append(f"{op.D:>8} {t_new:>12.2f} {t_old:>10.2f} {t_kernel:>16.3f} {t_kernel / t_new:>6.1%} {4 * args.n * op.D / 1e6:>10.1f}")
        del pg.graph[f"{name}_embedded"]
    lines += ["", "staged: the fp16 profiles (2 N D bytes) and their pg_pack_f16 copy (2 N D bytes); the stored route also reads the",
              "column from the host (np.vstack, the cast to fp16 and the upload), which the spectrum route does not."]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
