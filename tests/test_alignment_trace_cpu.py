"""
Alignment tracebacks (`op.align`, `Prograph.align`, prograph_amd/alignments.py) without a GPU.

The yardstick is tests/trace_testdata.py: `definition`, the canonical alignment of DESIGN.md §4.20 as plain loops over
single cells, `rescore`, which prices a list of ops from the table alone, and `brute_force`, every path of every admissible
pair of substrings.  Held against it here: the product's host expression (numpy rows, another walk), the kernel's own row
routine and walk compiled for the host under the address and undefined-behaviour sanitizers (tests/capi_trace), the host
logic of `Prograph.align` and `_native.alignment_trace` on the stand-in of tests/fake_trace_native.py, and the C ABI's
argument checks.  The kernel itself: tests/test_alignment_trace_gpu.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

import fake_aln_native
import fake_trace_native
from conftest import REPO
from trace_testdata import FIELDS, GLOBAL, LOCAL, SEMIGLOBAL, brute_force, definition, rescore, sequence
from prograph_amd import synth
from prograph_amd.alignments import Alignments
from prograph_amd.distance import alignment, levenshtein, local_alignment, semiglobal_alignment

A = 4
NEGATIVE = np.array([[3, -2, -1, -3], [-2, 4, -3, 1], [-1, -3, 2, -2], [-3, 1, -2, 5]])          # scores below zero
TRAP = np.array([[2, 3, 1, 2], [3, 1, -2, -1], [1, -2, 4, -3], [2, -1, -3, 2]])                  # S[a][0] > 0: padding must not pair
ONE_MINUS_I = 1 - np.eye(A, dtype=np.int64)
COSTS = np.array([[0, 2, 7, 1], [2, 0, 3, 9], [7, 3, 0, 4], [1, 9, 4, 0]])                       # C[a][0] > 0 likewise

CASES = [(alignment, GLOBAL, ONE_MINUS_I), (alignment, GLOBAL, COSTS)] + \
        [(cls, mode, S) for cls, mode in ((local_alignment, LOCAL), (semiglobal_alignment, SEMIGLOBAL))
         for S in (NEGATIVE, TRAP, ONE_MINUS_I)]


def all_lengths(rng, top=9, symbols=A):
    """Two (100, top) matrices: every pair of lengths 0..top, zeros inside the sequences, never at their ends."""
    X, Y = np.zeros(((top + 1) ** 2, top), dtype=np.int64), np.zeros(((top + 1) ** 2, top), dtype=np.int64)
    for p in range(len(X)):
        for M, l in ((X, p // (top + 1)), (Y, p % (top + 1))):
            M[p, :l] = rng.integers(0, symbols, l)
            if l:
                M[p, l - 1] = rng.integers(1, symbols)
    return X, Y


def same_as_definition(got, mode, T, gap, gap_open, X, Y, xi=None, yi=None):
    """Every field of an Alignments container against `definition`, pair by pair."""
    got = got.host()
    for f in FIELDS:
        assert getattr(got, f).dtype == torch.int64 and getattr(got, f).shape == (len(got),), f
    assert got.ops.dtype == torch.uint8
    for p in range(len(got)):
        want = definition(mode, T, gap, gap_open, X[p if xi is None else xi[p]], Y[p if yi is None else yi[p]])
        have = {f: int(getattr(got, f)[p]) for f in FIELDS}
        assert have == {f: want[f] for f in FIELDS}, (p, have, want)
        row = got.ops[p].tolist()
        assert row[:want["n_ops"]] == want["ops"] and not any(row[want["n_ops"]:]), (p, row, want["ops"])


@pytest.mark.parametrize("gap_open", [0, 11])
@pytest.mark.parametrize("gap", [1, 255])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_expression_is_the_definition(case, gap, gap_open):
    cls, mode, T = CASES[case]
    X, Y = all_lengths(np.random.default_rng(100 * case + gap + gap_open))
    op = cls(T, gap, gap_open=gap_open)
    got = op.align(torch.from_numpy(X), torch.from_numpy(Y))
    assert isinstance(got, Alignments) and len(got) == len(X) and got.score.device.type == "cpu"
    same_as_definition(got, mode, T, gap, gap_open, X, Y)
    # the invariants, on the product's output
    full = op(torch.from_numpy(X), torch.from_numpy(Y))                  # (M, N): row m is Y[m] against X[n]
    assert np.array_equal(got.score.numpy(), np.diag(full.numpy()))
    for p in range(len(X)):
        lx, ly = len(sequence(X[p])), len(sequence(Y[p]))
        n, ops = int(got.n_ops[p]), got.ops[p].tolist()
        xb, xe, yb, ye = (int(getattr(got, f)[p]) for f in ("x_begin", "x_end", "y_begin", "y_end"))
        value, i, j = rescore(mode, T, gap, gap_open, X[p], Y[p], xb, yb, ops[:n])
        assert value == int(got.score[p]) and (i, j) == (xe, ye), p                  # the ops are worth the score and
        assert 0 <= xb <= xe <= lx and 0 <= yb <= ye <= ly                           # consume exactly the stated ranges
        if mode == GLOBAL:
            assert (xb, xe, yb, ye) == (0, lx, 0, ly)
        elif mode == LOCAL:
            assert (n == 0 and (xb, xe, yb, ye) == (0, 0, 0, 0)) or (ops[0] == 1 and ops[n - 1] == 1)
        else:
            assert (xb == 0 or yb == 0) and (xe == lx or ye == ly)
        if lx <= 5 and ly <= 5:
            assert int(got.score[p]) == brute_force(mode, T, gap, gap_open, X[p], Y[p]), p
    ident = got.identity()
    assert ident.dtype == torch.float64 and ((ident >= 0) & (ident <= 1)).all()
    assert (ident[got.n_ops == 0] == 0).all()


def one(op, x, y):
    got = op.align(torch.tensor([x]), torch.tensor([y]))
    assert len(got) == 1
    return got


def test_ties_by_hand():
    # diagonal against gap: x = ab, y = b under 1 - I costs, gap 1: pairing a with b then gapping b costs 2, and so does
    # the other order; the walk back from (2, 1) finds H = H[1][0] + C[b][b] first: the pair is the LAST column
    got = one(alignment(ONE_MINUS_I, 1), [1, 2], [2])
    assert got.cigar(0) == "1X1M" and int(got.score[0]) == 1 and int(got.identities[0]) == 1
    assert got.gapped(0, "?ab") == ("ab", "-b")
    # a mismatch (cost 1) ties with two gaps at gap 1?  No: 2 > 1; at equal cost the diagonal wins
    got = one(alignment(np.array([[0, 2], [2, 0]]), 1), [1, 0, 1], [1, 1])
    assert int(got.score[0]) == 1 and got.cigar(0) in ("1M1X1M",) and got.gapped(0, "ab") == ("bab", "b-b")
    got = one(alignment(np.array([[0, 2, 2], [2, 0, 2], [2, 2, 0]]), 1), [1], [2])   # pair (2) against two gaps (2)
    assert got.cigar(0) == "1M" and int(got.identities[0]) == 0 and float(got.identity()[0]) == 0.0
    # open against extend at gap_open = 0: every step of a run ties, "open" wins and returns to state H, which finds the
    # run's next column through E again: one run all the same.  With gap_open = 2 the walk stays in E until the run opens
    got = one(alignment(ONE_MINUS_I, 1), [1, 2, 3], [1])
    assert got.cigar(0) == "1M2X" and int(got.score[0]) == 2
    assert definition(GLOBAL, ONE_MINUS_I, 1, 0, [1, 2, 3], [1])["ops"] == [1, 2, 2]
    got = one(alignment(ONE_MINUS_I, 1, gap_open=2), [1, 2, 3], [1])
    assert int(got.score[0]) == 4 and got.cigar(0) == "1M2X"
    got = one(alignment(ONE_MINUS_I, 1, gap_open=2), [1, 2, 3, 1], [1])  # 1M3X and 3X1M both cost 5: the diagonal first
    assert int(got.score[0]) == 5 and got.cigar(0) == "3X1M"
    # two equal maxima: the smallest i, then the smallest j
    S = np.array([[1, -3, -3], [-3, 2, -3], [-3, -3, 2]])
    got = one(local_alignment(S, 5), [1, 0, 2], [2, 0, 1])               # x_1 = y_3 and x_3 = y_1 both score 2
    assert (int(got.x_begin[0]), int(got.x_end[0]), int(got.y_begin[0]), int(got.y_end[0])) == (0, 1, 2, 3)
    assert got.cigar(0) == "1M" and float(got.identity()[0]) == 1.0
    got = one(semiglobal_alignment(S, 5), [1, 2, 1], [1])                # H[1][1] = H[3][1] = 2: the smaller i
    assert (int(got.x_begin[0]), int(got.x_end[0]), int(got.y_begin[0]), int(got.y_end[0])) == (0, 1, 0, 1)
    # local score 0: the empty alignment
    got = one(local_alignment(S, 1), [1, 1], [2, 2])
    assert int(got.score[0]) == 0 and int(got.n_ops[0]) == 0 and got.cigar(0) == "" and got.gapped(0) == ("", "")
    assert (int(got.x_begin[0]), int(got.x_end[0]), int(got.y_begin[0]), int(got.y_end[0])) == (0, 0, 0, 0)
    assert float(got.identity()[0]) == 0.0
    # a fragment in its parent, and the padding trap: the trailing zeros of the shorter row pair with nothing
    got = one(semiglobal_alignment(TRAP, 2), [2, 0, 2, 3, 0, 0], [1, 3, 2, 0, 2, 3, 1])
    assert got.cigar(0) == "4M" and (int(got.x_begin[0]), int(got.x_end[0]), int(got.y_begin[0]), int(got.y_end[0])) == (0, 4, 2, 6)
    assert got.gapped(0, "acgt") == ("gagt", "gagt") and int(got.identities[0]) == 4


def test_input_rules():
    op = local_alignment(NEGATIVE, 1)
    with pytest.raises(ValueError, match="outside the table"):
        op.align(torch.tensor([[1, 4]]), torch.tensor([[1, 2]]))
    with pytest.raises(ValueError):
        op.align(torch.zeros((0, 3), dtype=torch.int64), torch.tensor([[1, 2]]))
    with pytest.raises(ValueError, match="one row per pair"):
        op.align(torch.tensor([[1, 2], [2, 1]]), torch.tensor([[1, 2]]))
    with pytest.raises(ValueError, match="0..255"):
        op.align(torch.tensor([[1.5, 2]]), torch.tensor([[1, 2]]))
    assert not hasattr(levenshtein, "align") and "alignment(1 - I, 1)" in __import__("prograph_amd.distance.levenshtein", fromlist=["x"]).__doc__
    # beyond 2048 positions: still the host expression
    x = torch.ones((1, 2100), dtype=torch.int64)
    got = alignment(ONE_MINUS_I, 1).align(x, x[:, :2090])
    assert int(got.score[0]) == 10 and got.cigar(0) == "10X2090M"        # the diagonal wins every tie


def test_the_kernel_routines_on_the_host():
    """tests/capi_trace/trace_check.cpp: pg_aln_trace.h's row routine and walk, compiled for the host with
    -fsanitize=address,undefined, against a plain DP on a few thousand random pairs."""
    capi = os.path.join(REPO, "tests", "capi_trace")
    subprocess.check_call(["make", "-s", "-C", capi])
    out = subprocess.run([os.path.join(capi, "_build", "trace_check")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "trace routines OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_c_abi_argument_errors_without_gpu():
    from prograph_amd import _native
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                              # never dereferenced: every check is on the host
    one = ctypes.c_int64(0)
    assert lib.pg_alignment_trace_workspace(128, 128, ctypes.byref(one)) == 0 and one.value == 64 * 128 * 16 * 4
    assert lib.pg_alignment_trace_workspace(20, 9, ctypes.byref(one)) == 0 and one.value == 64 * 20 * 2 * 4
    assert _native.aln_trace_wave_bytes(20, 9) == one.value
    assert lib.pg_alignment_trace_workspace(129, 8, ctypes.byref(one)) == -2
    assert lib.pg_alignment_trace_workspace(0, 8, ctypes.byref(one)) == -1 and lib.pg_alignment_trace_workspace(8, 8, None) == -1

    def call(mode=0, x=p, n=4, xnpad=256, xl=20, y=p, m=4, ynpad=256, yl=9, xi=p, yi=p, npairs=3, table=p, gap=1, gap_open=0,
             head=p, ops=p, ldo=29, ws=p, ws_bytes=64 * 20 * 2 * 4):
        return lib.pg_alignment_trace(mode, x, n, xnpad, xl, y, m, ynpad, yl, xi, yi, npairs, table, gap, gap_open, head, ops,
                                      ldo, ws, ws_bytes, None)
    for bad in (dict(mode=3), dict(mode=-1), dict(gap=0), dict(gap=256), dict(gap_open=-1), dict(gap_open=256), dict(x=None),
                dict(y=None), dict(xi=None), dict(yi=None), dict(table=None), dict(head=None), dict(ops=None), dict(ws=None),
                dict(ldo=28), dict(ws_bytes=64 * 20 * 2 * 4 - 1), dict(npairs=0), dict(n=0), dict(xnpad=3), dict(ynpad=3)):
        assert call(**bad) == -1, bad
        assert b"pg_alignment_trace" in lib.pg_last_error()
    assert call(xl=129, ldo=300) == -2 and call(yl=129, ldo=300) == -2
    assert lib.pg_version() == 3


# ---------------------------------------------------------------- host logic through the stand-in
N, L = 60, 24


@pytest.fixture()
def pg(tmp_path, monkeypatch):
    fake_trace_native.install(monkeypatch)
    from prograph_amd import Prograph
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=10, seed=5, members=6)
    f = tmp_path / "trace.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    del fake_aln_native.calls[:]
    return P, tok


def _score_table(rng, a=21):
    S = rng.integers(-4, 2, (a, a))
    S = np.triu(S) + np.triu(S, 1).T
    S[np.arange(a), np.arange(a)] = rng.integers(2, 6, a)
    return S


def test_prograph_align_routes(pg):
    from prograph_amd import _native
    from prograph_amd.graph import CSRGraph, KNNGraph
    P, tok = pg
    calls = fake_aln_native.calls
    S = _score_table(np.random.default_rng(3))
    op = local_alignment(S, 3, gap_open=2)
    G = P.build_graph(k=3, distance=op, output="csr")
    assert isinstance(G, KNNGraph)
    del calls[:]
    got = P.align(G, distance=op)
    assert [c for c in calls if c[0] == "trace"] == [("trace", LOCAL, 0, 3 * N, 3, 2)] and ("operand", N, L, 21) in calls
    rows, cols = np.repeat(np.arange(N), 3), G.idx.numpy().reshape(-1)
    same_as_definition(got, LOCAL, S, 3, 2, tok, tok, rows, cols)
    assert np.array_equal(got.score.numpy(), G.dist.numpy().reshape(-1))             # the edge weights
    a, b = got.gapped(5)
    assert len(a) == len(b) == int(got.n_ops[5]) and set(a + b) <= set("-?" + P.amino_acids)
    # the same edges as a CSRGraph, as the tuple list, as a stored name, as explicit pairs
    for form in (G.as_csr(), G.to_tuples()):
        assert np.array_equal(P.align(form, distance=op).ops.numpy(), got.ops.numpy())
    P.build_graph(k=3, distance=op, store="Near")
    assert np.array_equal(P.align("Near", distance=op).ops.numpy(), got.ops.numpy())
    assert np.array_equal(P.align(rows=rows, cols=cols, distance=op).ops.numpy(), got.ops.numpy())
    # row0 is honoured
    part = CSRGraph(torch.tensor([0, 2, 3]), torch.tensor([4, 9, 1], dtype=torch.int32), torch.zeros(3), N, row0=7)
    same_as_definition(P.align(part, distance=op), LOCAL, S, 3, 2, tok, tok, [7, 7, 8], [4, 9, 1])
    # idxs: the graph was built over a selection; rows and columns are positions in it
    sub = np.arange(20, 50)
    Gs = P.build_graph(k=2, distance=op, idxs=sub, output="csr")
    gs = P.align(Gs, idxs=sub, distance=op)
    same_as_definition(gs, LOCAL, S, 3, 2, tok, tok, sub[np.repeat(np.arange(30), 2)], sub[Gs.idx.numpy().reshape(-1)])
    assert np.array_equal(gs.score.numpy(), Gs.dist.numpy().reshape(-1))
    # queries: x is the query, y the dataset row; the three operators
    Q = np.zeros((4, L + 5), dtype=np.int64)
    Q[:, :L] = tok[[3, 30, 31, 59]]
    Q[1, 4:9] = 0
    Q[2, L:L + 3] = 5
    for dist, mode, T in ((op, LOCAL, S), (semiglobal_alignment(S, 3, 2), SEMIGLOBAL, S),
                          (alignment(1 - np.eye(21, dtype=np.int64), 3, 2), GLOBAL, 1 - np.eye(21, dtype=np.int64))):
        R = P.search(Q, k=3, distance=dist, output="csr")
        del calls[:]
        got = P.align(R, queries=Q, distance=dist)
        assert [c for c in calls if c[0] == "trace"] == [("trace", mode, 0, 12, 3, 2)]
        same_as_definition(got, mode, T, 3, 2, Q, tok, np.repeat(np.arange(4), 3), R.idx.numpy().reshape(-1))
        assert np.array_equal(got.score.numpy(), R.dist.numpy().reshape(-1).astype(np.int64))
    strings = list(synth.tokens_to_strings(tok[[3, 8]]))
    R = P.search(strings, eps=1, distance=op, output="csr")
    got = P.align(R, queries=strings, distance=op)
    assert np.array_equal(got.score.numpy(), R.weights.numpy().astype(np.int64)) and len(got) == R.nnz > 0
    # splitting by workspace_bytes: 180 pairs, one wave's share at a time -> 3 launches of 64, 64, 52 pairs; same answer
    one = _native.aln_trace_wave_bytes(L, L)
    whole = P.align(G, distance=op)
    for ws, want in ((one, [(0, 64), (64, 128), (128, 180)]), (2 * one + 5, [(0, 128), (128, 180)]), (1 << 30, [(0, 180)])):
        del calls[:]
        part = P.align(G, distance=op, workspace_bytes=ws)
        assert [(c[2], c[3]) for c in calls if c[0] == "trace"] == want
        assert np.array_equal(part.ops.numpy(), whole.ops.numpy()) and np.array_equal(part.score.numpy(), whole.score.numpy())
    with pytest.raises(ValueError, match="one wave's share"):
        P.align(G, distance=op, workspace_bytes=one - 1)
    # errors
    from prograph_amd.distance import hamming, substitution
    for wrong in (hamming, levenshtein, substitution(1 - np.eye(21, dtype=np.int64)), None, "local"):
        with pytest.raises(TypeError, match="alignment, local_alignment or semiglobal_alignment"):
            P.align(G, distance=wrong)
    with pytest.raises(TypeError, match="graph must be"):
        P.align(3.5, distance=op)
    with pytest.raises(ValueError):
        P.align(distance=op)
    with pytest.raises(ValueError):
        P.align(G, rows=[1], cols=[2], distance=op)
    with pytest.raises(IndexError):
        P.align(rows=[0], cols=[N], distance=op)
    with pytest.raises(IndexError):
        _native.alignment_trace(_native.aln_operand(torch.zeros((2, 4), dtype=torch.uint8), 4),
                                _native.aln_operand(torch.zeros((2, 4), dtype=torch.uint8), 4), [0, 2], [0, 1], LOCAL,
                                torch.zeros((32, 32), dtype=torch.int8), 1, 0)
    assert len(P.align(rows=[], cols=[], distance=op)) == 0


def test_prograph_align_beyond_the_kernel(pg, monkeypatch):
    """Wider than 128 positions, or no device at all: the host expression, no launch."""
    P, tok = pg
    S = _score_table(np.random.default_rng(4))
    op = semiglobal_alignment(S, 2, gap_open=1)
    Q = np.zeros((2, 140), dtype=np.int64)
    Q[0, :L], Q[1, 100:100 + L] = tok[5], tok[6]
    Q[1, :100] = 1
    del fake_aln_native.calls[:]
    got = P.align(rows=[0, 1, 1], cols=[5, 6, 7], queries=Q, distance=op)
    assert not [c for c in fake_aln_native.calls if c[0] == "trace"]
    same_as_definition(got, SEMIGLOBAL, S, 2, 1, Q, tok, [0, 1, 1], [5, 6, 7])
    assert (int(got.x_begin[1]), int(got.x_end[1])) == (100, 100 + len(sequence(tok[6])))
    fake_trace_native.install(monkeypatch, ready=False)
    del fake_aln_native.calls[:]
    got = P.align(rows=[1, 2], cols=[2, 1], distance=op)
    assert not [c for c in fake_aln_native.calls if c[0] == "trace"]
    same_as_definition(got, SEMIGLOBAL, S, 2, 1, tok, tok, [1, 2], [2, 1])
