"""
Alignment tracebacks beyond 128 positions (`pg_alignment_trace_long`) without a GPU: the strip routine,
the order-free end-cell rule and the long walk of prograph_amd/csrc/pg_aln_trace.h compiled for the host under the address
and undefined-behaviour sanitizers (tests/capi_trace_long), the C ABI's argument checks, and the long route of
`alignments.trace` / `Prograph.align` on the stand-in of tests/fake_trace_long_native.py, against `definition` of
tests/trace_testdata.py.  The kernel itself: tests/test_alignment_trace_long_gpu.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

import fake_aln_native
import fake_trace_long_native
from conftest import REPO
from fake_long_native import FakeLongOperand
from trace_testdata import FIELDS, LOCAL, SEMIGLOBAL, definition
from prograph_amd import alignments, synth
from prograph_amd.distance import local_alignment, semiglobal_alignment

N, WIDE, NARROW = 30, 140, 24


def same_as_definition(got, mode, T, gap, gap_open, X, Y, xi, yi):
    got = got.host()
    for p in range(len(got)):
        want = definition(mode, T, gap, gap_open, X[xi[p]], Y[yi[p]])
        assert {f: int(getattr(got, f)[p]) for f in FIELDS} == {f: want[f] for f in FIELDS}, p
        row = got.ops[p].tolist()
        assert row[:want["n_ops"]] == want["ops"] and not any(row[want["n_ops"]:]), p


def test_the_strip_routines_on_the_host():
    """tests/capi_trace_long/trace_long_check.cpp: the strip sweep with its boundary column and the long walk, compiled for
    the host with -fsanitize=address,undefined, against a plain full-table DP on a few thousand random pairs of lengths
    0..300, and the hand-made cross-strip tie."""
    capi = os.path.join(REPO, "tests", "capi_trace_long")
    subprocess.check_call(["make", "-s", "-C", capi])
    out = subprocess.run([os.path.join(capi, "_build", "trace_long_check")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "long trace routines OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_c_abi_argument_errors_without_gpu():
    from prograph_amd import _native
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                              # never dereferenced: every check is on the host
    one = ctypes.c_int64(0)
    for xl, yl, want in ((2048, 2048, (128 << 20) + (1 << 20)), (400, 400, 64 * 400 * 50 * 4 + 64 * 400 * 8),
                         (130, 9, 64 * 130 * 2 * 4 + 64 * 130 * 8)):
        assert lib.pg_alignment_trace_long_workspace(xl, yl, ctypes.byref(one)) == 0 and one.value == want
        assert _native.aln_trace_long_wave_bytes(xl, yl) == want
    assert lib.pg_alignment_trace_long_workspace(2049, 8, ctypes.byref(one)) == -2
    assert lib.pg_alignment_trace_long_workspace(8, 2049, ctypes.byref(one)) == -2
    assert lib.pg_alignment_trace_long_workspace(0, 8, ctypes.byref(one)) == -1
    assert lib.pg_alignment_trace_long_workspace(8, 8, None) == -1
    share = 64 * 130 * 2 * 4 + 64 * 130 * 8

    def call(mode=0, x=p, n=4, xnpad=256, xl=130, y=p, m=4, ynpad=256, yl=9, xi=p, yi=p, npairs=3, table=p, gap=1, gap_open=0,
             head=p, ops=p, ldo=139, ws=p, ws_bytes=share):
        return lib.pg_alignment_trace_long(mode, x, n, xnpad, xl, y, m, ynpad, yl, xi, yi, npairs, table, gap, gap_open, head,
                                           ops, ldo, ws, ws_bytes, None)
    for bad in (dict(mode=3), dict(mode=-1), dict(gap=0), dict(gap=256), dict(gap_open=-1), dict(gap_open=256), dict(x=None),
                dict(y=None), dict(xi=None), dict(yi=None), dict(table=None), dict(head=None), dict(ops=None), dict(ws=None),
                dict(ldo=138), dict(ws_bytes=share - 1), dict(npairs=0), dict(n=0), dict(xnpad=3), dict(ynpad=3)):
        assert call(**bad) == -1, bad
        assert b"pg_alignment_trace_long" in lib.pg_last_error()
    assert call(xl=2049, ldo=5000) == -2 and call(yl=2049, ldo=5000) == -2
    assert lib.pg_version() == 3 and _native.ABI_VERSION == 3
    assert {"pg_alignment_trace_long", "pg_alignment_trace_long_workspace"} <= set(_native.SYMBOLS)


# ---------------------------------------------------------------- route logic through the stand-in
def _tokens(width, seed):
    """(N, width) tokens 1..20: short rows (the reference stays quick) in a wide operand, row 0 over its whole width."""
    rng = np.random.default_rng(seed)
    tok = np.zeros((N, width), dtype=np.int64)
    for r in range(N):
        l = width if r == 0 else int(rng.integers(6, 20))
        tok[r, :l] = rng.integers(1, 21, l)
    return tok


def _prograph(tmp_path, tok):
    from prograph_amd import Prograph
    f = tmp_path / f"trace_long_{tok.shape[1]}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P


def _score_table(seed, a=21):
    rng = np.random.default_rng(seed)
    S = rng.integers(-4, 2, (a, a))
    S = np.triu(S) + np.triu(S, 1).T
    S[np.arange(a), np.arange(a)] = rng.integers(2, 6, a)
    return S


def _launches(kind):
    return [c for c in fake_aln_native.calls if c[0] == kind]


def test_a_wide_dataset_goes_long(tmp_path, monkeypatch):
    from prograph_amd import _native
    fake_trace_long_native.install(monkeypatch)
    tok = _tokens(WIDE, 1)
    P, S = _prograph(tmp_path, tok), _score_table(2)
    op = local_alignment(S, 3, gap_open=2)
    one = _native.aln_trace_long_wave_bytes(WIDE, WIDE)
    G = P.build_graph(k=2, distance=op, output="csr")
    del fake_aln_native.calls[:]
    got = P.align(G, distance=op)
    # one long launch over every edge; the default workspace is what the list needs: one wave's share for 60 pairs
    assert _launches("trace_long") == [("trace_long", LOCAL, 0, 2 * N, 3, 2, one)] and not _launches("trace")
    assert ("long_operand", N, WIDE, 21) in fake_aln_native.calls
    rows, cols = np.repeat(np.arange(N), 2), G.idx.numpy().reshape(-1)
    same_as_definition(got, LOCAL, S, 3, 2, tok, tok, rows, cols)
    assert np.array_equal(got.score.numpy(), G.dist.numpy().reshape(-1)) and got.ops.shape == (2 * N, 2 * WIDE)
    # the split by workspace_bytes: 130 pairs, one wave's share at a time -> 64, 64, 2; the answers do not move
    rng = np.random.default_rng(3)
    r, c = rng.integers(0, N, 130), rng.integers(0, N, 130)
    del fake_aln_native.calls[:]
    whole = P.align(rows=r, cols=c, distance=op)
    assert [(k[2], k[3], k[6]) for k in _launches("trace_long")] == [(0, 130, 3 * one)]
    same_as_definition(whole, LOCAL, S, 3, 2, tok, tok, r, c)
    for ws, want in ((one, [(0, 64), (64, 128), (128, 130)]), (2 * one + 17, [(0, 128), (128, 130)]), (1 << 30, [(0, 130)])):
        del fake_aln_native.calls[:]
        part = P.align(rows=r, cols=c, distance=op, workspace_bytes=ws)
        assert [(k[2], k[3]) for k in _launches("trace_long")] == want
        assert torch.equal(part.ops, whole.ops) and torch.equal(part.score, whole.score)
    with pytest.raises(ValueError, match="one wave's share"):
        P.align(rows=r, cols=c, distance=op, workspace_bytes=one - 1)
    with pytest.raises(IndexError):
        P.align(rows=[0], cols=[N], distance=op)
    table = torch.zeros((32, 32), dtype=torch.int8)
    xo = _native.aln_long_operand(torch.zeros((2, 130), dtype=torch.uint8), 4)
    assert isinstance(xo, FakeLongOperand)
    for xi, yi in (([0, 2], [0, 1]), ([0, 1], [-1, 1])):
        with pytest.raises(IndexError, match="alignment_trace_long"):
            _native.alignment_trace_long(xo, xo, xi, yi, LOCAL, table, 1, 0)
    with pytest.raises(ValueError, match="non-empty"):
        _native.alignment_trace_long(xo, xo, [], [], LOCAL, table, 1, 0)
    # a token outside the table raises as on the short route
    with pytest.raises(ValueError, match="outside the table"):
        alignments.trace(local_alignment(S[:4, :4], 1), torch.full((1, 130), 4, dtype=torch.uint8),
                         torch.ones((1, 130), dtype=torch.uint8), native_long=True)
    # without the long kernel: no launch, the host expression's answer
    fake_trace_long_native.install(monkeypatch, long_ready=False)
    del fake_aln_native.calls[:]
    got = P.align(rows=r[:5], cols=c[:5], distance=op)
    assert not _launches("trace_long") and not _launches("trace")
    same_as_definition(got, LOCAL, S, 3, 2, tok, tok, r, c)


def test_wide_queries_go_long_and_narrow_ones_do_not(tmp_path, monkeypatch):
    from prograph_amd import _native
    fake_trace_long_native.install(monkeypatch)
    tok = _tokens(NARROW, 4)
    P, S = _prograph(tmp_path, tok), _score_table(5)
    op = semiglobal_alignment(S, 2, gap_open=1)
    Q = np.zeros((2, WIDE), dtype=np.int64)
    Q[0, :NARROW], Q[1, 100:100 + NARROW] = tok[5], tok[0]
    Q[1, :100] = 1
    del fake_aln_native.calls[:]
    got = P.align(rows=[0, 1, 1], cols=[5, 0, 7], queries=Q, distance=op)
    one = _native.aln_trace_long_wave_bytes(WIDE, NARROW)
    assert _launches("trace_long") == [("trace_long", SEMIGLOBAL, 0, 3, 2, 1, one)] and not _launches("trace")
    same_as_definition(got, SEMIGLOBAL, S, 2, 1, Q, tok, [0, 1, 1], [5, 0, 7])
    assert (int(got.x_begin[1]), int(got.x_end[1])) == (100, 100 + NARROW) and got.ops.shape == (3, WIDE + NARROW)
    # at most 128 positions on both sides: the short kernel's launch, with its own default workspace
    del fake_aln_native.calls[:]
    got = P.align(rows=[1, 0], cols=[2, 1], queries=Q[:, 100:], distance=op)
    assert _launches("trace") == [("trace", SEMIGLOBAL, 0, 2, 2, 1)] and not _launches("trace_long")
    same_as_definition(got, SEMIGLOBAL, S, 2, 1, Q[:, 100:], tok, [1, 0], [2, 1])
    # `trace` itself: CPU tensors take the host expression unless told otherwise, and `native=` still means the short kernel
    Xq, Xt = torch.from_numpy(Q.astype(np.uint8)), torch.from_numpy(tok.astype(np.uint8))
    del fake_aln_native.calls[:]
    host = alignments.trace(op, Xq, Xt, [0, 1], [5, 0])
    assert not _launches("trace_long") and not _launches("trace")
    long = alignments.trace(op, Xq, Xt, [0, 1], [5, 0], native_long=True)
    assert [(k[2], k[3]) for k in _launches("trace_long")] == [(0, 2)] and not _launches("trace")
    short = alignments.trace(op, Xq[:, 100:], Xt, [0, 1], [5, 0], native=True)
    assert [(k[2], k[3]) for k in _launches("trace")] == [(0, 2)] and len(_launches("trace_long")) == 1
    for f in FIELDS + ("ops",):
        assert torch.equal(getattr(host, f), getattr(long, f)), f
    same_as_definition(short, SEMIGLOBAL, S, 2, 1, Q[:, 100:], tok, [0, 1], [5, 0])
