"""
Alignment statistics without a GPU (`ops=False`, `min_identity=`).

Held against `definition` of tests/trace_testdata.py and `canonical` of tests/fit_testdata.py: the statistics kernel's row
routine compiled for the host beside the traceback's under the sanitizers (tests/capi_stats), the C ABI's argument checks,
the `ops=False` containers on the three routes (the stand-in of tests/fake_stats_native.py for the two device ones), the
slices of the route beyond 128 positions, and the percent-identity cuts of `build_graph` / `search`, whose expected edges
are computed here from the definition.  The kernel itself: tests/test_alignment_stats_gpu.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

import fake_aln_native
import fake_stats_native
from conftest import REPO
from fake_stats_native import FIT, head_of
from trace_testdata import FIELDS, GLOBAL, LOCAL, SEMIGLOBAL
from prograph_amd import alignments, synth
from prograph_amd.alignments import Alignments
from prograph_amd.distance import alignment, fit_alignment, hamming, levenshtein, local_alignment, semiglobal_alignment
from prograph_amd.graph import CSRGraph, KNNGraph

N, L = 60, 24


def _launches(kind):
    return [c for c in fake_aln_native.calls if c[0] == kind]


def _score_table(seed, a=21):
    rng = np.random.default_rng(seed)
    S = rng.integers(-4, 2, (a, a))
    S = np.triu(S) + np.triu(S, 1).T
    S[np.arange(a), np.arange(a)] = rng.integers(2, 6, a)
    return S


def _cost_table(seed, a=21):
    rng = np.random.default_rng(seed)
    C = rng.integers(1, 4, (a, a))
    return np.triu(C, 1) + np.triu(C, 1).T


def _prograph(tmp_path, tok):
    from prograph_amd import Prograph
    f = tmp_path / f"stats_{tok.shape[1]}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P


def fields_are(got, mode, T, gap, gap_open, X, Y, xi, yi):
    """The seven fields of a container against the definitions, pair by pair."""
    assert len(got) == len(xi)
    for f in FIELDS:
        assert getattr(got, f).dtype == torch.int64 and getattr(got, f).shape == (len(xi),), f
    have = np.stack([getattr(got, f).cpu().numpy() for f in FIELDS], 1)
    for p in range(len(xi)):
        assert have[p].tolist() == head_of(mode, T, gap, gap_open, X[xi[p]], Y[yi[p]]), (p, have[p])


def test_the_kernel_routines_on_the_host():
    """tests/capi_stats/stats_check.cpp: pg_aln_stats.h's row routine against pg_aln_trace.h's row routine and walk, both
    compiled for the host with -fsanitize=address,undefined: every pair of sequences over 2 and 3 symbols up to length 6
    under tables where ties are the rule, then random pairs up to 128 positions with the extreme tables."""
    capi = os.path.join(REPO, "tests", "capi_stats")
    subprocess.check_call(["make", "-s", "-C", capi])
    out = subprocess.run([os.path.join(capi, "_build", "stats_check")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "stats routines OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_c_abi_argument_errors_without_gpu():
    from prograph_amd import _native
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                              # never dereferenced: every check is on the host

    def call(mode=0, x=p, n=4, xnpad=256, xl=20, y=p, m=4, ynpad=256, yl=9, xi=p, yi=p, npairs=3, table=p, gap=1, gap_open=0,
             head=p):
        return lib.pg_alignment_stats(mode, x, n, xnpad, xl, y, m, ynpad, yl, xi, yi, npairs, table, gap, gap_open, head, None)
    for bad in (dict(mode=4), dict(mode=-1), dict(gap=0), dict(gap=256), dict(gap_open=-1), dict(gap_open=256), dict(x=None),
                dict(y=None), dict(xi=None), dict(yi=None), dict(table=None), dict(head=None), dict(npairs=0), dict(n=0),
                dict(m=0), dict(xl=0), dict(yl=0), dict(xnpad=3), dict(ynpad=3)):
        assert call(**bad) == -1, bad
        assert b"pg_alignment_stats" in lib.pg_last_error()
    for mode in (0, 1, 2, 3):
        assert call(mode=mode, xl=129) == -2 and call(mode=mode, yl=129) == -2
    assert lib.pg_version() == 3


# ---------------------------------------------------------------- containers and routes
@pytest.fixture()
def pg(tmp_path, monkeypatch):
    fake_stats_native.install(monkeypatch)
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=10, seed=5, members=6)
    P = _prograph(tmp_path, tok)
    del fake_aln_native.calls[:]
    return P, tok


def _operators():
    S, C = _score_table(3), _cost_table(4)
    return ((alignment(C, 2, gap_open=1), GLOBAL, C, 2, 1), (local_alignment(S, 3, gap_open=2), LOCAL, S, 3, 2),
            (semiglobal_alignment(S, 2), SEMIGLOBAL, S, 2, 0), (fit_alignment(S, 2, gap_open=1), FIT, S, 2, 1))


def test_containers_without_ops(pg):
    """`ops=False` on the three routes: the same seven fields, `ops` None, `cigar` / `gapped` raise."""
    P, tok = pg
    rng = np.random.default_rng(7)
    xi, yi = rng.integers(0, N, 40), rng.integers(0, N, 40)
    X = torch.from_numpy(tok.astype(np.uint8))
    for op, mode, T, gap, gap_open in _operators():
        # the 128-position kernel's stand-in: one launch, no trace launch, no workspace
        del fake_aln_native.calls[:]
        got = alignments.trace(op, X, X, xi, yi, native=True, ops=False)
        assert _launches("stats") == [("stats", mode, 40, gap, gap_open)] and not _launches("trace")
        assert isinstance(got, Alignments) and got.ops is None and len(got) == 40 and "no ops" in repr(got)
        fields_are(got, mode, T, gap, gap_open, tok, tok, xi, yi)
        # the host route on CPU tensors
        del fake_aln_native.calls[:]
        host = alignments.trace(op, X[:, :L], X, xi, yi, ops=False)
        assert not _launches("stats") and not _launches("trace") and host.ops is None
        for f in FIELDS:
            assert torch.equal(getattr(host, f), getattr(got, f)), f
        full = alignments.trace(op, X, X, xi, yi)                           # the default keeps the columns
        assert full.ops is not None and full.ops.shape == (40, 2 * L)
        for f in FIELDS:
            assert torch.equal(getattr(full, f), getattr(got, f)), f
        ident = got.identity()
        assert ident.dtype == torch.float64 and torch.equal(ident, full.identity())
        h = got.host()
        assert h.ops is None and torch.equal(h.n_ops, got.n_ops)
        for call in (lambda: got.cigar(0), lambda: got.gapped(0), lambda: h.cigar(3)):
            with pytest.raises(ValueError, match="built without ops"):
                call()
        # op.align(X, Y, ops=False): row p with row p
        pairs = op.align(torch.from_numpy(tok[xi[:6]]), torch.from_numpy(tok[yi[:6]]), ops=False)
        assert pairs.ops is None
        fields_are(pairs, mode, T, gap, gap_open, tok[xi[:6]], tok[yi[:6]], np.arange(6), np.arange(6))
    empty = alignments.trace(op, X, X, [], [], native=True, ops=False)
    assert len(empty) == 0 and empty.ops is None
    # the index check is alignment_trace's
    from prograph_amd import _native
    xo = _native.aln_operand(torch.zeros((2, 4), dtype=torch.uint8), 4)
    table = torch.zeros((32, 32), dtype=torch.int8)
    for bad_x, bad_y in (([0, 2], [0, 1]), ([0, 1], [-1, 1])):
        with pytest.raises(IndexError, match="alignment_stats"):
            _native.alignment_stats(xo, xo, bad_x, bad_y, LOCAL, table, 1, 0)
    with pytest.raises(ValueError, match="non-empty"):
        _native.alignment_stats(xo, xo, [], [], LOCAL, table, 1, 0)
    with pytest.raises(ValueError, match="outside the table"):
        alignments.trace(local_alignment(_score_table(3)[:4, :4], 1), torch.full((1, 8), 4, dtype=torch.uint8),
                         torch.ones((1, 8), dtype=torch.uint8), native=True, ops=False)


def test_prograph_align_without_ops(pg):
    P, tok = pg
    for op, mode, T, gap, gap_open in _operators()[:3]:
        G = P.build_graph(k=3, distance=op, output="csr")
        del fake_aln_native.calls[:]
        got = P.align(G, distance=op, ops=False)
        assert _launches("stats") == [("stats", mode, 3 * N, gap, gap_open)] and not _launches("trace") and got.ops is None
        full = P.align(G, distance=op)
        for f in FIELDS:
            assert torch.equal(getattr(full, f), getattr(got, f)), f
    # fit: the tracer's x is the edge's column
    op, mode, T, gap, gap_open = _operators()[3]
    got = P.align(rows=[3, 4, 5], cols=[7, 4, 1], distance=op, ops=False)
    fields_are(got, FIT, T, gap, gap_open, tok, tok, [7, 4, 1], [3, 4, 5])
    with pytest.raises(TypeError):
        P.align(rows=[0], cols=[1], distance=hamming, ops=False)


def test_the_long_route_runs_in_slices(tmp_path, monkeypatch):
    """129..2048 positions with `ops=False`: the strip kernel over slices of the pair list, one ops buffer of at most
    256 MiB, one workspace, only the heads kept."""
    from prograph_amd import _native
    fake_stats_native.install(monkeypatch)
    rng = np.random.default_rng(11)
    wide = 130
    tok = np.zeros((20, wide), dtype=np.int64)
    for r in range(20):
        l = wide if r == 0 else int(rng.integers(6, 20))
        tok[r, :l] = rng.integers(1, 21, l)
    S = _score_table(5)
    op = local_alignment(S, 3, gap_open=2)
    X = torch.from_numpy(tok.astype(np.uint8))
    xi, yi = rng.integers(0, 20, 150), rng.integers(0, 20, 150)
    xo = _native.aln_long_operand(X, 21)
    one = _native.aln_trace_long_wave_bytes(wide, wide)
    # slices of 64 pairs' ops: launches (0, 64), (0, 64), (0, 22) of three slices, each into the ONE buffer of 64 rows
    del fake_aln_native.calls[:]
    head = _native.alignment_trace_long_heads(xo, xo, xi, yi, LOCAL, torch.from_numpy(S.astype(np.int8)), 3, 2,
                                              ops_bytes=64 * 2 * wide + 5)
    assert [(c[2], c[3], c[6]) for c in _launches("trace_long")] == [(0, 64, one), (0, 64, one), (0, 22, one)]
    assert [c[2] for c in _launches("ops_buffer")] == [64, 64, 22] and all(c[1] <= 64 * 2 * wide for c in _launches("ops_buffer"))
    assert head.shape == (150, 8) and head.dtype == torch.int32
    for p in range(150):
        assert head[p].tolist() == head_of(LOCAL, S, 3, 2, tok[xi[p]], tok[yi[p]]) + [0], p
    # a buffer smaller than one pair's ops: one pair at a time
    del fake_aln_native.calls[:]
    few = _native.alignment_trace_long_heads(xo, xo, xi[:3], yi[:3], LOCAL, torch.from_numpy(S.astype(np.int8)), 3, 2, ops_bytes=1)
    assert [(c[2], c[3]) for c in _launches("trace_long")] == [(0, 1)] * 3 and torch.equal(few, head[:3])
    # through trace(): the default buffer takes the whole list in one slice, which holds 150 rows, not more
    del fake_aln_native.calls[:]
    got = alignments.trace(op, X, X, xi, yi, native_long=True, ops=False)
    assert got.ops is None and [(c[2], c[3]) for c in _launches("trace_long")] == [(0, 150)] and not _launches("stats")
    assert _launches("ops_buffer") == [("ops_buffer", 150 * 2 * wide, 150)]
    assert torch.equal(torch.stack([getattr(got, f) for f in FIELDS], 1), head[:, :7].to(torch.int64))
    with pytest.raises(IndexError, match="alignment_trace_long_heads"):
        _native.alignment_trace_long_heads(xo, xo, [0, 20], [0, 0], LOCAL, torch.from_numpy(S.astype(np.int8)), 3, 2)


def test_the_default_ops_buffer_stays_within_256_mib(monkeypatch):
    """The default slice at the widest operands: a list longer than 256 MiB of ops runs in two slices through one buffer of
    at most 256 MiB.  The launch here only records: nothing is computed for 66 000 pairs."""
    from prograph_amd import _native
    fake_stats_native.install(monkeypatch)
    seen = []

    def record(xo, yo, xi, yi, p0, p1, mode, table, gap, gap_open, head, ops, ws):
        assert ops.numel() <= 256 << 20 and ops.shape[1] == xo.l + yo.l and p1 <= xi.numel() == head.shape[0] <= ops.shape[0]
        seen.append((xi.numel(), p0, p1, ops.numel()))
        head[p0:p1] = 0
    monkeypatch.setattr(_native, "_trace_long_launch", record)
    X = torch.ones((2, 2048), dtype=torch.uint8)
    xo = _native.aln_long_operand(X, 4)
    per = (256 << 20) // 4096                                               # 65 536 pairs of 4096 ops bytes
    p = per + 464
    head = _native.alignment_trace_long_heads(xo, xo, torch.zeros(p, dtype=torch.int32), torch.ones(p, dtype=torch.int32), LOCAL,
                                              torch.zeros((32, 32), dtype=torch.int8), 1, 0)
    assert head.shape == (p, 8) and not head.any()
    assert sorted({s[0] for s in seen}) == [464, per] and max(s[3] for s in seen) == 256 << 20
    first = [s for s in seen if s[0] == per]
    assert first[0][1] == 0 and first[-1][2] == per and all(a[2] == b[1] for a, b in zip(first, first[1:]))
    assert [s[1:3] for s in seen if s[0] == 464] == [(0, 464)]


# ---------------------------------------------------------------- the percent-identity cut
def _edges(g):
    """(rows, cols, weights) of a CSRGraph / KNNGraph / tuple list, -1 slots dropped."""
    if isinstance(g, KNNGraph):
        g = g.as_csr()
    if isinstance(g, CSRGraph):
        ip, c, w = g.indptr.numpy(), g.indices.numpy().astype(np.int64), g.weights.numpy()
        r = np.repeat(np.arange(len(ip) - 1), np.diff(ip))
        return r[c >= 0], c[c >= 0], w[c >= 0]
    counts = [len(e[0]) for e in g]
    cat = lambda k: np.concatenate([np.asarray(e[k]) for e in g]) if sum(counts) else np.zeros(0)
    return np.repeat(np.arange(len(g)), counts), cat(0).astype(np.int64), cat(1)


def _stats(mode, T, gap, gap_open, X, Y, r, c):
    """(n_ops, identities) of the edges from the definitions; fit: the column has the free ends."""
    h = np.array([head_of(mode, T, gap, gap_open, *((Y[b], X[a]) if mode == FIT else (X[a], Y[b]))) for a, b in zip(r, c)]).reshape(-1, 7)
    return h[:, 5], h[:, 6]


def _expect(r, c, w, n_ops, ident, t, min_columns):
    keep = n_ops >= min_columns
    if t is not None:
        keep &= ident.astype(np.float64) / np.maximum(n_ops, 1).astype(np.float64) >= t
    return r[keep], c[keep], w[keep]


def _same_edges(g, want, nrows):
    r, c, w = _edges(g)
    assert np.array_equal(r, want[0]) and np.array_equal(c, want[1]) and np.array_equal(w, want[2])
    if isinstance(g, CSRGraph):
        assert g.nrows == nrows and np.array_equal(np.diff(g.indptr.numpy()), np.bincount(want[0], minlength=nrows))
        assert g.indptr.dtype == torch.int64 and int(g.indptr[0]) == 0 and int(g.indptr[-1]) == g.nnz


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_build_graph_min_identity(pg, which):
    P, tok = pg
    op, mode, T, gap, gap_open = _operators()[which]
    for kw in (dict(k=3), dict(eps=(14 if mode == GLOBAL else 20))):
        G = P.build_graph(distance=op, output="csr", **kw)
        r, c, w = _edges(G)
        n_ops, ident = _stats(mode, T, gap, gap_open, tok, tok, r, c)
        t = float(np.median(ident / np.maximum(n_ops, 1)))
        want = _expect(r, c, w, n_ops, ident, t, 0)
        assert 0 < len(want[0]) < len(r)                                    # at least one edge kept, at least one dropped
        del fake_aln_native.calls[:]
        F = P.build_graph(distance=op, output="csr", min_identity=t, **kw)
        assert isinstance(F, CSRGraph) and F.weights.dtype == (G.dist if isinstance(G, KNNGraph) else G.weights).dtype
        assert [c_[2] for c_ in _launches("stats")] == [len(r)] and not _launches("trace")
        _same_edges(F, want, N)
        tuples = P.build_graph(distance=op, min_identity=t, **kw)
        assert isinstance(tuples, list) and len(tuples) == N
        tr, tc, tw = _edges(tuples)
        assert np.array_equal(tr, want[0]) and np.array_equal(tc, want[1]) and np.array_equal(tw, want[2].astype(tw.dtype))
        # the defaults change nothing
        same = P.build_graph(distance=op, output="csr", min_identity=None, min_columns=0, **kw)
        assert type(same) is type(G) and all(np.array_equal(a, b) for a, b in zip(_edges(same), (r, c, w)))


def test_build_graph_min_columns_idxs_store_and_errors(pg):
    P, tok = pg
    op, mode, T, gap, gap_open = _operators()[1]
    G = P.build_graph(k=3, distance=op, output="csr")
    r, c, w = _edges(G)
    n_ops, ident = _stats(mode, T, gap, gap_open, tok, tok, r, c)
    cut = int(np.median(n_ops))
    want = _expect(r, c, w, n_ops, ident, None, cut + 1)
    assert 0 < len(want[0]) < len(r)
    _same_edges(P.build_graph(k=3, distance=op, output="csr", min_columns=cut + 1), want, N)
    both = _expect(r, c, w, n_ops, ident, 0.5, cut + 1)
    _same_edges(P.build_graph(k=3, distance=op, output="csr", min_columns=cut + 1, min_identity=0.5), both, N)
    # idxs: rows and columns are positions in the selection
    sub = np.arange(20, 50)
    Gs = P.build_graph(k=2, distance=op, idxs=sub, output="csr")
    rs, cs, ws = _edges(Gs)
    ns, ids = _stats(mode, T, gap, gap_open, tok, tok, sub[rs], sub[cs])
    ts = float(np.median(ids / np.maximum(ns, 1)))
    want_s = _expect(rs, cs, ws, ns, ids, ts, 0)
    assert 0 < len(want_s[0]) < len(rs)
    Fs = P.build_graph(k=2, distance=op, idxs=sub, output="csr", min_identity=ts)
    _same_edges(Fs, want_s, 30)
    assert Fs.ncols == 30
    mask = np.zeros(N, dtype=bool)
    mask[20:50] = True
    _same_edges(P.build_graph(k=2, distance=op, idxs=mask, output="csr", min_identity=ts), want_s, 30)
    # store= stores the filtered graph
    t = float(np.median(ident / np.maximum(n_ops, 1)))
    want_t = _expect(r, c, w, n_ops, ident, t, 0)
    P.build_graph(k=3, distance=op, store="Alike", min_identity=t)
    sr, sc, sw = _edges(list(P.graph["Alike"]))
    assert np.array_equal(sr, want_t[0]) and np.array_equal(sc, want_t[1])
    _same_edges(P.csr_graphs["Alike"], want_t, N)
    assert len(P.align("Alike", distance=op, ops=False)) == len(want_t[0])
    # errors
    for wrong in (hamming, levenshtein):
        with pytest.raises(TypeError):
            P.build_graph(k=3, distance=wrong, min_identity=0.5)
        with pytest.raises(TypeError):
            P.search(tok[:2], k=3, distance=wrong, min_columns=2)
    for bad in (dict(min_identity=-0.1), dict(min_identity=1.5), dict(min_columns=-1), dict(min_identity=0.5, min_columns=-2)):
        with pytest.raises(ValueError):
            P.build_graph(k=3, distance=op, **bad)
        with pytest.raises(ValueError):
            P.search(tok[:2], k=3, distance=op, **bad)


def test_the_empty_alignment_is_kept_only_at_zero(pg):
    """A local score of 0 is the empty alignment: identity 0, kept at min_identity = 0, dropped above it."""
    P, tok = pg
    S = _score_table(3)
    op = local_alignment(S, 3, gap_open=2)
    Q = np.zeros((2, L), dtype=np.int64)
    Q[0, :L] = tok[3]
    G = P.search(Q, k=2, distance=op, output="csr")                         # query 1 is empty: every score is 0
    r, c, w = _edges(G)
    n_ops, ident = _stats(LOCAL, S, 3, 2, Q, tok, r, c)
    assert (n_ops[r == 1] == 0).all() and (n_ops[r == 0] > 0).all() and len(r) == 4
    zero = P.search(Q, k=2, distance=op, output="csr", min_identity=0.0)
    assert isinstance(zero, CSRGraph) and np.array_equal(_edges(zero)[1], c) and zero.indptr.tolist() == [0, 2, 4]
    tiny = P.search(Q, k=2, distance=op, output="csr", min_identity=1e-9)
    assert tiny.indptr.tolist() == [0, 2, 2] and np.array_equal(_edges(tiny)[1], c[r == 0])
    cols = P.search(Q, k=2, distance=op, output="csr", min_columns=1)
    assert cols.indptr.tolist() == [0, 2, 2]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_search_min_identity(pg, which):
    P, tok = pg
    op, mode, T, gap, gap_open = _operators()[which]
    Q = np.zeros((5, L + 5), dtype=np.int64)
    Q[:, :L] = tok[[3, 30, 31, 59, 12]]
    Q[1, 4:9] = 0
    Q[2, L:L + 3] = 5
    for kw in (dict(k=4), dict(eps=(14 if mode == GLOBAL else 20))):
        R = P.search(Q, distance=op, output="csr", **kw)
        r, c, w = _edges(R)
        n_ops, ident = _stats(mode, T, gap, gap_open, Q, tok, r, c)
        t = float(np.median(ident / np.maximum(n_ops, 1)))
        want = _expect(r, c, w, n_ops, ident, t, 0)
        assert 0 < len(want[0]) < len(r)
        F = P.search(Q, distance=op, output="csr", min_identity=t, **kw)
        assert isinstance(F, CSRGraph) and F.ncols == N
        _same_edges(F, want, 5)
        tr, tc, tw = _edges(P.search(Q, distance=op, min_identity=t, **kw))
        assert np.array_equal(tr, want[0]) and np.array_equal(tc, want[1])
        assert len(P.align(F, queries=Q, distance=op, ops=False)) == len(want[0])
    strings = list(synth.tokens_to_strings(tok[[3, 8]]))
    R = P.search(strings, k=3, distance=op, output="csr")
    F = P.search(strings, k=3, distance=op, output="csr", min_identity=None, min_columns=0)
    assert type(F) is type(R) and torch.equal(F.idx, R.idx)                                              # nothing asked: nothing changes
    F = P.search(strings, k=3, distance=op, output="csr", min_identity=0.0, min_columns=1)
    assert isinstance(F, CSRGraph) and F.nrows == 2


def test_the_generic_loop_is_cut_too(pg):
    """A `comp` outside `operator`'s five takes `build_graph`'s generic loop, which hands back tuples: the cut applies."""
    P, tok = pg
    op, mode, T, gap, gap_open = _operators()[0]
    le = lambda a, b: a <= b                                                # noqa: E731
    r, c, w = _edges(P.build_graph(eps=14, distance=op, comp=le))
    n_ops, ident = _stats(mode, T, gap, gap_open, tok, tok, r, c)
    t = float(np.median(ident / np.maximum(n_ops, 1)))
    want = _expect(r, c, w, n_ops, ident, t, 0)
    assert 0 < len(want[0]) < len(r)
    _same_edges(P.build_graph(eps=14, distance=op, comp=le, min_identity=t, output="csr"), want, N)
