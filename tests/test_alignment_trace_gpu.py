"""
The traceback kernel (`pg_alignment_trace`, prograph_amd/csrc/pg_aln_trace.hip) on the GPU: every field of every pair
against `definition` of tests/trace_testdata.py, exactly, and the scores of a graph's edges against the graph's weights.
One list of 200 pairs per (mode, gap, gap_open, widths) serves every list length: the reference is computed once.
The kernel is the one-strip instance of the strip template: the narrow and odd widths, where the strip, its dwords of
direction bits and its dwords of tokens end early, run in four modes against `alignments.host_trace`.
"""
import functools

import numpy as np
import pandas as pd
import pytest
import torch

from trace_testdata import FIELDS, GLOBAL, LOCAL, SEMIGLOBAL, definition
from prograph_amd import _native, alignments, synth
from prograph_amd.distance import alignment, local_alignment, semiglobal_alignment

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

LENS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128)       # around the 8-cell dwords and the 4-token dwords
A, ROWS, PAIRS = 6, 48, 200
CLASSES = {GLOBAL: alignment, LOCAL: local_alignment, SEMIGLOBAL: semiglobal_alignment}


def table(mode):
    rng = np.random.default_rng(11 + mode)
    if mode == GLOBAL:
        T = rng.integers(1, 4, (A, A))
        T = np.triu(T, 1) + np.triu(T, 1).T
    else:
        T = rng.integers(-3, 2, (A, A))
        T = np.triu(T) + np.triu(T, 1).T
        T[np.arange(A), np.arange(A)] = rng.integers(1, 5, A)
        T[0, 1] = T[1, 0] = 2                                               # S[a][0] > 0: padding must not pair
    return T


def operand(rng, width):
    """(ROWS, width) tokens: the lengths of LENS that fit, mixed row by row (so within every wave), zeros inside."""
    lens = [l for l in LENS if l <= width]
    M = np.zeros((ROWS, width), dtype=np.uint8)
    for r in range(ROWS):
        l = lens[r % len(lens)] if r < 2 * len(lens) else int(rng.choice(lens))
        M[r, :l] = rng.integers(0, A, l)
        if l:
            M[r, l - 1] = rng.integers(1, A)
    return M[rng.permutation(ROWS)]


@functools.lru_cache(maxsize=None)
def problem(mode, gap, gap_open, xw, yw):
    """Two operands, a random pair list over their rows (200 pairs over 48 rows: rows and whole pairs repeat), and the
    definition's answer for every pair."""
    rng = np.random.default_rng(1000 * mode + 10 * gap + gap_open + xw)
    X, Y = operand(rng, xw), operand(rng, yw)
    xi, yi = rng.integers(0, ROWS, PAIRS), rng.integers(0, ROWS, PAIRS)
    xi[1], yi[1] = xi[0], yi[0]                                             # the same pair twice, the same row in two pairs
    xi[2] = xi[0]
    T = table(mode)
    want = [definition(mode, T, gap, gap_open, X[xi[p]], Y[yi[p]]) for p in range(PAIRS)]
    return X, Y, xi, yi, T, want


def device_table(mode, T):
    return _native.sub_cost(T) if mode == GLOBAL else _native.aln_local_score(T)


def check(head, ops, want, xw, yw):
    head, ops = head.cpu().numpy(), ops.cpu().numpy()
    assert head.shape == (len(want), 8) and ops.shape == (len(want), xw + yw) and ops.dtype == np.uint8
    for p, w in enumerate(want):
        assert head[p].tolist() == [w[f] for f in FIELDS] + [0], (p, head[p], w)
        assert ops[p, :w["n_ops"]].tolist() == w["ops"] and not ops[p, w["n_ops"]:].any(), (p, ops[p], w["ops"])


@pytest.mark.parametrize("pairs", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("gap_open", [0, 11])
@pytest.mark.parametrize("mode", [GLOBAL, LOCAL, SEMIGLOBAL])
@pytest.mark.parametrize("xw,yw", [(128, 128), (20, 128)])
def test_every_field_is_the_definition(xw, yw, mode, gap_open, pairs):
    X, Y, xi, yi, T, want = problem(mode, 2, gap_open, xw, yw)
    xo, yo = _native.aln_operand(torch.from_numpy(X), A), _native.aln_operand(torch.from_numpy(Y), A)
    head, ops = _native.alignment_trace(xo, yo, xi[:pairs], yi[:pairs], mode, device_table(mode, T), 2, gap_open)
    assert xo.valid() and yo.valid()
    check(head, ops, want[:pairs], xw, yw)


@functools.lru_cache(maxsize=None)
def narrow(mode, gap_open, xw, yw):
    """65 pairs (two waves, the second of one lane) over rows of every length 0..width that fits in 24 rows, the widths
    themselves and an all-zero row on either side among them; pairs 0..2 meet the empty rows.  The host's answer, once."""
    rng = np.random.default_rng(100 * xw + yw)
    def rows(w):
        M = np.zeros((24, w), dtype=np.uint8)
        for r, l in enumerate([0, w] + [int(v) for v in rng.integers(0, w + 1, 22)]):
            M[r, :l] = rng.integers(0, A, l)
            if l:
                M[r, l - 1] = rng.integers(1, A)
        return M
    X, Y = rows(xw), rows(yw)
    xi, yi = rng.integers(0, 24, 65), rng.integers(0, 24, 65)
    xi[:3], yi[:3] = (0, 0, 1), (0, 1, 0)                                   # len x = len y = 0; len x = 0; len y = 0
    T = table(mode)
    return X, Y, xi, yi, T, alignments.host_trace(mode, T, 2, gap_open, X, Y, xi, yi)


@pytest.mark.parametrize("gap_open", [0, 11])
@pytest.mark.parametrize("mode", [GLOBAL, LOCAL, SEMIGLOBAL, alignments.FIT])
@pytest.mark.parametrize("xw,yw", [(1, 1), (128, 1), (1, 128), (7, 9), (127, 121)])
def test_narrow_and_odd_widths_are_the_host_trace(xw, yw, mode, gap_open):
    """A y width that is no multiple of 8 or of 4, an x of one dword, one column, one row: the single strip against
    `host_trace`, field for field; fit through its own entry."""
    X, Y, xi, yi, T, (*fields, hops) = narrow(mode, gap_open, xw, yw)
    assert not X[0].any() and not Y[0].any()
    xo, yo = _native.aln_operand(torch.from_numpy(X), A), _native.aln_operand(torch.from_numpy(Y), A)
    head, ops = _native.alignment_trace(xo, yo, xi, yi, mode, device_table(mode, T), 2, gap_open)
    head, ops = head.cpu().numpy(), ops.cpu().numpy()
    assert head.shape == (65, 8) and ops.shape == (65, xw + yw) and ops.dtype == np.uint8
    for c, f in enumerate(FIELDS):
        assert np.array_equal(head[:, c], fields[c]), (f, head[:, c], fields[c])
    assert not head[:, 7].any() and np.array_equal(ops, hops)


@pytest.mark.parametrize("mode", [GLOBAL, LOCAL, SEMIGLOBAL])
def test_the_largest_penalties(mode):
    X, Y, xi, yi, T, want = problem(mode, 255, 255, 128, 128)
    xo, yo = _native.aln_operand(torch.from_numpy(X), A), _native.aln_operand(torch.from_numpy(Y), A)
    head, ops = _native.alignment_trace(xo, yo, xi[:65], yi[:65], mode, device_table(mode, T), 255, 255)
    check(head, ops, want[:65], 128, 128)


@pytest.mark.parametrize("mode", [GLOBAL, LOCAL, SEMIGLOBAL])
def test_a_small_workspace_changes_nothing(mode):
    """200 pairs are four waves: one wave's share of workspace makes four launches, two waves' share two."""
    X, Y, xi, yi, T, want = problem(mode, 2, 11, 128, 128)
    xo, yo = _native.aln_operand(torch.from_numpy(X), A), _native.aln_operand(torch.from_numpy(Y), A)
    one = _native.aln_trace_wave_bytes(128, 128)
    assert one == 64 * 128 * 16 * 4 and -(-PAIRS // 64) >= 3
    whole = _native.alignment_trace(xo, yo, xi, yi, mode, device_table(mode, T), 2, 11)
    check(*whole, want, 128, 128)
    for ws in (one, 2 * one + 17):
        part = _native.alignment_trace(xo, yo, xi, yi, mode, device_table(mode, T), 2, 11, workspace_bytes=ws)
        assert torch.equal(part[0], whole[0]) and torch.equal(part[1], whole[1])
    with pytest.raises(ValueError):
        _native.alignment_trace(xo, yo, xi, yi, mode, device_table(mode, T), 2, 11, workspace_bytes=one - 1)
    with pytest.raises(IndexError):
        _native.alignment_trace(xo, yo, [0, ROWS], [0, 0], mode, device_table(mode, T), 2, 11)


@pytest.mark.parametrize("mode", [GLOBAL, LOCAL, SEMIGLOBAL])
def test_operator_align_on_device_tokens(mode):
    """`op.align`: row p with row p, any integer dtype, the container's fields and helpers."""
    X, Y, xi, yi, T, want = problem(mode, 2, 11, 128, 128)
    op = CLASSES[mode](T, 2, gap_open=11)
    got = op.align(torch.from_numpy(X[xi[:70]].astype(np.int64)).cuda(), torch.from_numpy(Y[yi[:70]]).cuda())
    assert isinstance(got, alignments.Alignments) and len(got) == 70 and got.score.is_cuda and got.ops.is_cuda
    for f in FIELDS:
        assert getattr(got, f).dtype == torch.int64
        assert getattr(got, f).cpu().tolist() == [w[f] for w in want[:70]], f
    check(torch.cat([torch.stack([getattr(got, f) for f in FIELDS], 1), torch.zeros((70, 1), device="cuda", dtype=torch.int64)], 1),
          got.ops, want[:70], 128, 128)
    full = op(torch.from_numpy(X[xi[:70]]).cuda(), torch.from_numpy(Y[yi[:70]]).cuda())
    assert torch.equal(torch.diagonal(full), got.score)
    p = int(np.argmax([w["n_ops"] for w in want[:70]]))
    a, b = got.gapped(p)
    assert len(a) == len(b) == want[p]["n_ops"] and got.cigar(p) == got.host().cigar(p) != ""
    with pytest.raises(ValueError, match="outside the table"):
        op.align(torch.full((2, 8), A, dtype=torch.uint8).cuda(), torch.ones((2, 8), dtype=torch.uint8).cuda())


@pytest.fixture(scope="module")
def pg(tmp_path_factory):
    from prograph_amd import Prograph
    tok, _ = synth.clustered_varlen_tokens(150, Lmax=40, Lmin=8, seed=9, members=10)
    f = tmp_path_factory.mktemp("trace") / "trace.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P, tok


def _operators():
    rng = np.random.default_rng(5)
    S = rng.integers(-4, 2, (21, 21))
    S = np.triu(S) + np.triu(S, 1).T
    S[np.arange(21), np.arange(21)] = rng.integers(2, 6, 21)
    C = rng.integers(1, 5, (21, 21))
    C = np.triu(C, 1) + np.triu(C, 1).T
    return ((alignment(C, 2, gap_open=3), GLOBAL, C, 2, 3), (local_alignment(S, 1, gap_open=4), LOCAL, S, 1, 4),
            (semiglobal_alignment(S, 2), SEMIGLOBAL, S, 2, 0))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_edge_scores_are_the_graph_weights(pg, which):
    P, tok = pg
    op, mode, T, gap, gap_open = _operators()[which]
    G = P.build_graph(k=3, distance=op, output="csr")
    got = P.align(G, distance=op)
    assert len(got) == 450 and torch.equal(got.score, G.dist.reshape(-1).to(torch.int64))
    idx = G.idx.cpu().numpy().reshape(-1)
    for p in (0, 17, 449):
        w = definition(mode, T, gap, gap_open, tok[p // 3], tok[idx[p]])
        assert [int(getattr(got, f)[p]) for f in FIELDS] == [w[f] for f in FIELDS]
        assert got.ops[p, :w["n_ops"]].tolist() == w["ops"]
    # a search result: x is the query, y the dataset row
    Q = tok[[4, 77, 149]].copy()
    Q[1, 3:6] = 0
    R = P.search(Q, k=4, distance=op, output="csr")
    got = P.align(R, queries=Q, distance=op)
    assert len(got) == 12 and torch.equal(got.score, R.dist.reshape(-1).to(torch.int64))
    ridx = R.idx.cpu().numpy().reshape(-1)
    w = definition(mode, T, gap, gap_open, Q[1], tok[ridx[5]])
    assert [int(getattr(got, f)[5]) for f in FIELDS] == [w[f] for f in FIELDS] and got.ops[5, :w["n_ops"]].tolist() == w["ops"]
    E = P.search(Q, eps=(3 if mode == GLOBAL else 20), distance=op, output="csr")
    assert torch.equal(P.align(E, queries=Q, distance=op).score, E.weights.to(torch.int64)) and E.nnz > 0
