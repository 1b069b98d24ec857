"""
The per-pair alignment kernels on the GPU at every length and width: `pg_alignment_trace`, `pg_alignment_trace_long`, their
fit entries (prograph_amd/csrc/pg_aln_trace.hip) and `pg_alignment_stats` (pg_aln_stats.hip, its three instances).  Every
expected value is `oracle.c_oracle.align_trace` (orc_align_trace: whole int64 tables, a scan for the end cell, a walk that
compares table entries), which tests/test_alignment_trace_lengths_cpu.py pins to the Python definitions; every comparison
is an exact equality of integers.  The inputs are tests/trace_lengths_testdata.py's, whose coverage the CPU file asserts.

  A  every length 0..128 on either operand side: YS x XS (8 256 pairs) and YS x XN, both operand orders, head and ops
  B  every operand width 1..128, with guard rows round head and ops and guard bytes behind the workspace
  C  the count words at 128 in every field, and a row of ops filled to len x + len y
  D  every strip count 1..16 and every tail of the long tracer, lanes of one wave 1 to 16 strips apart
  E  the cross-strip tie at every seam
  F  a grid smaller than the list: the kernel strides and every share of workspace is used again
"""
import numpy as np
import pytest
import torch

import trace_lengths_testdata as D
from trace_testdata import FIELDS, GLOBAL, LOCAL, SEMIGLOBAL
from oracle import c_oracle
from prograph_amd import _native

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

FIT = D.FIT
GUARD, HEAD_SENTINEL, OPS_SENTINEL, WS_SENTINEL, WS_GUARD = 4, 0x5A5A5A5A, 0xEE, 0xA5, 256


def device_table(mode, T):
    return _native.sub_cost(T) if mode == GLOBAL else _native.aln_local_score(T)


def short(M):
    return _native.aln_operand(torch.from_numpy(np.array(M)), D.A)                  # a copy: the sets are read-only


def long(M):
    return _native.aln_long_operand(torch.from_numpy(np.array(M)), D.A)


def same(head, ops, want):
    """head and ops (device tensors or arrays) are the oracle's (head, ops), row for row."""
    wh, wo = want
    head = head.cpu().numpy() if isinstance(head, torch.Tensor) else head
    assert head.shape == wh.shape and head.dtype == np.int32
    wrong = (head != wh).any(1)
    if ops is not None:
        ops = ops.cpu().numpy() if isinstance(ops, torch.Tensor) else ops
        assert ops.shape == wo.shape and ops.dtype == np.uint8
        wrong |= (ops != wo).any(1)
    bad = np.flatnonzero(wrong)
    assert not len(bad), (len(bad), bad[:4], head[bad[:4]], wh[bad[:4]])


# ---------------------------------------------------------------- A: every length, the kernels up to 128 positions
def every_length(xset, mode, gap, gap_open, kind, swap):
    Y, X = D.rows("YS"), D.rows(xset)
    yi, xi = D.product(len(Y), len(X), 641)
    if swap:
        X, Y, xi, yi = Y, X, yi, xi
    T = D.table(mode, kind)
    want = c_oracle.align_trace(X, Y, xi, yi, T, gap, gap_open, mode)
    xo, yo, table = short(X), short(Y), device_table(mode, T)
    head, ops = _native.alignment_trace(xo, yo, xi, yi, mode, table, gap, gap_open)
    assert xo.valid() and yo.valid()
    same(head, ops, want)
    stats = _native.alignment_stats(xo, yo, xi, yi, mode, table, gap, gap_open)
    same(stats, None, want)
    assert torch.equal(stats, head)                                         # device against device


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("gap,gap_open", D.GAPS)
@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("xset", ["XS", "XN"])
def test_every_length(xset, mode, gap, gap_open, swap):
    """The full product of YS (every length 0..128) with XS and with XN (width 47) in a shuffled order, so that the lanes
    of a wave run lengths of their own: tracer (fit through its own entry) and statistics, head and ops."""
    every_length(xset, mode, gap, gap_open, None, swap)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("mode", D.MODES)
def test_every_length_under_the_extreme_tables(mode, swap):
    """Cost 255 off the diagonal, scores 127 / -128, gap = gap_open = 255, on YS x XN."""
    every_length("XN", mode, *D.GAPS_EXTREME, D.EXTREME, swap)


# ---------------------------------------------------------------- B: every operand width
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("mode", D.MODES)
def test_every_operand_width(mode, swap):
    """For w = 1..128 the y operand is YS cut to w columns (every ND = ceil(w / 8), every yg = ceil(w / 4), the three
    statistics kernels and both sides of 32 | 33 and 64 | 65) against XN; `swap`: the cut operand is x.  head and ops are
    the middle rows of buffers with guard rows before and after, the workspace has guard bytes behind the shares in use:
    every guard survives, and ops is zero from n_ops to ldo."""
    gap, gap_open = D.GAPS[1]
    T = D.table(mode)
    table = device_table(mode, T)
    YS, XN = D.rows("YS"), D.rows("XN")
    for w in range(1, 129):
        yr, xr = D.width_rows(w)
        Y, X = np.ascontiguousarray(YS[yr][:, :w]), np.ascontiguousarray(XN[xr])
        yi, xi = D.product(len(Y), len(X), 650 + w)
        if swap:
            X, Y, xi, yi = Y, X, yi, xi
        want = c_oracle.align_trace(X, Y, xi, yi, T, gap, gap_open, mode)
        xo, yo = short(X), short(Y)
        assert (xo.l, yo.l) == (X.shape[1], Y.shape[1])
        dxi, dyi = _native._pair_lists("test", xo, yo, xi, yi)
        p, ldo = len(xi), X.shape[1] + Y.shape[1]
        waves = -(-p // 64)
        share = _native.aln_trace_wave_bytes(xo.l, yo.l)
        assert share == 64 * xo.l * D.nd(yo.l) * 4
        head = torch.full((p + 2 * GUARD, 8), HEAD_SENTINEL, dtype=torch.int32, device="cuda")
        ops = torch.full((p + 2 * GUARD, ldo), OPS_SENTINEL, dtype=torch.uint8, device="cuda")
        ws = torch.full((waves * share + WS_GUARD,), WS_SENTINEL, dtype=torch.uint8, device="cuda")
        _native._trace_launch(xo, yo, dxi, dyi, 0, p, mode, table, gap, gap_open, head[GUARD:GUARD + p], ops[GUARD:GUARD + p],
                              ws[:waves * share])
        shead = torch.full((p + 2 * GUARD, 8), HEAD_SENTINEL, dtype=torch.int32, device="cuda")
        _native._stats_launch(xo, yo, dxi, dyi, mode, table, gap, gap_open, shead[GUARD:GUARD + p])
        head, ops, shead, tail = head.cpu().numpy(), ops.cpu().numpy(), shead.cpu().numpy(), ws[waves * share:].cpu().numpy()
        same(head[GUARD:GUARD + p], ops[GUARD:GUARD + p], want)
        same(shead[GUARD:GUARD + p], None, want)
        for guard in (head[:GUARD], head[GUARD + p:], shead[:GUARD], shead[GUARD + p:]):
            assert (guard == HEAD_SENTINEL).all(), w
        assert (ops[:GUARD] == OPS_SENTINEL).all() and (ops[GUARD + p:] == OPS_SENTINEL).all() and (tail == WS_SENTINEL).all(), w
        n = want[0][:, 5]
        assert not (ops[GUARD:GUARD + p] * (np.arange(ldo)[None, :] >= n[:, None])).any(), w
        assert xo.valid() and yo.valid()


# ---------------------------------------------------------------- C: the count words at 128, a full row of ops
def test_the_count_extremes_and_a_full_row_of_ops():
    """Widths 128 x 128.  Identical rows (identities = pairs = 128), a full row against an empty one (128 symbols of one
    sequence unaligned: the top field's 128 is the sign bit of the count word), disjoint alphabets under cost 255 (256
    columns, all gaps: ops has no zero tail), 128 matches at score 127, the suffix / prefix overlap, fit with y equal to
    x: the closed form by hand beside the oracle, tracer and statistics."""
    cases = D.extremes()
    X, Y = np.stack([c["x"] for c in cases]), np.stack([c["y"] for c in cases])
    xo, yo = short(X), short(Y)
    assert (xo.l, yo.l) == (128, 128)
    seen = set()
    for k, c in enumerate(cases):
        mode, T, gap, gap_open = c["mode"], c["table"], c["gap"], c["gap_open"]
        pairs = [k, k, k]                                                   # three lanes of one wave
        want = c_oracle.align_trace(X, Y, pairs, pairs, T, gap, gap_open, mode)
        head, ops = _native.alignment_trace(xo, yo, pairs, pairs, mode, device_table(mode, T), gap, gap_open)
        stats = _native.alignment_stats(xo, yo, pairs, pairs, mode, device_table(mode, T), gap, gap_open)
        same(head, ops, want)
        same(stats, None, want)
        head, ops = head.cpu().numpy(), ops.cpu().numpy()
        got = dict(zip(FIELDS, head[0, :7].tolist()), pairs=int((ops[0] == 1).sum()), x_gaps=int((ops[0] == 2).sum()),
                   y_gaps=int((ops[0] == 3).sum()))
        for f, v in c["expect"].items():
            assert got[f] == v, (c["name"], f, got)
        if got["n_ops"] == 256:
            assert ops[0].all()
        seen |= {f for f in ("identities", "pairs", "x_gaps", "y_gaps") if got[f] == 128} | ({"full"} if got["n_ops"] == 256 else set())
    assert seen == {"identities", "pairs", "x_gaps", "y_gaps", "full"}


# ---------------------------------------------------------------- D: strips
def strip_problem(which):
    """(X, Y, xi, yi): YL against 16 rows of XN (the y row changes fastest: the 64 lanes of a wave hold 64 rows of YL, 1 to
    16 strips), or B_MANY against XL (both operands long, shuffled); an x before the `x`: the operands change places."""
    if which in ("YLxXN", "XNxYL"):
        Y, X = D.rows("YL"), np.ascontiguousarray(D.rows("XN")[:16])
        yi, xi = D.lanes_first(len(Y), 16)
    else:
        Y, X = D.rows("B_MANY"), D.rows("XL")
        yi, xi = D.product(len(Y), len(X), 661)
    if which in ("XNxYL", "XLxMANY"):
        X, Y, xi, yi = Y, X, yi, xi
    return X, Y, xi, yi


@pytest.mark.parametrize("gap,gap_open", D.GAPS)
@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("which", ["YLxXN", "XNxYL", "MANYxXL", "XLxMANY"])
def test_every_strip_count(which, mode, gap, gap_open):
    """`alignment_trace_long` (fit through its own entry) at every strip count 1..16 and every tail of the last strip; with a
    long x, 2048 rows of one strip and a small ND.  The heads again from `alignment_trace_long_heads` in at least three
    slices, and the whole again under a workspace of one share and of three."""
    X, Y, xi, yi = strip_problem(which)
    T = D.table(mode)
    want = c_oracle.align_trace(X, Y, xi, yi, T, gap, gap_open, mode)
    xo, yo, table = long(X), long(Y), device_table(mode, T)
    head, ops = _native.alignment_trace_long(xo, yo, xi, yi, mode, table, gap, gap_open)
    assert xo.valid() and yo.valid()
    same(head, ops, want)
    p, ldo = len(xi), X.shape[1] + Y.shape[1]
    heads = _native.alignment_trace_long_heads(xo, yo, xi, yi, mode, table, gap, gap_open, ops_bytes=ldo * (p // 3))
    assert -(-p // (p // 3)) >= 3 and torch.equal(heads, head)
    one = _native.aln_trace_long_wave_bytes(xo.l, yo.l)
    assert one == 64 * xo.l * (D.nd(yo.l) + 2) * 4
    for shares in (1, 3):
        part = _native.alignment_trace_long(xo, yo, xi, yi, mode, table, gap, gap_open, workspace_bytes=shares * one)
        assert torch.equal(part[0], head) and torch.equal(part[1], ops), shares


# ---------------------------------------------------------------- E: the cross-strip tie at every seam
@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("gap_open", [0, 11])
@pytest.mark.parametrize("mode", [LOCAL, SEMIGLOBAL])
def test_the_cross_strip_tie_at_every_seam(mode, gap_open, swap):
    """M pairs with M at the cells up to (36, 8) and N with N up to (8, end), 16 either way; a strip sweep meets (36, 8)
    first, the canonical end cell is the one of the smaller i, in whichever strip 1..15 `end` lies - at its first column
    128 s + 1, inside it, or at the last column 128 s of the strip before."""
    X, Y = D.tie_rows()
    ends = D.tie_ends()
    xi, yi = np.zeros(len(ends), dtype=np.int32), np.arange(len(ends), dtype=np.int32)
    by_hand = [[16, 0, 8, e - 8, e, 8, 8, 0] for e in ends]
    if swap:
        X, Y, xi, yi = Y, X, yi, xi
        by_hand = [[16, 0, 8, 28, 36, 8, 8, 0]] * len(ends)
    S = D.tie_table()
    want = c_oracle.align_trace(X, Y, xi, yi, S, 1, gap_open, mode)
    assert want[0].tolist() == by_hand
    head, ops = _native.alignment_trace_long(long(X), long(Y), xi, yi, mode, device_table(mode, S), 1, gap_open)
    same(head, ops, want)


# ---------------------------------------------------------------- F: a grid smaller than the list
@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("kernel", ["short", "long"])
def test_a_grid_smaller_than_the_list(kernel, mode):
    """The C entry with five chunks of pairs and a workspace of two shares: two waves stride over the list and each share
    is used again by a later chunk.  The wrapper never asks for that (it splits the list into launches); the results are
    the wrapper's and the oracle's."""
    gap, gap_open = D.GAPS[1]
    if kernel == "short":
        Y, X = D.rows("YS"), D.rows("XS")
        yi, xi = D.product(len(Y), len(X), 671)
        pack, wave_bytes, launch, wrapper = short, _native.aln_trace_wave_bytes, _native._trace_launch, _native.alignment_trace
    else:
        Y, X = D.rows("B_MANY"), D.rows("XL")
        yi, xi = D.product(len(Y), len(X), 672)
        pack, wave_bytes, launch, wrapper = long, _native.aln_trace_long_wave_bytes, _native._trace_long_launch, _native.alignment_trace_long
    yi, xi = yi[:300], xi[:300]
    T = D.table(mode)
    want = c_oracle.align_trace(X, Y, xi, yi, T, gap, gap_open, mode)
    xo, yo, table = pack(X), pack(Y), device_table(mode, T)
    dxi, dyi = _native._pair_lists("test", xo, yo, xi, yi)
    one = wave_bytes(xo.l, yo.l)
    ws = torch.empty(2 * one, dtype=torch.uint8, device="cuda")
    head = torch.empty((300, 8), dtype=torch.int32, device="cuda")
    ops = torch.empty((300, xo.l + yo.l), dtype=torch.uint8, device="cuda")
    assert -(-300 // 64) == 5 and ws.numel() // one == 2
    launch(xo, yo, dxi, dyi, 0, 300, mode, table, gap, gap_open, head, ops, ws)
    same(head, ops, want)
    whole = wrapper(xo, yo, xi, yi, mode, table, gap, gap_open)
    assert torch.equal(whole[0], head) and torch.equal(whole[1], ops)
