"""
The alignment kernels at every length, chunk count and strip (inputs: tests/aln_lengths_testdata.py, which
tests/test_alignment_lengths_cpu.py pins): the four kernels up to 128 positions on a Y row of every length 0..128 - every
instance of the row routine, every position of the select chain - and the three kernels beyond 128 positions on every
length 0..256 (set A) and on rows of 3 to 16 strips with every NC in the last strip and every nb of the second profile
fill (set B), against X operands whose widths are no multiple of 4.  The yardsticks are the `definition` functions of
tests/long_testdata.py, tests/local_testdata.py and tests/semiglobal_testdata.py, evaluated once per (set, mode, table,
penalties); every shape is a window of that matrix and every comparison an every-entry equality of integers.
"""
import ctypes

import numpy as np
import pytest
import torch

import aln_lengths_testdata as D
from long_testdata import lengths

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def tokens(T):
    return torch.from_numpy(np.ascontiguousarray(T).astype(np.uint8))


def device_table(nat, mode, table):
    return nat.sub_cost(table) if mode == "global" else nat.aln_local_score(table)


def same(got, want, dtype):
    """Every entry, as integers; the position of the first differences in the message."""
    got = got.cpu().numpy()
    assert got.dtype == dtype and got.shape == want.shape
    got = got.astype(np.int64)
    first = [(int(r), int(c), int(got[r, c]), int(want[r, c])) for r, c in np.argwhere(got != want)[:8]]
    assert np.array_equal(got, want), first
    return True


# ---------------------------------------------------------------- 1. the kernels up to 128 positions
def short_operands(nat, X, Y):
    xo, yo = nat.aln_operand(tokens(X), D.SYMS), nat.aln_operand(tokens(Y), D.SYMS)
    assert xo.valid() and yo.valid()
    return xo, yo


def check_short(kernel, ops, want, fp16):
    """`kernel(xo, yo, **kw)` on set S against the 130 columns: whole, as row ranges that start inside a group of 8 rows,
    both output types where fp16 is exact, and with the operands exchanged (every length on the lane side)."""
    xo, yo = ops
    assert want.shape == (129, 130) and want.min() >= 0
    assert same(kernel(xo, yo), want, np.int64)
    if fp16:
        assert want.max() <= 2048
        assert same(kernel(xo, yo, out_bytes=2), want, np.float16)
    for r0, r1 in ((3, 77), (64, 65)):
        assert same(kernel(xo, yo, rows=(r0, r1)), want[r0:r1], np.int64)
        if fp16:
            assert same(kernel(xo, yo, out_bytes=2, rows=(r0, r1)), want[r0:r1], np.float16)
    assert same(kernel(yo, xo), want.T, np.int64)
    assert same(kernel(yo, xo, rows=(125, 130)), want.T[125:130], np.int64)


SHORT = {"global": "alignment_affine_dense", "local": "alignment_local_dense",
         "semiglobal": "alignment_semiglobal_dense"}


@pytest.fixture(scope="module")
def short(nat):
    return short_operands(nat, D.x("x128"), D.y("S"))


@pytest.mark.parametrize("mode,gap,gap_open,top", D.CASES_S)
def test_every_length_up_to_128(nat, short, mode, gap, gap_open, top):
    """pg_alignment_affine_dense, pg_alignment_local_dense and pg_alignment_semiglobal_dense on the same 129 rows."""
    table = D.table_of(mode, top)
    want = D.want("S", mode, gap, gap_open, top)
    entry = getattr(nat, SHORT[mode])
    dev = device_table(nat, mode, table)
    fp16 = (mode, gap, gap_open) != ("global", 255, 255)          # everywhere else the values stay within 2048
    check_short(lambda xo, yo, **kw: entry(xo, yo, dev, gap, gap_open, **kw), short, want, fp16=fp16)


@pytest.mark.parametrize("gap,top", D.LINEAR_S)
def test_every_length_up_to_128_linear(nat, short, gap, top):
    """pg_alignment_dense: the gaps alone; the yardstick with gap_open = 0."""
    want = D.want("S", "global", gap, 0, top)
    dev = nat.sub_cost(D.cost(top))
    check_short(lambda xo, yo, **kw: nat.alignment_dense(xo, yo, dev, gap, **kw), short, want, fp16=gap != 255)
    assert same(nat.alignment_affine_dense(*short, dev, gap, 0), want, np.int64)


# ---------------------------------------------------------------- 2. the kernels beyond 128 positions
LONG = {"global": "alignment_long_dense", "local": "alignment_local_long_dense",
        "semiglobal": "alignment_semiglobal_long_dense"}


def long_operand(nat, T):
    op = nat.aln_long_operand(tokens(T), D.SYMS)
    assert op.valid()
    return op


def fits(nat, mode, table, gap, gap_open, xw, yw):
    if mode == "global":
        return nat.aln_long_fits(max(xw, yw), max(int(table.max()), gap), gap, gap_open)
    return (nat.aln_local_long_fits if mode == "local" else nat.aln_semiglobal_long_fits)(xw, yw, int(table.max()))


def run_long(nat, mode, table, gap, gap_open, xo, yo, **kw):
    assert fits(nat, mode, table, gap, gap_open, xo.l, yo.l)
    return getattr(nat, LONG[mode])(xo, yo, device_table(nat, mode, table), gap, gap_open, **kw)


def one_workgroup(nat, mode, table, gap, gap_open, xo, yo):
    """The C entry with the smallest workspace: one workgroup loops over all items with one boundary column."""
    one = ctypes.c_int64(0)
    assert nat.lib().pg_alignment_long_workspace(xo.l, ctypes.byref(one), None) == 0
    assert one.value == 256 * 4 * ((xo.l + 3) // 4) * 4            # sized by the width rounded up to 4
    assert fits(nat, mode, table, gap, gap_open, xo.l, yo.l)
    ws = torch.empty(one.value, dtype=torch.uint8, device=xo.buf.device)
    out = torch.empty((yo.n, xo.n), dtype=torch.int64, device=xo.buf.device)
    tab = device_table(nat, mode, table)
    entry = getattr(nat.lib(), "pg_" + LONG[mode])
    x_args, y_args = [xo.buf.data_ptr(), xo.n, xo.npad, xo.l], [yo.buf.data_ptr(), yo.n, yo.npad, yo.l]
    assert entry(*x_args, *y_args, tab.data_ptr(), gap, gap_open, out.data_ptr(), xo.n, 8, ws.data_ptr(), one.value, None) == 0
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def long_ops(nat):
    return {"x47": long_operand(nat, D.x("x47")), "A": long_operand(nat, D.y("A")), "B": long_operand(nat, D.y("B"))}


@pytest.mark.parametrize("mode,gap,gap_open,top", D.CASES_A)
def test_every_length_up_to_256(nat, long_ops, mode, gap, gap_open, top):
    """Set A against the 47-wide X: every NC and select position in strip 0 and in a second, last strip; int64 and int32,
    row ranges from inside a group of 8 rows; and transposed - 257 lanes of 257 lengths against rows of a single strip."""
    table, want = D.table_of(mode, top), D.want("A", mode, gap, gap_open, top)
    xo, yo = long_ops["x47"], long_ops["A"]
    assert want.shape == (257, 70) and xo.l == 47 and yo.l == 256
    assert same(run_long(nat, mode, table, gap, gap_open, xo, yo), want, np.int64)
    assert same(run_long(nat, mode, table, gap, gap_open, xo, yo, out_bytes=4), want, np.int32)
    for r0, r1 in ((3, 77), (250, 257)):
        got = run_long(nat, mode, table, gap, gap_open, xo, yo, out_bytes=4, rows=(r0, r1))
        assert same(got, want[r0:r1], np.int32)
    assert same(run_long(nat, mode, table, gap, gap_open, yo, xo), want.T, np.int64)
    assert same(run_long(nat, mode, table, gap, gap_open, yo, xo, out_bytes=4), want.T, np.int32)


@pytest.mark.parametrize("mode,gap,gap_open,top", D.CASES_B)
def test_every_strip_count_with_every_last_strip(nat, long_ops, mode, gap, gap_open, top):
    """Set B against the 47-wide X: 3 to 16 strips, every NC in the last one, the second profile fill with nb = 1..8;
    int64 and int32, and one workgroup that reuses one boundary column for all 114 rows in turn."""
    table, want = D.table_of(mode, top), D.want("B", mode, gap, gap_open, top)
    xo, yo = long_ops["x47"], long_ops["B"]
    assert want.shape == (114, 70) and xo.l == 47 and yo.l == 2048
    assert same(run_long(nat, mode, table, gap, gap_open, xo, yo), want, np.int64)
    assert same(run_long(nat, mode, table, gap, gap_open, xo, yo, out_bytes=4), want, np.int32)
    assert same(one_workgroup(nat, mode, table, gap, gap_open, xo, yo), want, np.int64)


# ---------------------------------------------------------------- 3. both operands long, many strips
@pytest.mark.parametrize("mode,gap,gap_open,top", D.CASES_MANY)
def test_a_lane_a_length_against_many_strips(nat, mode, gap, gap_open, top):
    """64 lanes of 64 different lengths in 1..199 against rows of 5, 9, 12 and 16 strips, one per NC of the last strip:
    the boundary column is read and written at every outer step, by lanes that stop at different steps; whole, and by
    one workgroup with one boundary column for the eight rows."""
    table, want = D.table_of(mode, top), D.want("many", mode, gap, gap_open, top)
    X, Y = D.x("x199"), D.y_many()
    assert want.shape == (8, 64) and len(set(lengths(X))) == 64
    xo, yo = long_operand(nat, X), long_operand(nat, Y[:, :int(lengths(Y).max())])
    assert xo.l == 199 and yo.l == max(D.B_MANY) == 1992
    assert same(run_long(nat, mode, table, gap, gap_open, xo, yo), want, np.int64)
    assert same(run_long(nat, mode, table, gap, gap_open, xo, yo, out_bytes=4, rows=(3, 8)), want[3:], np.int32)
    assert same(one_workgroup(nat, mode, table, gap, gap_open, xo, yo), want, np.int64)
