"""
The strip-mined profile kernel `pg_alignment_profile_long_dense` (prograph_amd/csrc/pg_aln_profile.hip, the frame
`aln_long_profile_frame` of pg_aln_frame.h) at every length, seam and bound, and the operand contract of both profile
entries (include/prograph_hip.h).  Inputs: tests/profile_edges_testdata.py, pinned by tests/test_profile_edges_cpu.py.
    set A   one profile of every length 1..257 in ONE call (yl = 257, lpad = 384) against 64 rows of width 131: every NC of
            a last strip at 1, 2 and 3 strips, ns = 1 on the long kernel, Z from the call's yl
    set B   32 profiles of 3..16 strips, both ends of every NC of a last strip, every nb 1..8 of the second fill of the
            eight slots, 1024 / 1025 / 2047 / 2048
    set C   the long kernel with both sides at most 128 positions: what `search` runs as soon as the fp16 route is left
    bounds  2048 x 2048 on both sides of each mode's 16-bit cell bound, and top = 127 at the last profile length that fits
    one workgroup with one boundary column for six items and 17 profiles of different strip counts
    the operand contract through ctypes: lengths outside 0..yl, row offsets, an operand inside a larger allocation, ldo > n
The yardstick is `definition` of tests/profile_testdata.py, one penalty pair a mode; at 2048 x 2048, where it would take 50 s
a case, closed forms and the operator's torch expression on CPU tensors (tests/test_profile_alignment_cpu.py and
tests/test_profile_edges_cpu.py hold that expression against `definition`).  Every comparison is an every-entry equality.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import profile_edges_testdata as D
from local_testdata import rows_of
from profile_testdata import definition, random_profile
from prograph_amd import _native
from prograph_amd.distance import profile_alignment

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

FITS = {"local": lambda wx, wy, top, gap, gap_open: _native.aln_local_long_fits(wx, wy, top),
        "semiglobal": lambda wx, wy, top, gap, gap_open: _native.aln_semiglobal_long_fits(wx, wy, top),
        "fit": _native.aln_fit_fits}


def tokens(T):
    return torch.from_numpy(np.ascontiguousarray(T).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def x_operand(which, long=True):
    X = D.short_rows(D.LONG_SYMS) if which == "C" else D.long_rows(which)
    xo = (_native.aln_long_operand if long else _native.aln_operand)(tokens(X), D.LONG_SYMS)
    assert xo.valid() and xo.l == X.shape[1]
    return xo


@functools.lru_cache(maxsize=None)
def p_operand(which):
    po = _native.profile_operand(list(D.long_profiles(which)))
    assert (po.bias, po.top) == (6, 9) and po.l == max(len(P) for P in D.long_profiles(which)) and po.lpad == -(-po.l // 128) * 128
    return po


def same(got, want, dtype, shift=0):
    got = got.cpu().numpy()
    assert got.dtype == dtype and got.shape == want.shape
    got = got.astype(np.int64) - shift
    assert np.array_equal(got, want), [(int(r), int(c), int(got[r, c]), int(want[r, c])) for r, c in np.argwhere(got != want)[:8]]
    return True


def run_long(mode, gap, gap_open, xo, po, **kw):
    assert FITS[mode](xo.l, po.l, po.top, gap, gap_open)
    return _native.alignment_profile_long_dense(mode, xo, po, gap, gap_open, **kw)


# ---------------------------------------------------------------- sets A, B and C
@pytest.mark.parametrize("part", [0, 1])
@pytest.mark.parametrize("mode,gap,gap_open", D.LONG_CASES)
def test_every_profile_length_up_to_257_in_one_call(mode, gap, gap_open, part):
    """A profile of l < 257 positions stands beside longer ones: its Z is the call's (yl = 257), its strips its own.  Each
    case runs the whole call and holds every other profile, from `part` on, against the yardstick: half its work a case."""
    xo, po, want = x_operand("A"), p_operand("A"), D.long_want("A", mode, gap, gap_open, part)
    assert want.shape == (129 - part, 64) and (xo.l, po.l, po.lpad, po.n) == (131, 257, 384, 257)
    assert (want > 0).any() and ((want < 0).any() if mode == "fit" else (want >= 0).all())
    whole = run_long(mode, gap, gap_open, xo, po)
    assert same(whole[part::2], want, np.int64)
    assert same(run_long(mode, gap, gap_open, xo, po, out_bytes=4)[part::2], want, np.int32)
    for r0, r1 in ((3, 77), (250, 257)):                          # device against device: the rows of the whole call
        assert torch.equal(run_long(mode, gap, gap_open, xo, po, out_bytes=4, rows=(r0, r1)).long(), whole[r0:r1])
    if mode == "fit":
        K = D.select_bias(mode, gap, gap_open, 257)
        assert same(run_long(mode, gap, gap_open, xo, po, out_bytes=4, bias=K)[part::2], want, np.int32, shift=K)
        assert (want + K).min() == (0 if 257 in D.LENS_A[part::2] else gap)        # the longest profile against the empty row


def one_workgroup(mode, gap, gap_open, xo, po):
    """The C entry with exactly one share of workspace: one workgroup takes every item in turn with one boundary column."""
    one = ctypes.c_int64(0)
    assert _native.lib().pg_alignment_long_workspace(xo.l, ctypes.byref(one), None) == 0
    assert one.value == 256 * 4 * ((xo.l + 3) // 4) * 4
    assert FITS[mode](xo.l, po.l, po.top, gap, gap_open)
    ws = torch.empty(one.value, dtype=torch.uint8, device=xo.buf.device)
    out = torch.empty((po.n, xo.n), dtype=torch.int64, device=xo.buf.device)
    rc = _native.lib().pg_alignment_profile_long_dense(_native.ALN_PROFILE_MODES.index(mode), xo.buf.data_ptr(), xo.n, xo.npad, xo.l,
                                                       po.buf.data_ptr(), po.lengths.data_ptr(), po.n, po.lpad, po.l, po.bias, po.top,
                                                       gap, gap_open, 0, out.data_ptr(), xo.n, 8, ws.data_ptr(), one.value, None)
    assert rc == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode,gap,gap_open", D.LONG_CASES)
def test_every_strip_count_with_every_last_strip(mode, gap, gap_open):
    """Set B whole, and by one workgroup that takes its four groups of eight profiles in turn."""
    xo, po, want = x_operand("B"), p_operand("B"), D.long_want("B", mode, gap, gap_open)
    assert want.shape == (32, 24) and (xo.l, po.l, po.lpad) == (37, 2048, 2048)
    assert (want < 0).all() if mode == "fit" else (want > 0).any() and (want >= 0).all()       # 37 symbols hold no 257 positions
    assert same(run_long(mode, gap, gap_open, xo, po), want, np.int64)
    assert same(run_long(mode, gap, gap_open, xo, po, out_bytes=4), want, np.int32)
    assert same(run_long(mode, gap, gap_open, xo, po, out_bytes=4, rows=(5, 19)), want[5:19], np.int32)
    assert same(one_workgroup(mode, gap, gap_open, xo, po), want, np.int64)


@pytest.mark.parametrize("mode,gap,gap_open", D.LONG_CASES)
def test_the_long_kernel_on_short_operands(mode, gap, gap_open):
    """Profiles of 1, 17 and 128 positions against rows of at most 128 and of at most 37 positions: the long kernel, the
    short kernel and the definition agree."""
    po, want = p_operand("C"), D.long_want("C", mode, gap, gap_open)
    xo = x_operand("C")
    assert (xo.l, po.l, po.lpad) == (128, 128, 128) and want.shape == (3, 134)
    assert same(run_long(mode, gap, gap_open, xo, po), want, np.int64)
    assert same(run_long(mode, gap, gap_open, xo, po, out_bytes=4), want, np.int32)
    assert same(_native.alignment_profile_dense(mode, x_operand("C", long=False), po, gap, gap_open), want, np.int64)
    narrow = definition(mode, D.long_profiles("C"), gap, gap_open, D.long_rows("B"))
    assert same(run_long(mode, gap, gap_open, x_operand("B"), po, out_bytes=4), narrow, np.int32)
    assert same(_native.alignment_profile_dense(mode, _native.aln_operand(tokens(D.long_rows("B")), D.LONG_SYMS), po, gap, gap_open),
                narrow, np.int64)


@pytest.mark.parametrize("mode,gap,gap_open", D.LONG_CASES)
def test_one_workgroup_with_one_boundary_column(mode, gap, gap_open):
    """17 profiles - 2048 positions, then 5, then 129, 1, 1025, 128, 300, ... - against 300 rows of width 131: three groups
    of profiles x two column tiles = six items for one workgroup, whose one boundary column serves profiles of 16 strips,
    then of 1, of 2, ...: a column that a longer profile left must not reach the next one."""
    xo, po, want = x_operand("one"), p_operand("one"), D.long_want("one", mode, gap, gap_open)
    assert want.shape == (17, 300) and (xo.l, po.l) == (131, 2048)
    assert -(-po.n // 8) * -(-xo.n // 256) == 6
    full = run_long(mode, gap, gap_open, xo, po)
    assert same(full, want, np.int64)
    assert torch.equal(one_workgroup(mode, gap, gap_open, xo, po), full)


# ---------------------------------------------------------------- at the bounds of the 16-bit cells
BOUNDS = [("local", 31, 3, 11, 2048, True, 63743), ("local", 32, 3, 11, 2048, False, 65791),
          ("semiglobal", 15, 1, 0, 2048, True, 61695), ("semiglobal", 16, 1, 0, 2048, False, 65791),
          ("fit", 15, 1, 255, 2048, True, 63998), ("fit", 15, 2, 0, 2048, False, 65791), ("fit", 14, 3, 255, 2048, True, 63998),
          ("local", 127, 3, 11, 514, True, 65533), ("local", 127, 3, 11, 515, False, 65660),
          ("semiglobal", 127, 1, 0, 257, True, 65533), ("semiglobal", 127, 1, 0, 258, False, 65787)]


@pytest.mark.parametrize("mode,top,gap,gap_open,wy,inside,cell", BOUNDS)
def test_both_sides_of_every_bound(monkeypatch, mode, top, gap, gap_open, wy, inside, cell):
    """Rows of 2048 positions against a profile of `wy` positions whose position j scores `top` for one symbol and -128 for
    the others (bias = 128), and a short random companion.  Row 0 holds the profile's symbols: it scores wy * top in every
    mode, the largest cell there is (63 488 for local at top = 31).  The yardstick is the operator's torch expression on CPU
    tensors; `definition` would take 50 s here.  Inside the bound the kernel runs, directly and behind the operator; one step
    outside the operator answers through its torch expression on the device and asks the library for no block."""
    assert {"local": D.local_cell(2048, wy, top), "semiglobal": D.semiglobal_cell(2048, wy, top),
            "fit": D.fit_cell(wy, top, gap, gap_open)}[mode] == cell and (cell <= 65535) == inside
    rng = np.random.default_rng(wy + top)
    P, s = D.matched(rng, wy, 4, top, other=-128)
    profiles = [P, np.clip(random_profile(rng, 40, 4), -6, top)]
    X = rows_of(rng, 4, (2048, 2047, 2048, 300, 0), 2048)
    at = 2048 - wy - (700 if wy < 1000 else 0)
    X[0, at:at + wy] = s                                                        # holds the profile
    X[1, :min(wy, 2047)] = s[:2047]
    X[1, 100:2047] = np.concatenate([X[1, 101:2047], [1]])                      # ... with one symbol taken out
    X[1, 50] = 1 + X[1, 50] % 3                                                 # ... and one exchanged
    X[3, :300] = s[wy - 300:] if wy >= 300 else X[3, :300]
    X[3, 7] = 0                                                                 # an interior zero: -128
    op = profile_alignment(mode, gap, gap_open)
    assert op._fits(2048, wy, top) == inside
    want = op(torch.from_numpy(X), profiles).numpy()                            # the torch expression on CPU tensors
    assert want[0, 0] == wy * top and (top != 31 or want[0, 0] == 63488)
    assert want[0, 4] == (-(gap_open + gap * wy) if mode == "fit" else 0) and 0 < want[0, 1] < want[0, 0]
    asked = []
    real = _native.alignment_profile_long_dense
    monkeypatch.setattr(_native, "alignment_profile_long_dense", lambda *a, **kw: (asked.append(1), real(*a, **kw))[1])
    got = op(tokens(X).to(_native.device()), profiles)
    assert got.is_cuda and same(got, want, np.int64) and bool(asked) == inside
    if inside:
        xo, po = _native.aln_long_operand(tokens(X), 4), _native.profile_operand(profiles)
        assert xo.valid() and (po.bias, po.top, po.l) == (128, top, wy)
        assert same(real(mode, xo, po, gap, gap_open, out_bytes=4), want, np.int32)


# ---------------------------------------------------------------- the operand contract, through ctypes
SENTINEL = -77777


def raw_call(long, mode, xo, prof_ptr, lens_ptr, m, lpad, yl, bias, top, gap, gap_open, out_bias, out_bytes, pad=5):
    """One C entry on raw pointers; `out` is (m, n + pad) with ldo = n + pad and SENTINEL everywhere before the call."""
    dtype = {8: torch.int64, 4: torch.int32, 2: torch.float16}[out_bytes]
    out = torch.full((m, xo.n + pad), SENTINEL if out_bytes != 2 else -7.0, dtype=dtype, device=xo.buf.device)
    args = [_native.ALN_PROFILE_MODES.index(mode), xo.buf.data_ptr(), xo.n, xo.npad, xo.l, prof_ptr, lens_ptr, m, lpad, yl, bias, top,
            gap, gap_open, out_bias, out.data_ptr(), out.stride(0), out_bytes]
    if long:
        ws = _native.aln_long_workspace(xo, m)
        rc = _native.lib().pg_alignment_profile_long_dense(*args, ws.data_ptr(), ws.numel(), None)
    else:
        rc = _native.lib().pg_alignment_profile_dense(*args, None)
    assert rc == 0, _native.lib().pg_last_error()
    torch.cuda.synchronize()
    assert (out[:, xo.n:] == (SENTINEL if out_bytes != 2 else -7.0)).all()     # nothing is written behind column n
    return out[:, :xo.n]


def embedded(profiles, lens, before=2, after=3):
    """The packed profiles in the middle of an allocation of 0xFF bytes, `lens` in the middle of one of 2^31 - 1: device
    tensors (kept alive by the caller), the pointers of profile 0, lpad, bias, top."""
    buf, _, l, bias, top = _native.profile_pack(profiles)
    q, lpad = len(profiles), buf.shape[2]
    big = np.full((before + q + after, 32, lpad), 0xFF, dtype=np.uint8)
    big[before:before + q] = buf
    around = np.full(q + 8, 2 ** 31 - 1, dtype=np.int32)
    around[4:4 + q] = lens
    dev = _native.device()
    big, around = torch.from_numpy(big).to(dev), torch.from_numpy(around).to(dev)
    return (big, around), big.data_ptr() + before * 32 * lpad, around.data_ptr() + 16, lpad, bias, top


def contract_case(long):
    """(rows, xo, profiles, yl): 12 profiles, several of yl positions; the short entry at yl = 100 < lpad = 128, the long one
    at yl = 257 < lpad = 384."""
    rng = np.random.default_rng(77 + long)
    yl = 257 if long else 100
    lens = (yl, 5, yl, 129 if long else 17, 1, yl, 130 if long else 64, yl, 16, yl, 33, yl - 1)
    profiles = [random_profile(rng, l, D.LONG_SYMS) for l in lens]
    X = D.long_rows("A") if long else D.short_rows(D.LONG_SYMS)[::2]
    return X, x_operand("A") if long else _native.aln_operand(tokens(X), D.LONG_SYMS), profiles, yl


def padded(P, yl, bias):
    """P as the kernels read it when its length entry says yl or more: the bytes behind its positions are 0, a score of
    -bias for every symbol."""
    return np.concatenate([P, np.full((yl - len(P), P.shape[1]), -bias)])


def check_contract(long, given, expect):
    """`given`: {profile: the entry of `lengths`}; `expect(P, entry, yl, bias)`: the profile the definition scores.  Profiles
    3..11 of an operand that lies inside a larger allocation, every mode, int64 and the entry's small type, ldo = n + 5."""
    X, xo, profiles, yl = contract_case(long)
    lens = np.array([len(P) for P in profiles], dtype=np.int64)
    for q, v in given.items():
        lens[q] = v
    keep, prof_ptr, lens_ptr, lpad, bias, top = embedded(profiles, lens.astype(np.int32))
    assert lpad == (384 if long else 128) and (bias, top) == (6, 9) and yl < lpad
    r0, m = 3, len(profiles) - 3
    scored = [expect(P, int(lens[q]), yl, bias) for q, P in enumerate(profiles)][r0:]
    for mode, gap, gap_open in D.LONG_CASES:
        assert FITS[mode](xo.l, yl, top, gap, gap_open)
        want = definition(mode, scored, gap, gap_open, X)
        shift = 7 if mode == "fit" else 0                                       # out_bias is added in mode 2 alone
        empty = [q - r0 for q, v in given.items() if v <= 0 and q >= r0]
        assert all((want[q] == 0).all() for q in empty)
        for out_bytes in (8, 4 if long else 2):
            K = shift if out_bytes != 2 else D.select_bias(mode, gap, gap_open, yl)
            got = raw_call(long, mode, xo, prof_ptr + r0 * 32 * lpad, lens_ptr + 4 * r0, m, lpad, yl, bias, top, gap, gap_open,
                           K if mode == "fit" else 7, out_bytes)
            assert same(got, want, {8: np.int64, 4: np.int32, 2: np.float16}[out_bytes], shift=K if mode == "fit" else 0), (mode, out_bytes)
    del keep


@pytest.mark.parametrize("long", [False, True], ids=["short", "long"])
def test_lengths_between_yl_and_lpad_count_as_yl(long):
    """Entries yl + 1 and lpad, for profiles of yl positions and for shorter ones (whose bytes up to yl are 0: -bias)."""
    lpad = 384 if long else 128
    yl = 257 if long else 100
    check_contract(long, {0: lpad, 3: yl + 1, 5: yl + 1, 7: lpad, 8: lpad, 10: yl + 1, 11: yl + 1},
                   lambda P, entry, yl, bias: padded(P, yl, bias) if entry > len(P) else P)


@pytest.mark.parametrize("long", [False, True], ids=["short", "long"])
def test_lengths_outside_the_operand_are_clamped(long):
    """10^6 and 2^31 - 1 count as yl; 0, -1 and -2^31 are the empty profile: 0 in every mode, plus out_bias in mode 2."""
    check_contract(long, {2: 10 ** 6, 4: 10 ** 6, 5: 2 ** 31 - 1, 6: 2 ** 31 - 1, 7: 0, 8: -1, 9: -2 ** 31, 10: 0, 3: 0},
                   lambda P, entry, yl, bias: P[:0] if entry <= 0 else padded(P, yl, bias) if entry > len(P) else P)
