"""
The yardstick and the inputs of tests/test_alignment_trace_lengths_gpu.py, without a GPU: `oracle.c_oracle.align_trace`
(orc_align_trace, oracle/oracle.c) against `definition` of tests/trace_testdata.py and `canonical` of tests/fit_testdata.py
field for field and op for op, its score against `brute_force`, the product's CPU route `alignments.host_trace` against it,
what the lengths of tests/trace_lengths_testdata.py cover - asserted from the lengths alone - the extreme pairs on the
oracle's own output, and the two host programs (tests/capi_trace, tests/capi_stats) with their length sweeps under the
address and undefined-behaviour sanitizers.
"""
import os
import subprocess

import numpy as np
import pytest

import fit_testdata
import trace_lengths_testdata as D
from trace_testdata import FIELDS, GLOBAL, LOCAL, SEMIGLOBAL, brute_force, definition
from oracle import c_oracle
from prograph_amd import alignments

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIT = D.FIT
CASES = [(e, o, None) for e, o in D.GAPS + (D.GAPS_EXTREME,)] + [D.GAPS_EXTREME + (D.EXTREME,)]


def python_answer(mode, T, gap, gap_open, x, y):
    """(head list of 8, ops list) of one pair by the Python yardsticks."""
    if mode == FIT:
        c = fit_testdata.canonical(T, gap, gap_open, fit_testdata.seq(x), fit_testdata.seq(y))
        return list(c[:7]) + [0], c[7]
    d = definition(mode, T, gap, gap_open, x, y)
    return [d[f] for f in FIELDS] + [0], d["ops"]


def thinned(rng):
    """150 pairs at lengths up to 40, three at 120..128 and one at 130..300: (X, Y, xi, yi)."""
    lx = [int(v) for v in rng.integers(0, 41, 60)] + [0, 1, 40] + [int(v) for v in rng.integers(120, 129, 3)] + [int(rng.integers(130, 301))]
    ly = [int(v) for v in rng.integers(0, 41, 60)] + [0, 1, 40] + [int(v) for v in rng.integers(120, 129, 3)] + [int(rng.integers(130, 301))]
    X, Y = np.zeros((len(lx), 300), dtype=np.uint8), np.zeros((len(ly), 300), dtype=np.uint8)
    for M, lens in ((X, lx), (Y, ly)):
        for r, l in enumerate(lens):
            M[r, :l] = rng.integers(0, D.A, l)
            if l:
                M[r, l - 1] = rng.integers(1, D.A)
    for r in range(0, 60, 3):                                               # related rows: long diagonals, real gaps
        l = min(lx[r], ly[r])
        Y[r, :l] = X[r, :l]
        if l > 4:
            Y[r, 2:l - 1] = X[r, 3:l]
            Y[r, l - 1] = max(1, Y[r, l - 1])
    xi = np.concatenate([rng.integers(0, 63, 147), [60, 61, 60], [63, 64, 65], [66]])
    yi = np.concatenate([rng.integers(0, 63, 147), [60, 60, 61], [64, 65, 63], [66]])
    return X, Y, xi.astype(np.int32), yi.astype(np.int32)


@pytest.mark.parametrize("gap,gap_open,kind", CASES)
@pytest.mark.parametrize("mode", D.MODES)
def test_the_oracle_is_the_definition(mode, gap, gap_open, kind):
    """Sixteen lists of 154 pairs, a couple of thousand at lengths up to 40, 48 at 120..128 and 16 at 130..300: every field
    and every op, and zeros from n_ops to ldo."""
    rng = np.random.default_rng(100 * mode + gap + gap_open + (7 if kind else 0))
    X, Y, xi, yi = thinned(rng)
    T = D.table(mode, kind)
    head, ops = c_oracle.align_trace(X, Y, xi, yi, T, gap, gap_open, mode)
    assert head.shape == (len(xi), 8) and head.dtype == np.int32 and ops.shape == (len(xi), 600) and ops.dtype == np.uint8
    for p in range(len(xi)):
        h, o = python_answer(mode, T, gap, gap_open, X[xi[p]], Y[yi[p]])
        assert head[p].tolist() == h, (p, head[p], h)
        assert ops[p, :h[5]].tolist() == o and not ops[p, h[5]:].any(), p
    assert (head[:, 5] == 0).any() and (mode != GLOBAL or int(head[:, 5].max()) > 128)


@pytest.mark.parametrize("mode", D.MODES)
def test_the_oracle_scores_are_brute_force(mode):
    """Every alignment path of every admissible pair of substrings, sequences of up to five symbols."""
    rng = np.random.default_rng(40 + mode)
    rows = np.zeros((12, 5), dtype=np.uint8)
    for r in range(12):
        l = r % 6
        rows[r, :l] = rng.integers(0, 4, l)
        if l:
            rows[r, l - 1] = rng.integers(1, 4)
    xi, yi = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(np.arange(12), np.arange(12)))
    for gap, gap_open in ((1, 0), (2, 1), (1, 3)):
        T = D.table(mode)[:4, :4]
        head, _ = c_oracle.align_trace(rows, rows, xi, yi, T, gap, gap_open, mode)
        for p in range(0, len(xi), 2 if mode == LOCAL else 1):
            x, y = rows[xi[p]], rows[yi[p]]
            want = (fit_testdata.brute_force(T, gap, gap_open, fit_testdata.seq(x), fit_testdata.seq(y)) if mode == FIT
                    else brute_force(mode, T, gap, gap_open, x, y))
            assert head[p, 0] == want, (p, x, y, head[p], want)


def test_the_oracle_refuses_what_it_cannot_hold():
    big = np.ones((1, 2048), dtype=np.uint8)
    with pytest.raises(ValueError, match="cells"):
        c_oracle.align_trace(big, big[:, :300], [0], [0], D.table(LOCAL), 2, 0, LOCAL)
    with pytest.raises(ValueError, match="outside the table"):
        c_oracle.align_trace(np.full((1, 4), D.A, dtype=np.uint8), big[:, :4], [0], [0], D.table(LOCAL), 2, 0, LOCAL)
    with pytest.raises(ValueError, match="outside its operand"):
        c_oracle.align_trace(big[:, :4], big[:, :4], [1], [0], D.table(LOCAL), 2, 0, LOCAL)
    head, ops = c_oracle.align_trace(big, big[:, :199], [0], [0], D.table(LOCAL), 2, 0, LOCAL)       # the largest pair of the tests
    assert head[0, 5] == 199 and ops.shape == (1, 2247)


@pytest.mark.parametrize("mode", D.MODES)
def test_host_trace_is_the_oracle(mode):
    """`alignments.host_trace`, the product's CPU route, on YS x XS: all 8 256 pairs, every fourth one per mode (host_trace
    takes a millisecond per pair), the gap pairs alternating with the mode."""
    YS, XS = D.rows("YS"), D.rows("XS")
    yi, xi = D.product(len(YS), len(XS), 631)
    yi, xi = yi[mode::4], xi[mode::4]
    gap, gap_open = D.GAPS[mode % 2]
    T = D.table(mode)
    head, ops = c_oracle.align_trace(XS, YS, xi, yi, T, gap, gap_open, mode)
    *fields, hops = alignments.host_trace(mode, T, gap, gap_open, XS, YS, xi, yi)
    assert np.array_equal(np.stack(fields, 1), head[:, :7]) and np.array_equal(hops, ops)


def test_what_the_lengths_cover():
    YS, XS, XN, YL, XL = (D.rows(n) for n in ("YS", "XS", "XN", "YL", "XL"))
    assert YS.shape == (129, 128) and XS.shape == (64, 128) and XN.shape == (64, 47) and YL.shape[1] == 2048 and XL.shape == (64, 199)
    assert all(M.dtype == np.uint8 and int(M.max()) < D.A for M in (YS, XS, XN, YL, XL))
    # A: every y length 0..128, on either operand side (both operand orders run), against x of the dword edges
    assert D.lengths(YS).tolist() == D.lens_ys() and sorted(D.lens_ys()) == list(range(129))
    assert {0, 1, 15, 16, 17, 63, 64, 65, 127, 128} <= set(D.lengths(XS).tolist()) and D.lengths(XS).tolist() != sorted(D.lengths(XS).tolist())
    assert {0, 1, 47} <= set(D.lengths(XN).tolist())
    zeros = [r for r in range(129) if (YS[r, :D.lengths(YS)[r]] == 0).any()]
    assert len(zeros) >= 15 and all(r % 5 == 0 for r in zeros)
    # B: every operand width 1..128: every ND and yg, the three statistics kernels and both sides of their seams
    widths = range(1, 129)
    assert {D.nd(w) for w in widths} == set(range(1, 17)) and {D.yg(w) for w in widths} == set(range(1, 33))
    assert [D.stats_instance(w) for w in (1, 32, 33, 64, 65, 128)] == [32, 32, 64, 64, 128, 128]
    assert {D.stats_instance(w) for w in widths} == {32, 64, 128}
    for w in widths:
        yr, xr = D.width_rows(w)
        cut = D.lengths(YS[yr][:, :w])
        assert len(yr) * len(xr) == 128 and len(set(yr.tolist())) == 16 and len(set(xr.tolist())) == 8
        assert cut.max() == w and (cut == 0).any()                          # the last token and direction dword; an empty row
        assert (cut > 4 * ((w - 1) // 4)).any() and (cut > 8 * ((w - 1) // 8)).any()
        assert {0, 47} <= set(D.lengths(XN[xr]).tolist())
    # D: every strip count and every tail, lanes of one wave far apart
    ll = D.lengths(YL)
    assert ll.tolist() == D.lens_yl() and len(set(ll.tolist())) == len(ll) and set(D.LONG_EDGES) <= set(ll.tolist())
    assert {D.strips(l) for l in ll} == set(range(0, 17)) and {D.tail_dwords(l) for l in ll} == set(range(0, 17))
    yi, xi = D.lanes_first(len(YL), 16)
    first = [D.strips(ll[r]) for r in yi[:64]]
    assert len(set(yi[:64].tolist())) == 64 and min(s for s in first if s) == 1 and max(first) == 16
    assert sorted(set(D.lengths(XL).tolist())) == sorted(D.lengths(XL).tolist()) and D.lengths(XL).max() == 199 and D.lengths(XL).min() == 1
    assert D.lengths(D.rows("B_MANY")).tolist() == D.B_MANY and sorted({D.strips(l) for l in D.B_MANY}) == [5, 9, 12, 16]
    # the oracle holds every pair of the tests
    assert 2049 * 200 <= c_oracle.TRACE_MAX_CELLS
    # E: every seam 1..15, the column before it and the column after it
    ends = D.tie_ends()
    assert {e for e in ends if e % 128 == 0} == {128 * s for s in range(1, 16)}
    assert {e for e in ends if e % 128 == 1} == {128 * s + 1 for s in range(1, 16)}
    assert {D.strips(e) - 1 for e in ends if e % 128 > 1} == set(range(1, 16)) and max(ends) <= 2048


def counts(ops):
    return {"pairs": int((ops == 1).sum()), "x_gaps": int((ops == 2).sum()), "y_gaps": int((ops == 3).sum())}


def test_the_extremes_get_there():
    """The oracle's own answer on the hand-built pairs: a field of the count word at 128 (identities, pairs, x symbols
    unaligned, y symbols unaligned), a row of ops filled to len x + len y = 256, fit with len x = 0, local 128 x 127."""
    seen = {}
    for c in D.extremes():
        head, ops = c_oracle.align_trace(c["x"][None], c["y"][None], [0], [0], c["table"], c["gap"], c["gap_open"], c["mode"])
        got = dict(zip(FIELDS, head[0, :7].tolist()), **counts(ops[0]))
        for f, v in c["expect"].items():
            assert got[f] == v, (c["name"], f, got)
        assert got["n_ops"] == got["pairs"] + got["x_gaps"] + got["y_gaps"]
        for f in ("identities", "pairs", "x_gaps", "y_gaps", "n_ops", "score"):
            seen[f] = max(seen.get(f, 0), got[f])
        if got["n_ops"] == 256:
            assert ops.shape == (1, 256) and ops[0].all() and got["x_gaps"] == got["y_gaps"] == 128
    assert seen == dict(identities=128, pairs=128, x_gaps=128, y_gaps=128, n_ops=256, score=128 * 127)
    names = [c["name"] for c in D.extremes()]
    assert "fit empty x, full y" in names and len(set(names)) == len(names)


@pytest.mark.parametrize("mode", [LOCAL, SEMIGLOBAL])
def test_the_cross_strip_tie_by_hand(mode):
    """The construction of test E: the oracle gives the end cell of the smaller i, whichever strip it lies in."""
    X, Y = D.tie_rows()
    ends = D.tie_ends()
    for gap_open in (0, 11):
        head, ops = c_oracle.align_trace(X, Y, np.zeros(len(ends), dtype=np.int32), np.arange(len(ends)), D.tie_table(), 1, gap_open, mode)
        assert head[:, :5].tolist() == [[16, 0, 8, e - 8, e] for e in ends] and (ops[:, :8] == 1).all() and not ops[:, 8:].any()
        head, ops = c_oracle.align_trace(Y, X, np.arange(len(ends)), np.zeros(len(ends), dtype=np.int32), D.tie_table(), 1, gap_open, mode)
        assert head[:, :5].tolist() == [[16, 0, 8, 28, 36]] * len(ends) and (head[:, 5:7] == 8).all()


@pytest.mark.parametrize("which,said", [("capi_trace", "trace routines OK"), ("capi_stats", "stats routines OK")])
def test_the_host_programs_sweep_every_length(which, said):
    """tests/capi_trace/trace_check.cpp and tests/capi_stats/stats_check.cpp, stand-alone programs compiled with
    -fsanitize=address,undefined: every len y 0..128 against ten len x, both ways round, four modes, and the extreme pairs.
    Their argument "sweep" runs that part alone; tests/test_alignment_trace_cpu.py and tests/test_alignment_stats_cpu.py run
    the programs whole."""
    capi = os.path.join(REPO, "tests", which)
    subprocess.check_call(["make", "-s", "-C", capi])
    out = subprocess.run([os.path.join(capi, "_build", which.replace("capi_", "") + "_check"), "sweep"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and said in out.stdout and "sweep" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
