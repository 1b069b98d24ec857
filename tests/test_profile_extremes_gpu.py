"""
The profile kernels at the ends of their operand contract (include/prograph_hip.h: entries -128..127, bias 0..128, top
0..127): `pg_alignment_profile_dense`, the operator and `search` on the families of tests/profile_edges_testdata.py - byte
255 in the operand, bias = 0, bias = 128, 16 256 in a cell, the saturating floor at work, a padding trap - every entry
against `definition` of tests/profile_testdata.py (tests/test_profile_edges_cpu.py holds it against a brute force at these
entries and shows that the sets hold what is said here).  bias and top are call-wide and come from the host, so every
family runs in a call of its own AND in one call with all others: a profile's scores must not depend on its companions.
Every comparison is an every-entry equality of integers.
"""
import functools
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import profile_edges_testdata as D
from local_testdata import csr_of, knn_of
from profile_testdata import MODES, definition
from prograph_amd import _native, synth
from prograph_amd.distance import profile_alignment

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

FITS = {"local": lambda wx, wy, top, gap, gap_open: _native.aln_local_long_fits(wx, wy, top),
        "semiglobal": lambda wx, wy, top, gap, gap_open: _native.aln_semiglobal_long_fits(wx, wy, top),
        "fit": _native.aln_fit_fits}


@functools.lru_cache(maxsize=None)
def x_operand(a):
    xo = _native.aln_operand(torch.from_numpy(D.short_rows(a).astype(np.uint8)), a)
    assert xo.valid() and xo.l == 128 and xo.n == 134
    return xo


def same(got, want, dtype, shift=0):
    got = got.cpu().numpy()
    assert got.dtype == dtype and got.shape == want.shape
    got = got.astype(np.int64) - shift
    assert np.array_equal(got, want), [(int(r), int(c), int(got[r, c]), int(want[r, c])) for r, c in np.argwhere(got != want)[:8]]
    return True


def calls_of(a):
    """(name, places in `short_profiles`, (bias, top) the host must find): every family alone, its three shortest profiles
    alone (yl = 16), and all 35 profiles at once."""
    out = []
    for name in D.FAMILIES:
        out.append((name, D.members(name), D.RANGE[name]))
        out.append((name + ", 1..16 positions", D.members(name)[:D.FEW], D.RANGE[name]))
    return out + [("all", list(range(35)), (128, 127))]


def check_calls(a, mode, gap, gap_open):
    """Every call of `calls_of` that the mode's bound admits: int64 always, int64 with the search route's shift in fit mode,
    fp16 wherever every shifted value lies in 0..2048.  Returns the names of the calls that ran, and of those that ran fp16."""
    profiles, want_all, xo = D.short_profiles(a), D.short_want(a, mode, gap, gap_open), x_operand(a)
    ran, halves = [], []
    for name, at, expect in calls_of(a):
        po = _native.profile_operand([profiles[k] for k in at])
        assert (po.bias, po.top) == expect and po.l == max(len(profiles[k]) for k in at) and po.lpad == 128, name
        if not FITS[mode](xo.l, po.l, po.top, gap, gap_open):
            continue
        ran.append(name)
        want = want_all[at]
        assert same(_native.alignment_profile_dense(mode, xo, po, gap, gap_open), want, np.int64), name
        K = D.select_bias(mode, gap, gap_open, po.l)
        if K:
            assert same(_native.alignment_profile_dense(mode, xo, po, gap, gap_open, bias=K), want, np.int64, shift=K), name
        assert (want + K).min() >= 0
        if (want + K).max() <= 2048:
            halves.append(name)
            assert same(_native.alignment_profile_dense(mode, xo, po, gap, gap_open, out_bytes=2, bias=K), want, np.float16, shift=K), name
        if name == "all":
            for r0, r1 in D.ROW_RANGES:
                assert same(_native.alignment_profile_dense(mode, xo, po, gap, gap_open, rows=(r0, r1)), want[r0:r1], np.int64), (r0, r1)
    return ran, halves


# ---------------------------------------------------------------- the short kernel
@pytest.mark.parametrize("gap,gap_open", D.GAPS)
@pytest.mark.parametrize("mode", ["local", "semiglobal"])
@pytest.mark.parametrize("a", D.SYMBOLS)
def test_extreme_profiles_local_and_semiglobal(a, mode, gap, gap_open):
    """Both bounds always hold up to 128 positions (16 511 and 32 767 at top = 127), so every call runs.  fp16: the floor
    family (at most 128 * 1) and every family's profiles of 1, 15 and 16 positions (at most 16 * 127 = 2032)."""
    want = D.short_want(a, mode, gap, gap_open)
    assert want.min() == 0 and want.max() == 16256 == want[D.members("ceiling")[-1], 130]
    ran, halves = check_calls(a, mode, gap, gap_open)
    assert len(ran) == 11
    assert {"floor"} | {name + ", 1..16 positions" for name in D.FAMILIES} <= set(halves) and not {"ceiling", "all"} & set(halves)


@pytest.mark.parametrize("gap,gap_open", D.FIT_GAPS)
@pytest.mark.parametrize("a", D.SYMBOLS)
def test_extreme_profiles_fit(a, gap, gap_open):
    """The pairs that `aln_fit_fits(128, 128, top, gap, gap_open)` admits for the call's top: with top = 127, 255 / 128
    (65 535 exactly) and 254 / 255 (65 534) but not 255 / 255 (65 662), which runs for the floor family (top = 1: 33 406)
    and for the profiles of at most 16 positions (8 654) alone.  fp16 with the shift K = gap_open + gap * yl wherever K + the
    largest score stays within 2048: the floor family at the small penalties (K + 128 <= 523) and its short profiles at
    least; at 1 / 0 the ceiling's short profiles end at 16 + 2032 = 2048 exactly.  From gap 254 on K alone is beyond it."""
    want = D.short_want(a, "fit", gap, gap_open)
    assert want.min() == -(gap_open + 128 * gap) and want.max() == 16256
    ran, halves = check_calls(a, "fit", gap, gap_open)
    few = {name + ", 1..16 positions" for name in D.FAMILIES}
    if (gap, gap_open) == (255, 255):
        assert not _native.aln_fit_fits(128, 128, 127, 255, 255) and set(ran) == few | {"floor"} and not halves
    else:
        assert _native.aln_fit_fits(128, 128, 127, gap, gap_open) and len(ran) == 11
        assert {"floor", "floor, 1..16 positions"} <= set(halves) and "all" not in halves if gap < 254 else not halves


def test_fit_outside_the_bound_takes_the_torch_expression(monkeypatch):
    """255 / 255 with top = 127 at 128 positions is 65 662: the operator on device tensors answers with the definition's
    values through its torch expression, and no dense block is asked of the library."""
    at = D.members("ceiling") + D.members("trap") + D.members("spiky")
    profiles = [D.short_profiles(21)[k] for k in at]
    asked = []
    for name in ("alignment_profile_dense", "alignment_profile_long_dense"):
        real = getattr(_native, name)
        monkeypatch.setattr(_native, name, lambda *a, _f=real, _n=name, **kw: (asked.append(_n), _f(*a, **kw))[1])
    Xd = torch.from_numpy(D.short_rows(21).astype(np.uint8)).to(_native.device())
    got = profile_alignment("fit", 255, 255)(Xd, profiles)
    assert got.is_cuda and got.dtype == torch.int64 and not asked
    assert same(got, D.short_want(21, "fit", 255, 255)[at], np.int64)
    got = profile_alignment("fit", 255, 128)(Xd, profiles)                     # inside: the kernel, the same yardstick
    assert asked == ["alignment_profile_dense"] and same(got, D.short_want(21, "fit", 255, 128)[at], np.int64)
    floor = [D.short_profiles(21)[k] for k in D.members("floor")]              # top = 1: 255 / 255 is inside
    got = profile_alignment("fit", 255, 255)(Xd, floor)
    assert len(asked) == 2 and same(got, D.short_want(21, "fit", 255, 255)[D.members("floor")], np.int64)


@pytest.mark.parametrize("mode", MODES)
def test_the_operator_on_device_tensors(mode):
    """All 35 profiles of 32 symbols through the operator: Profiles' copies, the pack and the route, at 3 / 11."""
    Xd = torch.from_numpy(D.short_rows(32).copy()).to(_native.device())
    got = profile_alignment(mode, 3, 11)(Xd, list(D.short_profiles(32)))
    assert got.is_cuda and same(got, D.short_want(32, mode, 3, 11), np.int64)


# ---------------------------------------------------------------- search: the long kernel on 40-wide operands
N, L = 700, 40


@pytest.fixture(scope="module")
def pg(tmp_path_factory):
    from prograph_amd import Prograph
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=12, seed=9, members=14)
    f = tmp_path_factory.mktemp("profile_extremes") / "profiles.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P, tok


@functools.lru_cache(maxsize=None)
def queries():
    """Nine profiles of at most 40 positions from the ceiling, spiky and trap families."""
    rng = np.random.default_rng(40)
    return tuple(D.family(name, rng, l, 21) for l in (40, 7, 33) for name in ("ceiling", "spiky", "trap"))


def _arrays(got):
    return np.array([np.asarray(i) for i, _ in got]), np.array([np.asarray(w) for _, w in got])


def check_search(P, tok, profiles, op, mode, gap, gap_open, k):
    D_ = definition(mode, profiles, gap, gap_open, tok)
    wi, wd = knn_of(D_, k, 0)
    G = P.search(profiles, k=k, distance=op, output="csr")
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int32 and G.first == 0 and G.similarity is False
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    gi, gw = _arrays(P.search(profiles, k=k, distance=op))
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd)
    mid = int(np.median(D_[D_ > 0]))
    for comp, eps in ((operator.le, mid), (operator.lt, mid - 0.5), (operator.eq, mid), (operator.ge, mid), (operator.gt, mid + 1)):
        G = P.search(profiles, eps=eps, distance=op, comp=comp, output="csr")
        ip, ix, w = csr_of(D_, comp, eps)
        assert ip[-1] > 0 and G.ncols == N and np.array_equal(G.indptr.cpu().numpy(), ip)
        assert np.array_equal(G.indices.cpu().numpy(), ix) and np.array_equal(G.weights.cpu().numpy(), w)
    return wd


@pytest.mark.parametrize("mode", MODES)
def test_search_with_extreme_profiles_selects_from_int32_blocks(pg, mode):
    """40 * 127 > 2048: `_f16_route` is false and the strip-mined kernel runs on 40-wide operands behind `i32_knn` /
    `i32_eps`.  Fit at 20 / 50: K = 850, and a trap profile of 40 positions scores below 0 against every row."""
    P, tok = pg
    profiles = list(queries())
    gap, gap_open = (20, 50) if mode == "fit" else (2, 3)
    op = profile_alignment(mode, gap, gap_open)
    assert not op._f16_route(L, 40, 127) and op._i32_route(L, 40, 127)
    wd = check_search(P, tok, profiles, op, mode, gap, gap_open, 12)
    assert wd.max() > 2048 and (mode != "fit" or (wd < 0).any())


@pytest.mark.parametrize("mode", MODES)
def test_search_with_a_scaled_pssm_of_128_positions(pg, mode):
    """`from_aligned(..., scale=4.0)` of a family of 14 rows of 128 positions: a conserved column scores 17, and
    128 * 17 > 2048 takes fit off the fp16 route (local and semi-global are bounded by the 40 positions of the rows)."""
    P, tok = pg
    rng = np.random.default_rng(128)
    fam = np.tile(rng.integers(1, 21, 128), (14, 1))
    fam[rng.integers(0, 14, 60), rng.integers(0, 128, 60)] = rng.integers(1, 21, 60)
    fam[:, 10:50] = tok[3, :40]                                               # the family holds a row of the dataset
    pssm = profile_alignment.from_aligned(fam, 21, scale=4.0)
    top = int(pssm.max())
    assert pssm.shape == (128, 21) and top == 17 and 128 * top > 2048
    op = profile_alignment(mode, 2, 3)
    assert op._i32_route(L, 128, top) and op._f16_route(L, 128, top) == (mode != "fit")
    D_ = definition(mode, [pssm], 2, 3, tok)
    wi, wd = knn_of(D_, 12, 0)
    G = P.search(pssm, k=12, distance=op, output="csr")
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    assert wd[0, 0] > 50 and (mode != "fit" or (D_ < 0).any())
    G = P.search(pssm, eps=int(wd[0, 5]), distance=op, output="csr")          # s >= the sixth best
    ip, ix, w = csr_of(D_, operator.le, int(wd[0, 5]))
    assert np.array_equal(G.indptr.cpu().numpy(), ip) and np.array_equal(G.indices.cpu().numpy(), ix)
    assert np.array_equal(G.weights.cpu().numpy(), w)
