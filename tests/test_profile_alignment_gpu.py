"""
Profile (PSSM) queries on the GPU: `pg_alignment_profile_dense` and `pg_alignment_profile_long_dense`
(prograph_amd/csrc/pg_aln_profile.hip), the operator and the search route, every entry against `definition` of
tests/profile_testdata.py (the recurrences as a numpy double loop, held against a brute force over the worded definitions
and against the sequence scores' yardsticks in tests/test_profile_alignment_cpu.py).  Every comparison is exact and no entry
is left out.  Profiles are random per position - not derivable from any table, not symmetric - with entries -6..9, so that
128 * 9 <= 2048 keeps the fp16 blocks exact.
"""
import ctypes
import functools
import operator

import numpy as np
import pandas as pd
import pytest
import torch

from local_testdata import csr_of, knn_of, rows_of, score_table
from profile_testdata import MODES, definition, random_profile
from prograph_amd import _native, synth
from prograph_amd.distance import fit_alignment, local_alignment, profile_alignment, semiglobal_alignment

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

GAPS = ((1, 0), (3, 11), (255, 255))
SHORT_LENS = (1, 15, 16, 17, 33, 127, 128, 40, 64)          # nine profiles: two workgroups, the last one partial
LONG_LENS = (129, 255, 256, 257, 1030)                      # 1030: nine strips, the second batch of the eight slots
TOKEN_OPS = {"local": local_alignment, "semiglobal": semiglobal_alignment, "fit": fit_alignment}


def fits(mode, wx, wy, top, gap, gap_open):
    if mode == "local":
        return _native.aln_local_long_fits(wx, wy, top)
    if mode == "semiglobal":
        return _native.aln_semiglobal_long_fits(wx, wy, top)
    return _native.aln_fit_fits(wx, wy, top, gap, gap_open)


def run(mode, gap, gap_open, X, profiles, out_bytes, long=False, bias=0, rows=None):
    a = profiles[0].shape[1]
    xo = (_native.aln_long_operand if long else _native.aln_operand)(torch.from_numpy(np.ascontiguousarray(X.astype(np.uint8))), a)
    po = _native.profile_operand(profiles)
    assert po.top == 9 and po.bias == 6 and po.l == max(len(p) for p in profiles) and po.lpad % 128 == 0
    assert fits(mode, xo.l, po.l, po.top, gap, gap_open)
    entry = _native.alignment_profile_long_dense if long else _native.alignment_profile_dense
    out = entry(mode, xo, po, gap, gap_open, out_bytes=out_bytes, rows=rows, bias=bias)
    assert xo.valid()
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def short_data(a):
    """(profiles, {name: rows}) for an alphabet of `a` symbols, built once."""
    rng = np.random.default_rng(a)
    profiles = tuple(random_profile(rng, l, a) for l in SHORT_LENS)
    lanes = rows_of(rng, a, list(rng.permutation(129)) + [77], 128)           # 130 rows: every lane its own length 0..128
    lanes[::5, 3] = 0                                                         # interior zeros (and shorter rows where l <= 4)
    many = rows_of(rng, a, rng.integers(0, 41, 600), 40)                      # 600 rows: three column tiles, the last partial
    many[::7, 5] = 0
    return profiles, {"a lane a length": lanes, "600 rows": many}


@functools.lru_cache(maxsize=None)
def short_want(a, mode, gap, gap_open, name):
    profiles, data = short_data(a)
    return definition(mode, profiles, gap, gap_open, data[name])


# ---------------------------------------------------------------- up to 128 positions
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gap,gap_open", GAPS)
@pytest.mark.parametrize("a", [5, 32])
def test_short_kernel_against_the_definition(a, gap, gap_open, mode):
    """int64 and fp16 blocks of every pair.  Fit scores go below 0, so their fp16 block carries the search route's shift
    K = gap_open + gap * 128 and holds 0..K + 128 * 9: exact in fp16 while that is at most 2048, the caller's guarantee in
    include/prograph_hip.h.  At 255 / 255 it is 34 047: there the shifted block is compared as int64 instead."""
    profiles, data = short_data(a)
    for name, X in data.items():
        want = short_want(a, mode, gap, gap_open, name)
        assert (want > 0).any() and ((want < 0).any() if mode == "fit" else (want >= 0).all())
        assert np.array_equal(run(mode, gap, gap_open, X, profiles, 8), want), name
        K = gap_open + gap * 128 if mode == "fit" else 0
        assert (want + K >= 0).all()
        if K + 128 * 9 <= 2048:
            got = run(mode, gap, gap_open, X, profiles, 2, bias=K)
            assert got.dtype == np.float16 and np.array_equal(got.astype(np.int64) - K, want), name
        else:
            assert mode == "fit" and np.array_equal(run(mode, gap, gap_open, X, profiles, 8, bias=K) - K, want), name
    X = data["a lane a length"]
    got = run(mode, gap, gap_open, X, profiles, 8, rows=(3, 9))                # a row range: profiles 3..8
    assert np.array_equal(got, short_want(a, mode, gap, gap_open, "a lane a length")[3:9])


@pytest.mark.parametrize("mode", ["semiglobal", "fit"])
def test_every_profile_length_picks_its_own_last_column(mode):
    """Profile lengths 1..128: the last column at each of the 16 positions of each of the 8 chunk counts."""
    rng = np.random.default_rng(128)
    profiles = [random_profile(rng, l, 21) for l in range(1, 129)]
    X = rows_of(rng, 21, list(rng.permutation(129)) + [60], 128)
    X[::6, 2] = 0
    want = np.concatenate([definition(mode, profiles[l0:l0 + 32], 2, 3, X) for l0 in range(0, 128, 32)])   # tables to 32, 64, ..
    assert np.array_equal(run(mode, 2, 3, X, profiles, 8), want)
    assert (want > 0).any() and (mode != "fit" or (want < 0).any())


# ---------------------------------------------------------------- up to 2048 positions
@functools.lru_cache(maxsize=None)
def long_data():
    rng = np.random.default_rng(2048)
    profiles = tuple(random_profile(rng, l, 21) for l in LONG_LENS)
    rows = rows_of(rng, 21, [0, 1, 300, 299, 128, 129] + list(rng.integers(0, 301, 58)), 300)      # 64 rows of 0..300 symbols
    rows[::4, 7] = 0
    wide = rows_of(rng, 21, [1030, 1025, 513, 0], 1030)                        # the X side long too: nine dwords past 1024
    return profiles, {"64 rows": rows, "4 wide rows": wide}


@pytest.mark.parametrize("mode,gap,gap_open", [("local", 3, 11), ("semiglobal", 1, 0), ("fit", 2, 5)])
def test_long_kernel_against_the_definition(mode, gap, gap_open):
    """One penalty pair a mode (the short kernel's cases cover the penalties; here the strips, the boundary columns and the
    second batch of slots are new): affine, linear, affine."""
    profiles, data = long_data()
    both = np.zeros((68, 1030), dtype=np.int64)                                # one pass of the yardstick over both datasets
    both[:64, :300], both[64:] = data["64 rows"], data["4 wide rows"]
    both = definition(mode, profiles, gap, gap_open, both)
    for name, X, want in (("64 rows", data["64 rows"], both[:, :64]), ("4 wide rows", data["4 wide rows"], both[:, 64:])):
        assert (want > 0).any() and ((want < 0).any() if mode == "fit" else (want >= 0).all())
        assert np.array_equal(run(mode, gap, gap_open, X, profiles, 8, long=True), want), name
        got = run(mode, gap, gap_open, X, profiles, 4, long=True)
        assert got.dtype == np.int32 and np.array_equal(got, want), name
        assert np.array_equal(run(mode, gap, gap_open, X, profiles, 4, long=True, rows=(1, 4)), want[1:4]), name


# ---------------------------------------------------------------- the defining equivalence, on the device
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", [128, 300])
def test_from_sequence_equals_the_token_operator(width, mode):
    rng = np.random.default_rng(width)
    S = score_table(rng, 21, -4, 2, diag=np.arange(3, 8))
    X = rows_of(rng, 21, [0, 1, width, width - 1] + list(rng.integers(0, width + 1, 60)), width)
    Y = rows_of(rng, 21, [1, 16, 17, width, width - 1, 100, 65, 33, 127], width)
    dev = _native.device()
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    profiles = [profile_alignment.from_sequence(y, S) for y in Y]
    for gap, gap_open in ((1, 0), (3, 11)):
        got = profile_alignment(mode, gap, gap_open)(Xd, profiles)
        assert got.is_cuda and got.dtype == torch.int64 and torch.equal(got, TOKEN_OPS[mode](S, gap, gap_open)(Xd, Yd))


# ---------------------------------------------------------------- search
N, L = 700, 40


@pytest.fixture(scope="module")
def pg(tmp_path_factory):
    from prograph_amd import Prograph
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=12, seed=9, members=14)
    f = tmp_path_factory.mktemp("profiles") / "profiles.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok), "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P, tok


@functools.lru_cache(maxsize=None)
def queries():
    """Nine profiles of different lengths: random ones and the PSSM of a family of the dataset."""
    rng = np.random.default_rng(9)
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=12, seed=9, members=14)
    motif = np.full((40, 21), -6)                                             # hard positions: one symbol each, so that most
    motif[np.arange(40), rng.integers(1, 21, 40)] = 9                         # rows hold it nowhere and fit scores go below 0
    return tuple([random_profile(rng, l, 21) for l in (5, 40, 9, 30, 16, 33, 24)] + [motif, profile_alignment.from_aligned(tok[:14, :32], 21)])


def _arrays(got):
    return np.array([np.asarray(i) for i, _ in got]), np.array([np.asarray(w) for _, w in got])


@pytest.mark.parametrize("mode", MODES)
def test_search_against_the_definition(pg, mode):
    P, tok = pg
    profiles = list(queries())
    op = profile_alignment(mode, 2, gap_open=3)
    assert op._f16_route(L, 40, 9)
    D = definition(mode, profiles, 2, 3, tok)
    wi, wd = knn_of(D, 12, 0)
    assert (wd > 0).any() and (mode != "fit" or (wd < 0).any())               # fit: negative scores in the list
    G = P.search(profiles, k=12, distance=op, output="csr")
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.first == 0 and G.similarity is False
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    gi, gw = _arrays(P.search(profiles, k=12, distance=op))
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd)
    mid = int(np.median(D[D > 0]))
    for comp, eps in ((operator.le, mid), (operator.lt, mid - 0.5), (operator.eq, mid), (operator.ge, mid), (operator.gt, mid + 1)):
        G = P.search(profiles, eps=eps, distance=op, comp=comp, output="csr")
        ip, ix, w = csr_of(D, comp, eps)
        assert ip[-1] > 0 and G.ncols == N and np.array_equal(G.indptr.cpu().numpy(), ip)
        assert np.array_equal(G.indices.cpu().numpy(), ix) and np.array_equal(G.weights.cpu().numpy(), w)
    got = P.search(profiles, eps=mid, distance=op, comp=lambda a, b: a <= b)   # outside the five orderings: torch selects
    ip, ix, w = csr_of(D, operator.le, mid)
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]]), i


@pytest.mark.parametrize("mode", MODES)
def test_search_beyond_128_positions_selects_from_int32_blocks(pg, mode):
    P, tok = pg
    rng = np.random.default_rng(140)
    profiles = [random_profile(rng, 140, 21), random_profile(rng, 7, 21)]
    op = profile_alignment(mode, 2, gap_open=3)
    assert not op._f16_route(L, 140, 9) and op._i32_route(L, 140, 9)
    D = definition(mode, profiles, 2, 3, tok)
    G = P.search(profiles, k=9, distance=op, output="csr")
    wi, wd = knn_of(D, 9, 0)
    assert G.dist.dtype == torch.int32 and np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    G = P.search(profiles, eps=1, distance=op, output="csr")
    ip, ix, w = csr_of(D, operator.le, 1)
    assert ip[-1] > 0 and np.array_equal(G.indptr.cpu().numpy(), ip) and np.array_equal(G.indices.cpu().numpy(), ix)
    assert np.array_equal(G.weights.cpu().numpy(), w)


# ---------------------------------------------------------------- the entries' argument checks: no launch
def test_argument_checks_return_before_any_launch():
    lib, p = _native.lib(), ctypes.c_void_p(256)

    def short(mode=0, x=p, n=1, npad=256, xl=8, prof=p, lens=p, m=1, lpad=128, yl=8, bias=0, top=9, gap=1, gap_open=0, obias=0,
              out=p, ldo=1, ob=8):
        return lib.pg_alignment_profile_dense(mode, x, n, npad, xl, prof, lens, m, lpad, yl, bias, top, gap, gap_open, obias, out, ldo, ob, None)

    def long(mode=0, x=p, n=1, npad=256, xl=8, prof=p, lens=p, m=1, lpad=128, yl=8, bias=0, top=9, gap=1, gap_open=0, obias=0,
             out=p, ldo=1, ob=8, ws=p, wsb=1 << 20):
        return lib.pg_alignment_profile_long_dense(mode, x, n, npad, xl, prof, lens, m, lpad, yl, bias, top, gap, gap_open, obias, out,
                                                   ldo, ob, ws, wsb, None)

    BADARG, TOOLONG = -1, lib.pg_alignment_dense(p, 1, 256, 129, p, 1, 256, 8, p, 1, p, 1, 8, None)
    assert TOOLONG not in (0, BADARG)
    for entry in (short, long):
        for kw in ({"mode": 3}, {"mode": -1}, {"gap": 0}, {"gap": 256}, {"gap_open": -1}, {"gap_open": 256}, {"npad": 300}, {"npad": 0},
                   {"x": None}, {"prof": None}, {"lens": None}, {"out": None}, {"n": 0}, {"m": 0}, {"xl": 0}, {"yl": 0}, {"ldo": 0},
                   {"lpad": 100}, {"lpad": 0}, {"lpad": 2176}, {"bias": -1}, {"bias": 129}, {"top": -1}, {"top": 128},
                   {"obias": -1}, {"ob": 1}, {"ob": 4 if entry is short else 2}):
            assert entry(**kw) == BADARG, (entry.__name__, kw)
            assert entry.__name__ in ("short", "long") and b"pg_alignment_profile" in lib.pg_last_error()
    assert short(xl=129) == TOOLONG and short(yl=129, lpad=256) == TOOLONG
    assert long(xl=2049) == TOOLONG and long(yl=2049, lpad=2176) == TOOLONG
    assert long(ws=None) == BADARG and long(wsb=8) == BADARG
