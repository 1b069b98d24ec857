"""
Substitution-matrix distance on the GPU: `pg_substitution_dense` (every entry against the definition in numpy below),
`build_graph` / `search` with `distance=substitution(C)` against a stable sort / nonzero of that definition, and the table
1 - I against the reference-generated Hamming goldens.  Every comparison is an every-entry equality.
"""
import operator

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import load_golden
from prograph_amd import synth
from prograph_amd.distance import hamming, substitution

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

PASS = 120                     # positions per LDS image of the kernel (SUB_PASS of pg_sub.hip)
OPS = {"le": operator.le, "lt": operator.lt, "eq": operator.eq, "ge": operator.ge, "gt": operator.gt}


# ---------------------------------------------------------------- the yardstick: the definition
def definition(C, X, Y):
    """(M, N) int64: sum_j C[Y[m, j], X[n, j]] after zero right-padding, in blocks of Y rows."""
    C, X, Y = np.asarray(C, dtype=np.int64), np.asarray(X, dtype=np.intp), np.asarray(Y, dtype=np.intp)
    w = max(X.shape[1], Y.shape[1])
    X, Y = np.pad(X, ((0, 0), (0, w - X.shape[1]))), np.pad(Y, ((0, 0), (0, w - Y.shape[1])))
    out = np.empty((len(Y), len(X)), dtype=np.int64)
    step = max(1, (1 << 24) // max(1, len(X) * w))
    for r in range(0, len(Y), step):
        out[r:r + step] = C[Y[r:r + step, None, :], X[None, :, :]].sum(-1)
    return out


def knn_of(D, k, first):
    order = np.argsort(D, axis=1, kind="stable")[:, first:first + k]
    return order, np.take_along_axis(D, order, 1)


def csr_of(D, comp, eps, keep_zero=False):
    keep = comp(D, eps) & ((D >= 0) if keep_zero else (D > 0))
    r, c = np.nonzero(keep)
    return np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64), c, D[r, c]


def table(rng, a, values):
    """A random symmetric (a, a) table with a zero diagonal, entries drawn from `values`."""
    C = rng.choice(np.asarray(values), size=(a, a))
    C = np.triu(C, 1)
    return C + C.T


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def dense(nat, C, X, Y, **kw):
    a = len(C)
    xo, yo = nat.sub_operand(torch.from_numpy(X.astype(np.uint8)), a), nat.sub_operand(torch.from_numpy(Y.astype(np.uint8)), a)
    assert xo.valid() and yo.valid()
    return nat.substitution_dense(xo, yo, nat.sub_cost(C), **kw)


# ---------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("a", [21, 32])
def test_kernel_against_the_definition(nat, a):
    """16 rows per workgroup, 512 columns per tile, 4 positions per dword, PASS positions per image: every size below,
    at and above them, all combinations."""
    rng = np.random.default_rng(a)
    C = table(rng, a, np.arange(256))
    C[1, a - 1] = C[a - 1, 1] = 255
    for L in (1, 3, 33, PASS - 1, PASS, PASS + 1, 2 * PASS + 60):           # the last: three images
        Xall, Yall = rng.integers(0, a, (1000, L)), rng.integers(0, a, (200, L))
        Xall[5] = 0                                                           # an all-zero row on either side
        Yall[0] = 0
        for M in (1, 15, 17, 200):
            for N in (1, 63, 257, 1000):
                X, Y = Xall[:N], Yall[:M]
                got = dense(nat, C, X, Y)
                assert got.dtype == torch.int64 and got.shape == (M, N)
                assert np.array_equal(got.cpu().numpy(), definition(C, X, Y)), (a, L, M, N)


def test_kernel_more_than_one_tile_and_column_chunk(nat):
    rng = np.random.default_rng(5)
    C = table(rng, 21, np.arange(256))
    X, Y = rng.integers(0, 21, (2100, 40)), rng.integers(0, 21, (70, 40))      # 5 tiles of 512 columns, 5 row blocks
    assert np.array_equal(dense(nat, C, X, Y).cpu().numpy(), definition(C, X, Y))


def test_kernel_sums_beyond_16_bits_and_output_types(nat):
    C = np.zeros((21, 21), dtype=np.int64)
    C[3, 7] = C[7, 3] = 255
    X, Y = np.full((70, 300), 3), np.full((18, 300), 7)
    got = dense(nat, C, X, Y).cpu().numpy()
    assert (got == 76500).all()                                               # 300 * 255: a 16-bit sum fails this
    got32 = dense(nat, C, X, Y, out_bytes=4)
    assert got32.dtype == torch.int32 and (got32.cpu().numpy() == 76500).all()
    # fp16 and int32 equal int64 up to d = 2048 exactly: 64 positions at cost 32
    rng = np.random.default_rng(9)
    C = table(rng, 32, np.arange(33))
    C[1, 2] = C[2, 1] = 32
    X, Y = rng.integers(0, 32, (300, 64)), rng.integers(0, 32, (33, 64))
    X[17], Y[4] = 1, 2
    want = definition(C, X, Y)
    assert want.max() == 2048 and want[4, 17] == 2048
    assert np.array_equal(dense(nat, C, X, Y).cpu().numpy(), want)
    h, i = dense(nat, C, X, Y, out_bytes=2), dense(nat, C, X, Y, out_bytes=4)
    assert h.dtype == torch.float16 and i.dtype == torch.int32
    assert np.array_equal(h.cpu().numpy().astype(np.int64), want) and np.array_equal(i.cpu().numpy().astype(np.int64), want)


def test_kernel_accumulates_column_segments(nat):
    rng = np.random.default_rng(2)
    C = table(rng, 21, np.arange(256))
    X, Y = rng.integers(0, 21, (130, 150)), rng.integers(0, 21, (19, 150))
    xo, yo = (nat.sub_operand(torch.from_numpy(T.astype(np.uint8)), 21) for T in (X, Y))
    cost = nat.sub_cost(C)
    one = nat.substitution_dense(xo, yo, cost)
    for ob in (8, 4):
        two = nat.substitution_dense(xo, yo, cost, out_bytes=ob, cols=(0, 52))
        assert np.array_equal(two.cpu().numpy(), definition(C, X[:, :52], Y[:, :52]))
        two = nat.substitution_dense(xo, yo, cost, cols=(52, 150), out=two)
        assert np.array_equal(two.cpu().numpy(), one.cpu().numpy())
    rows = nat.substitution_dense(xo, yo, cost, rows=(3, 19))                 # a Y operand from row 3 on
    assert np.array_equal(rows.cpu().numpy(), one.cpu().numpy()[3:])
    assert np.array_equal(one.cpu().numpy(), definition(C, X, Y))


# ---------------------------------------------------------------- 1b. several tiles per workgroup, packed sums at their limit
SUB_TILES = 8


def tiles_of(m, n):
    """The tiles of 512 columns one workgroup of `pg_sub_dense_kernel` sweeps per LDS image, as `pg_substitution_dense`
    (prograph_amd/csrc/pg_sub.hip) chooses them: from SUB_TILES = 8, halved while (row blocks of 16) x (column groups of
    `tiles` tiles) stays below 4096 workgroups.  Mirrored here so that a change of the rule makes the tests below say that
    their shapes no longer reach the tile loop."""
    row_blocks, ntiles = -(-m // 16), -(-n // 512)
    tiles = SUB_TILES
    while tiles > 1 and row_blocks * -(-ntiles // tiles) < 4096:
        tiles >>= 1
    return tiles


def test_the_mirrored_tiles_rule_and_the_older_shapes():
    assert tiles_of(70, 2100) == 1 and tiles_of(200, 1000) == 1          # every shape of the tests above: one tile
    assert tiles_of(4096, 50_000) == 4 and tiles_of(65536, 50_000) == 8     # row blocks of a graph at N = 50 000


#                 tiles  M      N     L    table entries  output types
TILE_SHAPES = [(8, 32763, 5637, 5, 256, (2,)),       # groups of tiles 0-7 and 8-11 (breaks at the 12th); 5 columns in the last
               (4, 16375, 6151, 33, 256, (4,)),      # the last workgroup holds a single tile of 7 columns
               (2, 16375, 3172, 121, 17, (2, 4))]    # two LDS images: the tile loop runs again with add = true


@pytest.mark.parametrize("tiles,M,N,L,values,outs", TILE_SHAPES, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_kernel_with_several_tiles_per_workgroup(nat, tiles, M, N, L, values, outs):
    """Shapes at which a workgroup sweeps 8, 4 and 2 tiles with one image: the tile loop beyond its first turn, its
    break past the last tile, the column base of the second group, the operand clamp of lanes beyond npad(N) and the
    re-entry in a second pass.  The Y rows are a random gather of 48 distinct rows (every 16-row group mixes them), so
    the definition is computed on 48 x N and gathered on the device."""
    ntiles = -(-N // 512)
    assert tiles_of(M, N) == tiles, "the tiles rule changed: this shape no longer runs the tile loop as stated"
    assert -(-ntiles // tiles) * tiles > ntiles and M % 16                  # the last column group breaks early
    assert L * (values - 1) <= 2048 or 2 not in outs                        # fp16 holds every distance exactly
    rng = np.random.default_rng(M + N)
    C = table(rng, 21, np.arange(values))
    pool, X = rng.integers(0, 21, (48, L)), rng.integers(0, 21, (N, L))
    pool[0] = 0                                                           # an all-zero row on either side
    X[7] = X[N - 2] = 0
    ids = rng.integers(0, 48, M)
    ids[[5, M - 1]] = 0
    assert min(len(set(g)) for g in ids[:M - M % 16].reshape(-1, 16)) > 4     # every 16-row group mixes pool rows
    dev = nat.device()
    xo = nat.sub_operand(torch.from_numpy(X.astype(np.uint8)), 21)
    yo = nat.sub_operand(torch.from_numpy(pool[ids].astype(np.uint8)), 21)
    assert xo.valid() and yo.valid()
    cost = nat.sub_cost(C)
    ref = torch.from_numpy(definition(C, X, pool)).to(dev)
    ids_dev = torch.from_numpy(ids).to(dev)
    for ob in outs:
        got = nat.substitution_dense(xo, yo, cost, out_bytes=ob)
        want = ref.to(got.dtype)[ids_dev]
        same = got.shape == (M, N) and torch.equal(got, want)
        assert same, (ob, "entries that differ:", int((got != want).sum()), "the first at", torch.nonzero(got != want)[:4].tolist())
        del got, want
    if len(outs) == 2:                                                    # a row range that starts inside a 16-row group
        assert tiles_of(M - 5, N) == tiles
        got = nat.substitution_dense(xo, yo, cost, rows=(5, M))
        same = got.dtype == torch.int64 and torch.equal(got, ref[ids_dev[5:]])
        assert same, "rows=(5, M)"


def _lane_patterns():
    """Groups of 16 Y rows over {0, 1}: 0101.., 1010.., 0011.., 0110.., and a single 1 at each of the 16 places."""
    groups = [[0, 1] * 8, [1, 0] * 8, [0, 0, 1, 1] * 4, [0, 1, 1, 0] * 4] + [[int(i == j) for i in range(16)] for j in range(16)]
    return np.array(groups).reshape(-1)


@pytest.mark.parametrize("L", [PASS - 1, PASS, PASS + 1, 2048])
def test_packed_sums_with_neighbouring_lanes_at_their_limits(nat, L):
    """C[1][2] = 255 and C[1][3] = 0, X rows of 1s, Y rows of 2s (cost 255 at every position) or 3s (cost 0) arranged so
    that the two byte lanes of a 16-bit half hold PASS * 255 and 0 in either order, next to equal lanes: the recovery
    b0 = aw - (ao << 8) borrows, and a lane that leaks into its neighbour shows.  2048 positions: 18 passes, 522 240."""
    C = np.zeros((21, 21), dtype=np.int64)
    C[1, 2] = C[2, 1] = 255
    rows = _lane_patterns()
    X, Y = np.full((70, L), 1), np.where(rows[:, None] == 1, 2, 3) * np.ones((1, L), dtype=np.int64)
    want = definition(C, X, Y)
    assert want.max() == 255 * L and np.array_equal(want[:, 0], rows * 255 * L)
    for ob, dtype in ((8, torch.int64), (4, torch.int32)):
        got = dense(nat, C, X, Y, out_bytes=ob)
        assert got.dtype == dtype and np.array_equal(got.cpu().numpy().astype(np.int64), want), (L, ob)


def test_fp16_accumulation_over_eighteen_passes(nat):
    """2048 positions under 1 - I: every pass adds into the fp16 output, the largest distance is exactly 2048."""
    rng = np.random.default_rng(18)
    C = 1 - np.eye(21, dtype=np.int64)
    X, Y = rng.integers(0, 21, (300, 2048)), rng.integers(0, 21, (33, 2048))
    X[17], Y[4] = 1, 2
    X[40, 100:] = Y[9, 100:]                                              # a near pair: most passes add 0
    want = definition(C, X, Y)
    assert want.max() == 2048 and want[4, 17] == 2048 and want[9, 40] <= 100
    got = dense(nat, C, X, Y, out_bytes=2)
    assert got.dtype == torch.float16 and np.array_equal(got.cpu().numpy().astype(np.int64), want)


def test_pack_flags_tokens_outside_the_table(nat):
    T = np.full((3, 9), 20, dtype=np.uint8)
    assert nat.sub_operand(torch.from_numpy(T), 21).valid()
    T[2, 8] = 21
    assert not nat.sub_operand(torch.from_numpy(T), 21).valid()


def test_operator_on_device_and_host_agree():
    rng = np.random.default_rng(4)
    C = table(rng, 21, np.arange(256))
    dist = substitution(C)
    X, Y = rng.integers(0, 21, (300, 50)), rng.integers(0, 21, (21, 37))       # unequal widths
    want = definition(C, X, Y)
    on_gpu = dist(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda())
    on_cpu = dist(torch.from_numpy(X), torch.from_numpy(Y))
    assert on_gpu.is_cuda and on_gpu.dtype == torch.int64 and not on_cpu.is_cuda
    assert np.array_equal(on_gpu.cpu().numpy(), want) and np.array_equal(on_cpu.numpy(), want)
    half = dist(torch.from_numpy(X).cuda().half(), torch.from_numpy(Y).cuda().half(), similarity=True)
    assert half.dtype == torch.float32 and torch.equal(half, 1 / (1 + on_gpu))
    Xw, Yw = rng.integers(0, 21, (40, 2050)), rng.integers(0, 21, (3, 2050))     # beyond the kernel: the torch expression
    assert np.array_equal(dist(torch.from_numpy(Xw).cuda(), torch.from_numpy(Yw).cuda()).cpu().numpy(), definition(C, Xw, Yw))
    with pytest.raises(ValueError):
        dist(torch.tensor([[1, 21]]).cuda(), torch.tensor([[1, 2]]).cuda())


# ---------------------------------------------------------------- datasets
def _prograph(tmp, tok, name):
    from prograph_amd import Prograph
    f = tmp / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P


def _same_tuples(got, want):
    assert len(got) == len(want)
    for (gi, gw), (wi, ww) in zip(got, want):
        assert gi.dtype == wi.dtype and gw.dtype == ww.dtype
        assert np.array_equal(gi, wi) and np.array_equal(gw, ww)


# ---------------------------------------------------------------- 2. 1 - I reproduces the reference
@pytest.mark.parametrize("name", ["synth_n1000_l32", "synth_n515_l20_dups", "synth_n2085_l64"])
def test_one_minus_identity_reproduces_the_hamming_goldens(name, tmp_path):
    g = load_golden(name)
    P = _prograph(tmp_path, g["tokens"], name)
    dist = substitution(1 - np.eye(32, dtype=np.int64))
    seen = 0
    for key in g.files:
        if "sub" in key or "sim" in key or "ana" in key:
            continue
        if key.startswith("knn") and key.endswith("_idx"):
            k = int(key[3:-4])
            G = P.build_graph(k=k, distance=dist, output="csr")
            assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16      # (uint8 on the Hamming engines)
            assert np.array_equal(G.idx.cpu().numpy(), g[f"knn{k}_idx"]) and np.array_equal(G.dist.cpu().numpy(), g[f"knn{k}_w"])
            _same_tuples(G.to_tuples(), P.build_graph(k=k))
            seen += 1
        elif key.startswith("eps") and key.endswith("_indptr"):
            base = key[:-7]
            assert "_" not in base
            eps = int(base[3:])
            G = P.build_graph(eps=eps, distance=dist, output="csr")
            assert G.weights.dtype == torch.int16
            assert np.array_equal(G.indptr.cpu().numpy(), g[base + "_indptr"])
            assert np.array_equal(G.indices.cpu().numpy(), g[base + "_indices"])
            assert np.array_equal(G.weights.cpu().numpy(), g[base + "_weights"])
            _same_tuples(G.to_tuples(), P.build_graph(eps=eps))
            seen += 1
    assert seen >= 4
    if "knn3_sim_idx" in g.files:
        sub = g["sub_idxs"]
        G = P.build_graph(k=3, distance=dist, idxs=sub, output="csr")
        assert np.array_equal(G.idx.cpu().numpy(), g["knn3_sub_idx"]) and np.array_equal(G.dist.cpu().numpy(), g["knn3_sub_w"])
        sim = P.build_graph(k=3, distance=dist, similarity=True)
        assert np.array_equal(np.array([i for i, _ in sim]), g["knn3_sim_idx"])
        w = np.array([w for _, w in sim])
        assert w.dtype == g["knn3_sim_w"].dtype and np.array_equal(w, g["knn3_sim_w"])
    # search equals search(distance=hamming): strings (shorter, longer, unknown letters), dataset rows, token arrays
    strings = synth.tokens_to_strings(g["tokens"][[3, 77, 400]])
    strings += [strings[0][:-4], strings[1] + "ACDXZ", "WWWW"]
    for q in (strings, g["tokens"][10:14].astype(np.int64)):
        _same_tuples(P.search(q, k=7, distance=dist), P.search(q, k=7, distance=hamming))
        _same_tuples(P.search(q, eps=3, distance=dist), P.search(q, eps=3, distance=hamming))
        _same_tuples(P.search(q, eps=0, distance=dist), P.search(q, eps=0, distance=hamming))


# ---------------------------------------------------------------- 3. weighted graphs against the definition
@pytest.fixture(scope="module")
def weighted(tmp_path_factory):
    """700 clustered rows of 32 positions with duplicates; a table of multiples of 8 up to 48, so that many symbol pairs
    share a cost and distances tie; 32 * 48 = 1536 <= 2048, and queries of up to 42 positions (2016) stay native."""
    tok = synth.clustered_tokens(700, 32, seed=11, members=50)
    tok[40], tok[699] = tok[41], tok[41]
    rng = np.random.default_rng(21)
    C = table(rng, 21, 8 * np.arange(1, 7))
    assert C.max() == 48
    P = _prograph(tmp_path_factory.mktemp("sub"), tok, "weighted")
    return P, tok, C, substitution(C), definition(C, tok, tok)


@pytest.mark.parametrize("k", [1, 16, 70])
def test_weighted_knn_graph(weighted, k):
    P, tok, C, dist, D = weighted
    wi, wd = knn_of(D, k, 1)
    G = P.build_graph(k=k, distance=dist, output="csr")
    assert G.idx.dtype == torch.int32 and G.dist.dtype == torch.int16 and G.first == 1
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    assert k == 1 or (np.diff(wd, axis=1) == 0).any(), "ties must be present"
    got = P.build_graph(k=k, distance=dist)
    assert all(gi.dtype == np.int64 and gw.dtype == np.int64 for gi, gw in got)
    assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)
    sim = P.build_graph(k=k, distance=dist, similarity=True)
    ws = (1 / (1 + torch.from_numpy(wd))).numpy()
    assert all(gw.dtype == np.float32 for _, gw in sim)
    assert np.array_equal(np.array([i for i, _ in sim]), wi) and np.array_equal(np.array([w for _, w in sim]), ws)


@pytest.mark.parametrize("comp,eps", [("le", 96), ("lt", 96), ("eq", 64), ("ge", 1000), ("gt", 999.5), ("le", 40.5)])
def test_weighted_eps_graph(weighted, comp, eps):
    P, tok, C, dist, D = weighted
    ip, ix, w = csr_of(D, OPS[comp], eps)
    assert 0 < ip[-1] < D.size
    G = P.build_graph(eps=eps, distance=dist, comp=OPS[comp], output="csr")
    assert G.indptr.dtype == torch.int64 and G.indices.dtype == torch.int32 and G.weights.dtype == torch.int16
    assert np.array_equal(G.indptr.cpu().numpy(), ip) and np.array_equal(G.indices.cpu().numpy(), ix)
    assert np.array_equal(G.weights.cpu().numpy(), w)
    for i in (40, 41, 699):
        assert not {40, 41, 699} & set(ix[ip[i]:ip[i + 1]])       # d > 0: a row and its duplicates are no neighbours
    got = P.build_graph(eps=eps, distance=dist, comp=OPS[comp], similarity=True)
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]])
        assert not len(gi) or (gw.dtype == np.float32 and np.array_equal(gw, (1 / (1 + torch.from_numpy(w[ip[i]:ip[i + 1]]))).numpy()))


def test_weighted_surface(weighted):
    P, tok, C, dist, D = weighted
    sub = np.arange(100, 400)
    ip, ix, w = csr_of(D[np.ix_(sub, sub)], operator.le, 120)
    got = P.build_graph(eps=120, distance=dist, idxs=sub)
    assert len(got) == len(sub) and ip[-1] > 0
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])      # subset-relative
        assert not len(gi) or (gi.dtype == np.int64 and gw.dtype == np.int64)
    wi, wd = knn_of(D[np.ix_(sub, sub)], 5, 1)
    got = P.build_graph(k=5, distance=dist, idxs=sub)
    assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)
    G = P.build_graph(eps=150, distance=dist, store="S", output="csr")
    assert "S" in P.csr_graphs and P._device_graph("S") is not None
    deg, dirichlet, lv = P.degree("S"), P.dirichlet("S"), P.local_variance("S")
    P.graph["S_host"] = list(P.graph["S"])                       # same rows, no device graph behind them: the tuple route
    assert P._device_graph("S_host") is None
    assert np.array_equal(deg, P.degree("S_host")) and np.isclose(dirichlet, P.dirichlet("S_host"), rtol=1e-9)
    assert np.allclose(lv, P.local_variance("S_host"), equal_nan=True)
    assert (P.adjacency("S") != P.adjacency("S_host")).nnz == 0
    ip, ix, w = csr_of(D, operator.le, 150)
    assert np.array_equal(G.indptr.cpu().numpy(), ip) and np.array_equal(G.weights.cpu().numpy(), w)
    twin = substitution(C.copy())                                # an equal table: the same route, the same graph
    T = P.build_graph(eps=150, distance=twin, output="csr")
    assert T.weights.dtype == torch.int16 and torch.equal(T.indices, G.indices) and torch.equal(T.weights, G.weights)


# ---------------------------------------------------------------- 4. search
def test_search(weighted):
    P, tok, C, dist, D = weighted
    lut = np.array([""] + list(synth.AMINO))
    rng = np.random.default_rng(8)
    rows = tok[rng.integers(0, len(tok), 9)].copy()
    for r in rows[:6]:
        r[rng.integers(0, 32, 3)] = rng.integers(1, 21, 3)
    strings = ["".join(lut[r]) for r in rows]
    strings[0] = strings[0][:25]                                  # shorter than the dataset
    strings[1] = strings[1] + "ACDEFGHIKL"                        # longer
    strings[2] = "XB" + strings[2][2:]                            # unknown letters: token 0
    Q = P.tokenize(strings)
    assert Q.shape[1] == 42 and (Q[2, :2] == 0).all() and np.array_equal(Q[8, :32], rows[8])
    assert Q.shape[1] * C.max() <= 2048
    DQ = definition(C, tok, Q)
    for q in (strings, Q, torch.from_numpy(Q)):
        for k in (1, 5, 70, len(tok) + 5):                        # k >= N: every row, in order
            kk = min(k, len(tok))
            wi, wd = knn_of(DQ, kk, 0)
            got = P.search(q, k=k, distance=dist)
            assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)
            assert got[0][0].dtype == np.int64 and got[0][1].dtype == np.int64
        for comp, eps in (("le", 0), ("le", 100), ("ge", 1000), ("eq", 48), ("lt", 64.5)):
            ip, ix, w = csr_of(DQ, OPS[comp], eps, keep_zero=True)
            got = P.search(q, eps=eps, distance=dist, comp=OPS[comp])
            for i, (gi, gw) in enumerate(got):
                assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]]), (comp, eps, i)
    exact = P.search(strings[8], eps=0, distance=dist)[0]
    assert len(exact[0]) >= 1 and (exact[1] == 0).all()             # a query equal to a dataset row: d = 0 kept
    first = P.search(strings[8], k=2, distance=dist)[0]
    assert first[1][0] == 0 and first[0][0] == exact[0][0]
    G = P.search(Q, k=3, distance=dist, output="csr")
    assert G.first == 0 and G.nrows == len(Q) and G.ncols == len(tok) and G.dist.dtype == torch.int16
    S = P.search(Q, eps=100, distance=dist, output="csr", similarity=True)
    assert S.weights.dtype == torch.int16 and S.nrows == len(Q)
    wi, wd = knn_of(DQ, 1, 0)
    hit, dmin = P.nearest_neighbour(strings[3], distance=dist)
    assert list(hit.index) == [int(wi[3, 0])] and dmin == wd[3, 0]


def test_search_with_fewer_rows_than_k(tmp_path):
    tok = synth.clustered_tokens(40, 12, seed=3, members=8)
    P = _prograph(tmp_path, tok, "small")
    C = table(np.random.default_rng(1), 21, np.arange(1, 100))
    dist = substitution(C)
    DQ = definition(C, tok, tok[:3])
    wi, wd = knn_of(DQ, 40, 0)
    got = P.search(tok[:3].astype(np.int64), k=64, distance=dist)
    assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)


# ---------------------------------------------------------------- 5. the non-native side
def test_beyond_the_fp16_bound_the_generic_loop_gives_the_definition(tmp_path, monkeypatch):
    from prograph_amd import _native
    rng = np.random.default_rng(13)
    tok = rng.integers(1, 21, (90, 683))
    tok[1::3] = tok[0]                                            # near rows: one position apart
    tok[1::3, 5] = rng.integers(1, 21, 30)
    C = table(rng, 21, [1, 2, 3])
    assert C.max() * tok.shape[1] == 2049
    P = _prograph(tmp_path, tok, "wide")
    dist = substitution(C)
    D = definition(C, tok, tok)
    monkeypatch.setattr(_native, "f16_knn", None)                 # the selection layer must not run
    monkeypatch.setattr(_native, "f16_eps", None)
    got = P.build_graph(k=4, distance=dist)
    wi, wd = knn_of(D, 4, 1)
    assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)
    ip, ix, w = csr_of(D, operator.le, 3)
    assert ip[-1] > 0
    got = P.build_graph(eps=3, distance=dist)
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]])
    got = P.search(tok[:2], k=3, distance=dist)
    wi, wd = knn_of(D[:2], 3, 0)
    assert np.array_equal(np.array([i for i, _ in got]), wi) and np.array_equal(np.array([w for _, w in got]), wd)
