"""
The chained filter MFMAs of the MFMA engine's hot loop (pg_mm.h scan()): three column tiles share one
accumulator, a super-tile's candidates show as flag bits of its byte fields, and the flagged MFMAs are evaluated again
for their sign words.  Every entry of small forced-engine calls against a host expression (kNN: the canonical
(distance, column) order; eps: the oracle's CSR), for both pass heights (PG_MM_R = 1: chains of tiles 0-2 and tile 3;
2: two row blocks, chains of tiles 0-2 per block and tile 3 of both blocks).  Bit-exact: integer work throughout.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K = 16


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def host_knn_rect(rows, cols, k):
    """Ranks 1..k of the canonical (distance, column) order of every row of `rows` against all of `cols`."""
    d = (rows[:, None, :] != cols[None, :, :]).sum(axis=2).astype(np.int64)
    key = np.sort(d * (1 << 24) + np.arange(len(cols))[None, :], axis=1)[:, 1:k + 1]
    return (key & ((1 << 24) - 1)).astype(np.int32), (key >> 24).astype(np.uint8)


def mutant(seq, dist, rng, lo=10, hi=54):
    """`seq` with `dist` tokens changed in their lowest bit, at positions whose signature bits nothing else folds onto
    (pg_sig54: positions 54..63 share the bits of 0..9): signature bound = Hamming distance = dist."""
    out = seq.copy()
    pos = rng.choice(np.arange(lo, hi), size=dist, replace=False)
    out[pos] ^= 1
    return out


@pytest.fixture(scope="module")
def planted():
    """64 rows (two row blocks) against 3 072 hand-placed columns (24 super-tiles of four 32-column tiles); everything not
    planted is unrelated (distance ~60).  Row q < 16 and row q + 32 share super-tile q: their neighbours sit at the SAME
    in-tile columns of two or three tiles of one accumulator - tiles (0,1), (1,2), (0,2) or (0,1,2) by q % 4 - at
    distances 0..6 around the rows' final bounds (a result of 0 beside one of -1, borrows from a lower field); for
    q % 4 == 3 tile 3 holds columns near BOTH rows (row q + 32 is a neighbour of row q: both fields of the tile-3 chain).
    Rows 16..31 and 48..63 have all their neighbours in ONE tile: positions 0..3 of super-tiles 16..23, either block."""
    rng = np.random.RandomState(5)
    cols = rng.randint(2, 20, size=(3072, 64)).astype(np.uint8)
    rows = rng.randint(2, 20, size=(64, 64)).astype(np.uint8)
    for q in range(16):
        if q % 4 == 3:
            rows[q + 32] = mutant(rows[q], 1, rng)
        tiles = [(0, 1), (1, 2), (0, 2), (0, 1, 2)][q % 4]
        for r, c0 in ((q, 0), (q + 32, 12)):
            for t in tiles:
                for c in range(c0, c0 + 12):
                    cols[q * 128 + t * 32 + c] = mutant(rows[r], int(rng.randint(0, 7)), rng)
        if q % 4 == 3:
            for c in range(24, 32):
                cols[q * 128 + 96 + c] = mutant(rows[q], int(rng.randint(0, 5)), rng)
    for i, r in enumerate(list(range(16, 32)) + list(range(48, 64))):
        for c in range(20):
            cols[(64 + i) * 32 + c] = mutant(rows[r], int(rng.randint(0, 7)), rng)
    return rows, cols, host_knn_rect(rows, cols, K)


def force(monkeypatch, r):
    monkeypatch.setenv("PG_ENGINE", "mfma")
    monkeypatch.setenv("PG_MM_R", r)


@pytest.mark.parametrize("bits", [5, 8])
@pytest.mark.parametrize("r", ["1", "2"])
def test_neighbours_in_one_two_and_three_fields_of_an_accumulator(nat, planted, monkeypatch, r, bits):
    """(i) and (vii): the planted layout, 5 and 8 bit planes"""
    rows, cols, (want_idx, want_d) = planted
    force(monkeypatch, r)
    rp, cp = nat.pack(torch.from_numpy(rows), bits=bits), nat.pack(torch.from_numpy(cols), bits=bits)
    idx, dist = nat.knn_graph(rp, cp, K)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(dist.cpu().numpy(), want_d)


@pytest.fixture(scope="module")
def clustered():
    """name -> (tokens, {(row0, nrows): host kNN}); computed once"""
    from prograph_amd import synth
    out = {}

    def add(name, tok, windows):
        out[name] = (tok, {w: host_knn_rect(tok[w[0]:w[0] + w[1]], tok, K) for w in windows})

    for extra in (1, 33, 97):                                           # (ii) a clamped last super-tile, partial tiles
        n = 128 * 5 + extra
        add(f"ncols_{n}", synth.clustered_tokens(n, 64, seed=41 + extra, members=32), [(n - 70, 70), (0, 40)])
    add("short_passes", synth.clustered_tokens(900, 64, seed=43, members=60), [(100, 19), (300, 45)])      # (iii)
    add("open_bounds", synth.clustered_tokens(1500, 64, seed=44, members=8), [(0, 70), (1431, 69)])        # (iv) clusters < k + 1
    add("one_cluster", synth.clustered_tokens(2000, 64, seed=45, members=2000), [(0, 90)])                 # (v) dense forms
    return out


@pytest.mark.parametrize("r", ["1", "2"])
@pytest.mark.parametrize("name", ["ncols_641", "ncols_673", "ncols_737", "short_passes", "open_bounds", "one_cluster"])
def test_knn_windows(nat, clustered, monkeypatch, name, r):
    """(ii) - (v): self-graph windows; rows past the end of a pass carry bound 0, rows of clusters smaller than k + 1 an
    open bound (the most negative results), one-cluster data leaves the loop for the dense forms"""
    tok, wins = clustered[name]
    force(monkeypatch, r)
    planes = nat.pack(torch.from_numpy(tok), bits=5)
    for (r0, nr), (want_idx, want_d) in wins.items():
        idx, dist = nat.knn_graph(planes, planes, K, row0=r0, nrows=nr)
        assert np.array_equal(idx.cpu().numpy(), want_idx), (name, r0)
        assert np.array_equal(dist.cpu().numpy(), want_d), (name, r0)


@pytest.fixture(scope="module")
def eps_case():
    """(vi) L = 32 (one group: a 32-bit signature), clustered, with neighbours at distances 1, 2 (inside eps = 2) and 3
    (a filter result of exactly 0) planted at the same in-tile column of the three tiles of one accumulator"""
    from oracle import prograph_oracle as O
    from prograph_amd import synth
    rng = np.random.RandomState(9)
    tok = synth.clustered_tokens(1500, 32, seed=46, members=50)
    tok[200:1300] = rng.randint(2, 20, size=(1100, 32))                 # unrelated in the middle
    for i, row in enumerate(range(640, 672)):                          # rows of one pass; their neighbours in super-tile 3
        for t, dist in enumerate([(3, 1, 2), (1, 3, 3), (2, 2, 1), (3, 3, 3)][i % 4]):
            tok[384 + 32 * t + i] = mutant(tok[row], dist, rng, 0, 32)
    t64 = tok.astype(np.int64)
    return tok, {e: O.neighbours_to_csr(O.build_graph(t64, eps=e)) for e in (1, 2)}


@pytest.mark.parametrize("sym", ["0", "1"])
@pytest.mark.parametrize("eps", [1, 2])
def test_eps_and_symmetric_eps_against_the_oracle(nat, eps_case, monkeypatch, eps, sym):
    tok, ref = eps_case
    monkeypatch.setenv("PG_ENGINE", "mfma")
    monkeypatch.setenv("PG_EPS_SYM", sym)
    planes = nat.pack(torch.from_numpy(tok), bits=5)
    indptr, idx, w = [x.cpu().numpy() for x in nat.eps_graph(planes, planes, nat.CMP_LE, eps, cap=32)]
    want = ref[eps]
    assert np.array_equal(indptr, want[0]) and np.array_equal(idx, want[1]) and np.array_equal(w, want[2])
