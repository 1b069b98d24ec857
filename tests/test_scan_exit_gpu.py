"""
The exit path of the MFMA engine's hot loop in the short-list kNN instances (pg_mm.h scan() / push_signs):
the flagged links of a stopped super-tile are evaluated again for their sign words, and the queueing loop walks the
flagged tiles by a scalar mask and picks a tile's sign word with masks of the scalar tile index.  Small forced-engine self graphs whose rows are laid out so that
a pass meets, in known super-tiles: candidates in all links at once (more than 64 of them: two batches in one exit),
candidates in the LAST link only, in the FIRST link only, its own rows (the dense forms), and rows that lose their
optimistic cap - a few of a pass (evicted, or the second phase with PG_MM_EVICT=0) and a whole pass of them (the second
phase either way).  Every kNN entry against the C oracle; bit-exact.

The layout is checked on the CPU (test_layout_*: no GPU needed) against a model of the filter: the signature bound
lb = popcount(sig_i ^ sig_j) (pg_sig54 of the plane-0 bits), a pair being a certain candidate when lb is below the row's
FINAL bound min(cap, distance of its k-th neighbour) - bounds only fall during a sweep - and a possible one when lb is
below the cap.
"""
import numpy as np
import pytest
import torch

KS = (1, 16, 19)
CAP = {64: 10, 32: 7}                                        # the optimistic cap of the MFMA engine (pg_api.hip: knnGuess)
N = {64: 1371, 32: 1115}                                     # no multiples of 128: a clamped last super-tile, a short last pass
P0 = 1024                                                    # first row of the pass the planted super-tiles are for


def signature(tok):
    """pg_sig54 of the plane-0 bits: position p = bit p, positions 54..63 folded onto 0..9 (L = 32: the 32 bits)"""
    s = np.zeros(len(tok), dtype=np.uint64)
    for p in range(tok.shape[1]):
        s |= (tok[:, p] & 1).astype(np.uint64) << np.uint64(p)
    if tok.shape[1] > 32:
        s = (s & np.uint64((1 << 54) - 1)) ^ (s >> np.uint64(54))
    return s


def popcount(x):
    return np.unpackbits(np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(axis=-1)


def layout(L):
    """tokens (N, L) and the positions the tests talk about.  Clusters of ~100 (synth.clustered_tokens, members=100: every
    member within 6 of the others); rows are placed by hand:
      positions P0 .. +31  32 members of cluster A       } the 64-row pass 16 (32-row passes 32 and 33); it meets its own
                +32.. +63  32 members of cluster B       } rows - a dense run of super-tiles - only after the planted ones
                 64..127  54 members of cluster C + 10 unrelated rows       (pass 1: a few rows lose their cap)
                128..191  64 unrelated rows                                 (pass 2: the whole pass loses it)
      super-tile 2 (256..): per 32-column tile three more members of A and three of B        -> all links of that pass
      super-tile 4 (512..): seven members of B in tile 3 only                                 -> the last link only
      super-tile 5 (640..): seven members of A in tile 0 only                                 -> the first link only
    everything else: the remaining rows, cluster by cluster (runs of mates: the dense forms), A's and B's at the end."""
    from prograph_amd import synth
    n = N[L]
    src = synth.clustered_tokens(n, L, seed=77 + L, members=100)
    nc = max(1, n // 100)
    rng = np.random.RandomState(L)
    member = [list(np.nonzero(np.arange(n) % nc == c)[0]) for c in range(nc)]
    A, B, C = member[0], member[1], member[2]
    place = {}
    for i in range(32):
        place[P0 + i] = A[i]
        place[P0 + 32 + i] = B[i]
    for i in range(54):
        place[64 + i] = C[i]
    for t in range(4):
        for j in range(3):
            place[256 + 32 * t + j] = A[32 + 3 * t + j]
            place[256 + 32 * t + 10 + j] = B[32 + 3 * t + j]
    for j in range(7):
        place[512 + 96 + 5 + j] = B[44 + j]
        place[640 + 2 + j] = A[44 + j]
    used = set(place.values())
    unrelated = list(range(118, 192))                        # positions of rows without any neighbour
    rest = [r for c in list(range(3, nc)) + [2, 1, 0] for r in member[c] if r not in used]   # (the other members of A, B: last, far from the planted tiles)
    free = [q for q in range(n) if q not in place and q not in unrelated]
    spare = rest[len(free):]                                 # source rows that found no position: overwritten below
    for q, r in zip(free, rest):
        place[q] = r
    tok = np.empty_like(src)
    for q in range(n):
        tok[q] = src[place[q]] if q in place else src[spare.pop()]
    tok[unrelated] = rng.randint(1, 21, size=(len(unrelated), L)).astype(np.uint8)
    return np.ascontiguousarray(tok)


@pytest.fixture(scope="module")
def cases():
    """L -> (tokens, {k: oracle kNN}); computed once, shared, never changed"""
    from oracle import c_oracle as Co
    out = {}
    for L in (64, 32):
        tok = layout(L)
        out[L] = (tok, {k: Co.knn(tok, k, fast=True) for k in KS})
    return out


def filter_model(tok, want_d, L, p0, nr, S):
    """pass rows [p0, p0 + nr) against super-tile S: (certain, possible) candidate matrices, rows x 128 columns"""
    sig = signature(tok)
    c0, c1 = S * 128, min(S * 128 + 128, len(tok))
    lb = np.full((nr, 128), 99, dtype=np.int64)
    lb[:, :c1 - c0] = popcount(sig[p0:p0 + nr, None] ^ sig[None, c0:c1])
    final = np.minimum(CAP[L], want_d[p0:p0 + nr, -1].astype(np.int64))   # (k-th neighbour = entry k + 1 of the list: its threshold)
    return lb < final[:, None], lb < CAP[L]


def links(m, rb):
    """{(tile, row block)} with a set entry; lane slots (column x 4-row group parity: the MFMA's C layout) with one"""
    got, slots = set(), 0
    for t in range(4):
        for b in range(m.shape[0] // 32 if rb == 64 else 1):
            blk = m[32 * b:32 * b + 32, 32 * t:32 * t + 32]
            if blk.any():
                got.add((t, b))
            rows = np.arange(blk.shape[0])
            slots += int(blk[(rows & 4) == 0].any(axis=0).sum() + blk[(rows & 4) != 0].any(axis=0).sum())
    return got, slots


@pytest.mark.parametrize("k", KS)
def test_layout_l64_has_the_super_tiles_it_is_there_for(cases, k):
    """CPU: what the pass at P0 (64 rows; or two 32-row passes) certainly / possibly finds in super-tiles 2, 4, 5 and its own"""
    tok, ref = cases[64]
    d = ref[k][1]
    sure, may = filter_model(tok, d, 64, P0, 64, 2)
    assert sure.sum() > 64                                   # more than one batch in ONE exit
    assert links(sure, 64)[0] == {(t, b) for t in range(4) for b in range(2)}          # all eight links (32-row passes: all four, twice)
    assert links(may, 64)[1] < 2 * 56                        # ... in the MFMA form (pg_mm.h: PG_MM_DENSE_L1 per row block)
    assert links(may[:32], 32)[1] < 56 and links(may[32:], 32)[1] < 56
    sure, may = filter_model(tok, d, 64, P0, 64, 4)
    assert links(sure, 64)[0] == {(3, 1)} == links(may, 64)[0]                          # link 7 and nothing else (32-row pass 1: link 3)
    sure, may = filter_model(tok, d, 64, P0, 64, 5)
    assert links(sure, 64)[0] == {(0, 0)} == links(may, 64)[0]                          # link 0 and nothing else
    sure, may = filter_model(tok, d, 64, P0, 64, P0 // 128)
    assert links(sure, 64)[1] >= 2 * 56                      # its own rows: the signature is not selective, the dense forms


@pytest.mark.parametrize("L", [64, 32])
@pytest.mark.parametrize("k", KS)
def test_layout_has_rows_that_lose_their_cap(cases, L, k):
    """CPU: pass 1 (positions 64..127) holds 10 rows without k neighbours inside the cap (at most PG_MM_EVICT_MAX = 48: evicted),
    pass 2 (128..191) only such rows (more than 48: the second phase inside the pass); the pass at P0 none.  L = 32: more than 64
    certain candidates in super-tile 2 as well."""
    tok, ref = cases[L]
    d = ref[k][1].astype(np.int64)
    lost = d[:, -1] >= CAP[L]
    assert lost[P0:P0 + 64].sum() == 0 and lost[64:128].sum() == 10 and lost[128:192].all()
    assert filter_model(tok, ref[k][1], L, P0, 64, 2)[0].sum() > 64


@pytest.mark.gpu
@pytest.mark.parametrize("evict", ["1", "0"])
@pytest.mark.parametrize("r", ["1", "2"])
@pytest.mark.parametrize("L", [64, 32])
def test_knn_against_the_oracle(cases, monkeypatch, L, r, evict):
    """every entry, k = 1, 16, 19; full passes of 32 / 64 rows (left to the planner a launch this small gets 4-row passes)"""
    from prograph_amd import _native as nat
    tok, ref = cases[L]
    monkeypatch.setenv("PG_ENGINE", "mfma")
    monkeypatch.setenv("PG_MM_R", r)
    monkeypatch.setenv("PG_ROWS_PER_WAVE", "64")
    monkeypatch.setenv("PG_MM_EVICT", evict)
    planes = nat.pack(torch.from_numpy(tok), bits=5)
    for k in KS:
        idx, dist = nat.knn_graph(planes, planes, k)
        assert np.array_equal(idx.cpu().numpy(), ref[k][0]), (L, r, evict, k)
        assert np.array_equal(dist.cpu().numpy(), ref[k][1]), (L, r, evict, k)
    # a window that starts inside the first pass: other rows share the passes, the last one is short
    idx, dist = nat.knn_graph(planes, planes, 16, row0=21, nrows=len(tok) - 21)
    assert np.array_equal(idx.cpu().numpy(), ref[16][0][21:]) and np.array_equal(dist.cpu().numpy(), ref[16][1][21:])
