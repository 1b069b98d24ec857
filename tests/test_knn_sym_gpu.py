"""
The symmetric kNN sweep of a self graph (pg_mm_knn_sym_kernel, pg_knn_sym_merge_kernel): every unordered pair
is evaluated once, by the pass of its lower row, and delivered to the higher row.  Forced with PG_KNN_SYM=1 on small self
graphs - the shapes at which the diagonal block, the seams and the delivery can go wrong: two row blocks in one super-tile
(65), super-tile and block seams and a last block of one row (128, 129, 193), several blocks and pieces (1000, 3000).  Every
entry of indices and distances against the C oracle AND byte for byte against the rectangular path (PG_KNN_SYM=0) in the same
process; k = 1, 16, 19, L = 64.

Data: the generator's strided clusters of 256, 64 and 12 members (12 < k + 1: every row loses the cap, the merge evicts
them all and the gated rectangular launch takes over), contiguous clusters (a pass's own super-tile holds up to 64
candidates a column: the dense forms), exact duplicates on either side of a row (distance-0 ties, index tie-breaks) and
1 % unrelated rows (evicted: pg_knn_rows_kernel finishes them).  Forced: slots of 8 delivered keys (rows overflow and are
evicted; with a limit of 0 the rectangular fallback runs), pieces that cut a block's columns in 2 and in 7.
"""
import numpy as np
import pytest
import torch

KS = (1, 16, 19)
L = 64
NS = (65, 128, 129, 193, 1000, 3000)
KINDS = ("strided256", "strided64", "strided12", "contiguous")


def tokens(n, kind):
    from prograph_amd import synth
    members = {"strided256": 256, "strided64": 64, "strided12": 12, "contiguous": 64}[kind]
    tok = synth.clustered_tokens(n, L, seed=1400 + n, members=members)
    rng = np.random.RandomState(n)
    if kind == "contiguous":                                 # mates side by side: cluster by cluster
        nc = max(1, n // members)
        tok = tok[np.argsort(np.arange(n) % nc, kind="stable")]
    tok = np.ascontiguousarray(tok)
    # exact duplicates: a copy BELOW its original (the duplicate has the lower index) and one ABOVE it, near and far
    for a, b in ((3, n - 2), (n - 1, 7), (n // 2, n // 2 + 1), (min(n - 1, 70), 1)):
        tok[a] = tok[b]
    # 1 % unrelated rows (at least one)
    for r in rng.choice(n, size=max(1, n // 100), replace=False):
        tok[r] = rng.randint(1, 21, size=L).astype(np.uint8)
    return tok


_cache = {}


def case(n, kind):
    """(tokens, {k: oracle kNN}); computed once per shape and kind, shared, never changed"""
    from oracle import c_oracle as Co
    if (n, kind) not in _cache:
        tok = tokens(n, kind)
        _cache[(n, kind)] = (tok, {k: Co.knn(tok, k, fast=True) for k in KS})
    return _cache[(n, kind)]


def check(monkeypatch, capfd, n, kind, env, ks=KS):
    """... and the planner's debug line says which launch ran: the forced call is the symmetric one, PG_KNN_SYM=0 is not"""
    from prograph_amd import _native as nat
    tok, ref = case(n, kind)
    monkeypatch.setenv("PG_ENGINE", "mfma")
    monkeypatch.setenv("PG_DEBUG_PLAN", "1")
    monkeypatch.setenv("PG_MM_R", "2")
    planes = nat.pack(torch.from_numpy(tok), bits=5)
    for k in ks:
        monkeypatch.setenv("PG_KNN_SYM", "0")
        capfd.readouterr()
        ridx, rdist = [x.cpu().numpy() for x in nat.knn_graph(planes, planes, k)]
        assert "[pg plan sym]" not in capfd.readouterr().err, (n, kind, k, "PG_KNN_SYM=0 took the symmetric path")
        monkeypatch.setenv("PG_KNN_SYM", "1")
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        idx, dist = [x.cpu().numpy() for x in nat.knn_graph(planes, planes, k)]
        for key in env:
            monkeypatch.delenv(key)
        assert f"[pg plan sym] rows={n}:" in capfd.readouterr().err, (n, kind, k, env, "the forced call declined the symmetric path")
        assert np.array_equal(idx, ref[k][0]) and np.array_equal(dist, ref[k][1]), (n, kind, k, env, "oracle")
        assert idx.tobytes() == ridx.tobytes() and dist.tobytes() == rdist.tobytes(), (n, kind, k, env, "rectangular path")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", NS)
def test_symmetric_sweep_against_oracle_and_rectangular_path(monkeypatch, capfd, n, kind):
    """the eviction limit out of reach: the gated rectangular launch never runs, what is compared is the merge's own
    output (and pg_knn_rows_kernel's for the rows the merge evicts)"""
    check(monkeypatch, capfd, n, kind, {"PG_KNN_SYM_EVICT_LIMIT": "100000000"})


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["strided64", "strided12"])
@pytest.mark.parametrize("n", NS)
def test_default_eviction_limit(monkeypatch, capfd, n, kind):
    """N / 16 evicted rows at most: clusters of 12 lose the cap in every row - the rectangular fallback; clusters of 64 stay"""
    check(monkeypatch, capfd, n, kind, {}, ks=(16,))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["strided64", "contiguous"])
@pytest.mark.parametrize("n", [1000, 3000])
def test_slots_of_eight_delivered_keys_overflow(monkeypatch, capfd, n, kind):
    """capL = 8 against clusters of 64: most rows receive more keys than their slot holds.  First the evicted rows are
    finished one by one (limit out of reach), then the limit of 0 sends the launch to the gated rectangular sweep."""
    check(monkeypatch, capfd, n, kind, {"PG_KNN_SYM_CAPL": "8", "PG_KNN_SYM_EVICT_LIMIT": "100000000"})
    check(monkeypatch, capfd, n, kind, {"PG_KNN_SYM_CAPL": "8", "PG_KNN_SYM_EVICT_LIMIT": "0"})


@pytest.mark.gpu
@pytest.mark.parametrize("piece", ["12", "3"])
@pytest.mark.parametrize("kind", ["strided256", "contiguous"])
def test_blocks_cut_into_two_and_seven_pieces(monkeypatch, capfd, kind, piece):
    """N = 3000: 24 super-tiles.  Pieces of 12 cut the first blocks' columns in 2, pieces of 3 the blocks with 21..23
    super-tiles in 7 (pg_knn_sym_plan; checked on the CPU in test_knn_sym_cpu.py)"""
    check(monkeypatch, capfd, 3000, kind, {"PG_KNN_SYM_PIECE": piece})
    check(monkeypatch, capfd, 1000, kind, {"PG_KNN_SYM_PIECE": "4"}, ks=(16,))


@pytest.mark.gpu
def test_the_forced_launch_is_the_symmetric_one(monkeypatch, capfd):
    """PG_KNN_SYM=1 takes the path (the planner's debug line names it); PG_KNN_SYM=0 and a window of the rows do not"""
    from prograph_amd import _native as nat
    tok, ref = case(1000, "strided64")
    monkeypatch.setenv("PG_ENGINE", "mfma")
    monkeypatch.setenv("PG_DEBUG_PLAN", "1")
    planes = nat.pack(torch.from_numpy(tok), bits=5)
    monkeypatch.setenv("PG_KNN_SYM", "1")
    nat.knn_graph(planes, planes, 16)
    torch.cuda.synchronize()
    assert "[pg plan sym] rows=1000" in capfd.readouterr().err
    idx, dist = nat.knn_graph(planes, planes, 16, row0=64, nrows=936)          # not a whole self graph: the rectangular path
    assert np.array_equal(idx.cpu().numpy(), ref[16][0][64:]) and np.array_equal(dist.cpu().numpy(), ref[16][1][64:])
    assert "[pg plan sym]" not in capfd.readouterr().err
    monkeypatch.setenv("PG_KNN_SYM", "0")
    nat.knn_graph(planes, planes, 16)
    torch.cuda.synchronize()
    assert "[pg plan sym]" not in capfd.readouterr().err
