"""
Profile (PSSM) queries (`distance.profile_alignment`) without a GPU.

tests/profile_testdata.py holds the yardstick: `definition`, the recurrence of each mode as a numpy double loop, and
`brute_force`, the worded definitions.  Here the two are held against each other and `definition` against the `definition`s
of the three sequence scores through sequence profiles; then the operator's torch expression on CPU tensors, its rules, the
two helpers, `search` and the queries-only errors are compared with `definition`.  The kernels are compared with it in
tests/test_profile_alignment_gpu.py.
"""
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import fake_native
import fit_testdata
import local_testdata
import semiglobal_testdata
from local_testdata import csr_of, knn_of, lengths, rows_of, score_table
from profile_testdata import MODES, brute_force, definition, random_profile
from prograph_amd import synth
from prograph_amd.distance import fit_alignment, local_alignment, profile_alignment, semiglobal_alignment

SEQUENCE = {"local": (local_testdata.definition, local_alignment), "semiglobal": (semiglobal_testdata.definition, semiglobal_alignment),
            "fit": (fit_testdata.definition, fit_alignment)}


# ---------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gap,gap_open", [(1, 0), (2, 3), (1, 4)])
def test_the_recurrence_is_the_worded_definition(mode, gap, gap_open):
    """Profiles of 1..4 positions over three symbols with entries -3..4, not derivable from a table, against rows of 0..4
    symbols (symbol 0 only inside a row)."""
    rng = np.random.default_rng(10 * gap + gap_open)
    profiles = [rng.integers(-3, 5, (l, 3)) for l in (1, 2, 3, 4, 4, 3)]
    rows = np.zeros((10, 4), dtype=np.int64)
    for r in range(10):
        l = r // 2
        rows[r, :l] = rng.integers(0, 3, l)
        if l:
            rows[r, l - 1] = rng.integers(1, 3)
    assert (rows[:, :3] == 0).any()
    D = definition(mode, profiles, gap, gap_open, rows)
    lens = lengths(rows)
    for q, P in enumerate(profiles):
        for c in range(10):
            assert D[q, c] == brute_force(mode, P, gap, gap_open, list(rows[c, :lens[c]])), (q, c)
    assert (D > 0).any() and ((D < 0).any() if mode == "fit" else (D >= 0).all())


@pytest.mark.parametrize("mode", MODES)
def test_a_sequence_profile_scores_what_the_sequence_scores(mode):
    """The defining equivalence on the yardsticks: P[j][a] = S[y_j][a] under a symmetric S gives the sequence score."""
    rng = np.random.default_rng(7)
    S = score_table(rng, 6, -5, 3, diag=[2, 4, 6])
    X = rows_of(rng, 6, rng.integers(0, 19, 14), 18, low=0)
    Y = rows_of(rng, 6, [1, 2, 5, 9, 17, 18, 3], 18, low=0)
    profiles = [profile_alignment.from_sequence(y, S) for y in Y]
    assert [len(p) for p in profiles] == list(lengths(Y)) and np.array_equal(profiles[2], S[Y[2, :5]])
    for gap, gap_open in ((1, 0), (2, 5)):
        assert np.array_equal(definition(mode, profiles, gap, gap_open, X), SEQUENCE[mode][0](S, gap, gap_open, X, Y))


# ---------------------------------------------------------------- the operator's rules
def test_constructor_and_profile_rules():
    op = profile_alignment("fit", 7, gap_open=11)
    assert op.mode == "fit" and op.gap == 7 and op.gap_open == 11
    assert repr(op) == "profile_alignment('fit', gap=7, gap_open=11)" and repr(profile_alignment("local", 2)) == "profile_alignment('local', gap=2)"
    for name in ("mode", "gap", "gap_open"):
        with pytest.raises(AttributeError):
            setattr(op, name, 3)
    for mode in ("global", "Fit", None, 2):
        with pytest.raises(ValueError, match="mode"):
            profile_alignment(mode, 1)
    for g in (0, 256, -1, 2.5, True, None, "3"):
        with pytest.raises(ValueError):
            profile_alignment("local", g)
    for o in (-1, 256, 2.5, True, None):
        with pytest.raises(ValueError):
            profile_alignment("local", 1, gap_open=o)
    X = torch.tensor([[1, 2, 0]])
    good = np.array([[0, 3, -1], [-2, 1, 4]])
    assert torch.equal(op(X, good), op(X, good, similarity=True)) and op(X, good).shape == (1, 1) and op(X, good).dtype == torch.int64
    assert torch.equal(op(X, good[None]), op(X, [good])) and torch.equal(op(X, torch.from_numpy(good)), op(X, good.astype(np.float64)))
    with pytest.raises(ValueError, match="similarity"):
        op(X, good, similarity=False)
    bad = [good[:, :1], np.zeros((2, 33), dtype=np.int64) + 1, good + 0.5, good.astype(bool), np.where(good == 4, 128, good),
           np.where(good == -2, -129, good), np.minimum(good, 0), good.reshape(-1), good[:0], np.ones((2049, 3), dtype=np.int64),
           [], [good, good[:, :2]], np.ones((1, 2, 2, 3), dtype=np.int64)]
    for P in bad:
        with pytest.raises(ValueError):
            op(X, P)
    op(X, np.ones((2048, 32), dtype=np.int64)[:, :3])             # the longest profile
    with pytest.raises(ValueError, match="profile_alignment"):
        op(torch.tensor([[1, 3]]), good)                          # a token outside the profile's symbols
    with pytest.raises(ValueError):
        op(torch.tensor([[0.5, 1]]), good)
    with pytest.raises(ValueError):
        op(X[:0], good)


# ---------------------------------------------------------------- the torch expression
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("a,gap,gap_open", [(21, 1, 0), (21, 3, 11), (32, 255, 255), (5, 2, 1)])
def test_operator_against_the_definition_on_cpu_tensors(mode, a, gap, gap_open):
    """Profiles of different lengths in one call, rows of every length with interior zeros, -128 and 127 among the
    entries."""
    rng = np.random.default_rng(100 * a + gap + gap_open)
    profiles = [random_profile(rng, l, a, -128 if a == 32 else -6, 127 if a == 32 else 9) for l in (1, 2, 16, 17, 40, 23)]
    X = rows_of(rng, a, list(range(0, 33)) + [40, 64], 64, low=0)
    want = definition(mode, profiles, gap, gap_open, X)
    op = profile_alignment(mode, gap, gap_open)
    assert np.array_equal(op(torch.from_numpy(X), profiles).numpy(), want)
    assert np.array_equal(op(torch.from_numpy(X.astype(np.uint8)), profiles[3]).numpy(), want[3:4])      # one (L, A) array
    same = np.stack([profiles[2], random_profile(rng, 16, a)])
    assert np.array_equal(op(torch.from_numpy(X), same).numpy(), definition(mode, list(same), gap, gap_open, X))
    assert (want > 0).any() and ((want < 0).any() if mode == "fit" else (want >= 0).all())


@pytest.mark.parametrize("mode", MODES)
def test_from_sequence_equals_the_sequence_operator_on_cpu(mode):
    rng = np.random.default_rng(11)
    S = score_table(rng, 21, -4, 2, diag=np.arange(3, 8))
    X = rows_of(rng, 21, rng.integers(0, 41, 30), 40)
    Y = rows_of(rng, 21, [1, 7, 16, 33, 40, 12], 40)
    Xt = torch.from_numpy(X)
    for gap, gap_open in ((1, 0), (3, 11)):
        got = profile_alignment(mode, gap, gap_open)(Xt, [profile_alignment.from_sequence(y, S) for y in Y])
        assert torch.equal(got, SEQUENCE[mode][1](S, gap, gap_open)(Xt, torch.from_numpy(Y)))
    for bad in (np.zeros(4, dtype=np.int64), np.array([1, 21]), np.array([1.5, 2])):
        with pytest.raises(ValueError):
            profile_alignment.from_sequence(bad, S)
    assert profile_alignment.from_sequence([3, 0, 5, 0, 0], S).shape == (3, 21)      # the interior zero stays, the padding goes


def test_from_aligned_on_a_hand_computed_case():
    """Three rows, two columns, symbols {0, 1, 2}, uniform background b = 1/2, pseudocount 1, scale 2.
    Column 0 holds 1, 1, 1: f1 = (3 + 1/2) / 4 = 7/8, f2 = (1/2) / 4 = 1/8; 2 log2(7/4) = 1.61.. -> 2, 2 log2(1/4) = -4.
    Column 1 holds 1, 2 and a skipped 0: f1 = f2 = (1 + 1/2) / 3 = 1/2; 2 log2(1) = 0.  Symbol 0 takes the column's minimum."""
    P = profile_alignment.from_aligned([[1, 1], [1, 2], [1, 0]], 3)
    assert P.dtype == np.int64 and np.array_equal(P, [[-4, 2, -4], [0, 0, 0]])
    # background 1 : 3, pseudocount 2, scale 1, column 0: f1 = (3 + 1/2) / 5 = 0.7, log2(0.7 / 0.25) = 1.49 -> 1;
    # f2 = (0 + 3/2) / 5 = 0.3, log2(0.3 / 0.75) = -1.32 -> -1
    P = profile_alignment.from_aligned(np.array([[1, 1], [1, 2], [1, 0]]), 3, background=[9, 1, 3], pseudocount=2.0, scale=1.0)
    assert np.array_equal(P[0], [-1, 1, -1])
    assert profile_alignment.from_aligned([[1] * 5] * 400, 2, pseudocount=1e-30, scale=100.0).max() == 0          # one symbol: f = b = 1
    assert profile_alignment.from_aligned([[1] * 5] * 400, 3, pseudocount=1e-30, scale=100.0).min() == -128       # clipped
    for kw in ({"rows": [[1, 3]], "symbols": 3}, {"rows": [[1, 2]], "symbols": 1}, {"rows": [[1, 2]], "symbols": 3, "pseudocount": 0},
               {"rows": [[1, 2]], "symbols": 3, "scale": -1}, {"rows": [[1, 2]], "symbols": 3, "background": [1, 0, 1]},
               {"rows": [1, 2], "symbols": 3}, {"rows": [[1, 2]], "symbols": 3, "background": [1, 1]}):
        with pytest.raises(ValueError):
            profile_alignment.from_aligned(**kw)
    fam = rows_of(np.random.default_rng(2), 21, [12] * 9, 12)
    pssm = profile_alignment.from_aligned(fam, 21)
    assert pssm.shape == (12, 21) and pssm.max() >= 1             # usable as a query as it is
    assert int(profile_alignment("fit", 2)(torch.from_numpy(fam[:1]), pssm)) == pssm[np.arange(12), fam[0]].sum()


# ---------------------------------------------------------------- search and the queries-only errors
N, L = 90, 24


@pytest.fixture()
def pg(tmp_path, monkeypatch):
    """A dataset on the stand-in of tests/fake_native.py (the constructor's Hamming graph needs one): it reports a CPU
    device, so `search` takes the operator's torch expression and the selection in torch."""
    fake_native.install(monkeypatch)
    from prograph_amd import Prograph
    tok, _ = synth.clustered_varlen_tokens(N, Lmax=L, Lmin=10, seed=5, members=9)
    f = tmp_path / "profiles.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    P = Prograph(file=str(f))
    assert np.array_equal(P.tokenized, tok)
    return P, tok


def _arrays(got):
    return np.array([np.asarray(i) for i, _ in got]), np.array([np.asarray(w) for _, w in got])


def _same_csr(got, ip, ix, w):
    assert len(got) == len(ip) - 1
    for i, (gi, gw) in enumerate(got):
        assert np.array_equal(gi, ix[ip[i]:ip[i + 1]]) and np.array_equal(gw, w[ip[i]:ip[i + 1]]), i


@pytest.mark.parametrize("mode", MODES)
def test_search_against_a_stable_descending_sort_of_the_definition(pg, mode):
    P, tok = pg
    rng = np.random.default_rng(3)
    profiles = [random_profile(rng, l, 21) for l in (5, 24, 9, 30)]
    profiles.append(profile_alignment.from_aligned(tok[:9, :20], 21))         # a family's PSSM among them
    op = profile_alignment(mode, 2, gap_open=3)
    D = definition(mode, profiles, 2, 3, tok)
    assert (D > 0).any() and (mode != "fit" or (D < 0).any())
    wi, wd = knn_of(D, 6, 0)
    gi, gw = _arrays(P.search(profiles, k=6, distance=op))
    assert np.array_equal(gi, wi) and np.array_equal(gw, wd)
    G = P.search(profiles, k=6, distance=op, output="csr", similarity=True)    # `similarity` is not consulted
    assert G.first == 0 and G.similarity is False and G.idx.dtype == torch.int32
    assert np.array_equal(G.idx.cpu().numpy(), wi) and np.array_equal(G.dist.cpu().numpy(), wd)
    gi, gw = _arrays(P.search(profiles[1], k=N + 5, distance=op))              # one (L, A) array; min(k, N) ranks
    assert gi.shape == (1, N) and np.array_equal(gw[0], knn_of(D[1:2], N, 0)[1][0])
    mid = int(np.median(D[D > 0]))
    for comp, eps in ((operator.le, mid), (operator.lt, mid - 0.5), (operator.eq, mid), (operator.ge, mid), (operator.gt, mid + 1),
                      (lambda a, b: a <= b, mid)):
        _same_csr(P.search(profiles, eps=eps, distance=op, comp=comp), *csr_of(D, comp, eps))
    G = P.search(profiles, eps=-1000, distance=op, output="csr")               # s >= -1000: every s > 0
    assert G.nnz == (D > 0).sum() and G.ncols == N
    stack = np.stack([profiles[1], random_profile(rng, 24, 21)])               # a (Q, L, A) array
    assert np.array_equal(_arrays(P.search(stack, k=3, distance=op))[1], knn_of(definition(mode, list(stack), 2, 3, tok), 3, 0)[1])
    with pytest.raises(ValueError):
        P.search(profiles, k=2, eps=3, distance=op)
    with pytest.raises(ValueError, match="profile"):
        P.search("ACDEF", k=2, distance=op)                                    # a string is no profile
    with pytest.raises(ValueError, match="profile_alignment"):
        P.search(random_profile(rng, 5, 20), k=2, distance=op)                 # the dataset has a token 20


def test_profiles_are_queries_only(pg):
    P, tok = pg
    op = profile_alignment("local", 2)
    prof = random_profile(np.random.default_rng(0), 8, 21)
    for call in (lambda: P.build_graph(k=3, distance=op), lambda: P.build_graph(eps=3, distance=op),
                 lambda: P.build_graph(k=3, distance=op, min_identity=0.5), lambda: P.search(prof, k=3, distance=op, min_identity=0.5),
                 lambda: P.search(prof, k=3, distance=op, min_columns=4), lambda: P.align(rows=[0], cols=[1], distance=op),
                 lambda: P.align(P.search(prof, k=2, distance=op, output="csr"), queries=prof, distance=op)):
        with pytest.raises(ValueError, match="queries only"):
            call()


def test_the_header_declares_what_the_binding_lists():
    import test_capi_symbols
    from prograph_amd import _native
    assert {"pg_alignment_profile_dense", "pg_alignment_profile_long_dense"} <= set(test_capi_symbols._declared()) & set(_native.SYMBOLS)
    assert sorted(_native.SYMBOLS) == test_capi_symbols._declared()
