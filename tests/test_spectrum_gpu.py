"""
GPU checks of the k-mer spectrum distance: the profile kernel (pg_spectrum_profile, prograph_amd/csrc/
pg_spectrum.hip) against the `collections.Counter` definition of tests/spectrum_testdata.py with equal fp16 bit patterns,
its flag word, the operator on device tensors against the operator on CPU tensors, and the routes of `build_graph` and
`search` against (a) the same calls on the reference profiles stored with `pg.embedding` under the plain metric and (b),
for Euclidean, an independent oracle on int64 squared distances.  Everything is compared bit for bit: the counts are
integers, and every fp32 sum the cosine tile routine forms from them is an integer below 2^24.
"""
import ctypes
import operator

import numpy as np
import pandas as pd
import pytest
import torch

from spectrum_testdata import COMPS, d2_of, eps_oracle, euclid_of, knn_oracle, profiles, sim_of

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
# (symbols, k, dims): D = 3; 16; 400; 9261 (odd: the last packed pair is half used); 32768; and three hashed widths
CASES = [(3, 1, 0), (4, 2, 0), (20, 2, 0), (21, 3, 0), (32, 3, 0), (20, 3, 64), (20, 5, 1024), (31, 6, 32768)]
N_ROWS = 300
SLICES = {1: 11, 2: 10, 5: 7, N_ROWS: 0}          # N -> first row of the (N, width) matrix cut from the 300 rows


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def _matrix(symbols, k, width, seed):
    """(300, width) uint8: row r has length {0, k-1, k, k+1, 63, 64, 65, 127, 128, 129, 2047, 2048}[r % 12] (at most the
    width); every fifth row has interior zeros; row 11 is one repeated letter at full width (the largest count, the most
    contended bucket), row 23 the last letter at full width (the highest bucket), row 35 the period (s, .., s, s - 1)
    (the bucket below it)."""
    rng = np.random.default_rng(seed)
    lens = [0, k - 1, k, k + 1, 63, 64, 65, 127, 128, 129, 2047, 2048]
    T = np.zeros((N_ROWS, width), dtype=np.uint8)
    for r in range(N_ROWS):
        l = min(lens[r % 12], width)
        T[r, :l] = rng.integers(1, symbols + 1, l)
        if r % 5 == 3 and l > 4:
            T[r, rng.integers(0, l, max(1, l // 10))] = 0
    T[11] = 1
    T[23] = symbols
    T[35] = np.tile([symbols] * (k - 1) + [symbols - 1], width // k + 1)[:width]
    return T


_REF = {}


def _case(symbols, k, dims, width=2048):
    key = (symbols, k, dims, width)
    if key not in _REF:
        T = _matrix(symbols, k, width, seed=symbols * 10 + k)
        want = profiles(T, k, symbols, dims)
        assert want.max() == width - k + 1 and want[0].sum() == 0 and want[1].sum() == 0
        if not dims:
            assert want[11, 0] == width - k + 1 and want[23, -1] == width - k + 1 and want[35, -2] > 0
        _REF[key] = (T, want.astype(np.float16).view(np.uint16))
        _REF[key][0].setflags(write=False)
        _REF[key][1].setflags(write=False)
    return _REF[key]


def _u16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _launch(nat, tok, k, symbols, dims, rows=None, ldo=None):
    """pg_spectrum_profile itself, into an (n, ldo) output filled with a sentinel and a flag word that is not 0."""
    lib, dev = nat.lib(), nat.device()
    D = lib.pg_spectrum_dims(k, symbols, dims)
    n = tok.shape[0] if rows is None else len(rows)
    ldo = D if ldo is None else ldo
    out = torch.full((n, ldo), SENTINEL, dtype=torch.float16, device=dev)
    flags = torch.full((1,), 77, dtype=torch.int32, device=dev)
    rows_t = None if rows is None else torch.as_tensor(np.asarray(rows), dtype=torch.int64, device=dev)
    ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    assert tok.is_cuda and tok.dtype == torch.uint8 and tok.stride(1) == 1
    rc = lib.pg_spectrum_profile(ptr(tok), n, tok.shape[1], tok.stride(0), ptr(rows_t), k, symbols, dims, ptr(out), ldo, ptr(flags),
                                 nat._stream())
    assert rc == 0, lib.pg_last_error()
    return out, int(flags.item()), D


@pytest.mark.parametrize("symbols,k,dims", CASES)
def test_kernel_equals_the_counter_reference(nat, symbols, k, dims):
    """N in {1, 2, 5, 300} through the wrapper; then a shuffled gather list, ld > l (a column slice at an odd byte offset
    of a wider matrix), and ldo > D (rows that start off and on a 16-byte boundary), where the bytes beyond D keep their
    sentinel."""
    T, want = _case(symbols, k, dims)
    dev = nat.device()
    Td = torch.tensor(T).to(dev)
    for n, r0 in SLICES.items():
        got, flags = nat.spectrum_profile(Td[r0:r0 + n], k, symbols, dims or None)
        assert got.shape == want[r0:r0 + n].shape and got.dtype == torch.float16 and got.is_cuda
        assert int(flags.item()) == 0
        assert np.array_equal(_u16(got), want[r0:r0 + n]), (n, r0)
    D = want.shape[1]
    perm = np.random.default_rng(5).permutation(N_ROWS)[:200]
    got, flags = nat.spectrum_profile(Td, k, symbols, dims or None, rows=perm)
    assert int(flags.item()) == 0 and np.array_equal(_u16(got), want[perm])
    wide = torch.full((N_ROWS, 2056), symbols, dtype=torch.uint8, device=dev)     # what lies beside the slice would count
    wide[:, 3:2051] = Td
    got, flags = nat.spectrum_profile(wide[:, 3:2051], k, symbols, dims or None)
    assert int(flags.item()) == 0 and np.array_equal(_u16(got), want)
    for ldo in (D + 3, (D + 7) // 8 * 8 + 8):
        out, flags, _ = _launch(nat, Td, k, symbols, dims, ldo=ldo)
        assert flags == 0 and np.array_equal(_u16(out[:, :D]), want), ldo
        assert bool((out[:, D:] == SENTINEL).all()), ldo
        out, flags, _ = _launch(nat, wide[:, 3:2051], k, symbols, dims, rows=perm, ldo=ldo)
        assert flags == 0 and np.array_equal(_u16(out[:, :D]), want[perm]) and bool((out[:, D:] == SENTINEL).all()), ldo


@pytest.mark.parametrize("symbols,k,dims", [(20, 3, 0), (4, 2, 0), (20, 5, 1024)])
def test_a_narrow_matrix(nat, symbols, k, dims):
    T, want = _case(symbols, k, dims, width=40)
    got, flags = nat.spectrum_profile(torch.tensor(T), k, symbols, dims or None)
    assert int(flags.item()) == 0 and np.array_equal(_u16(got), want)
    got, flags = nat.spectrum_profile(torch.tensor(T)[:, :37], k, symbols, dims or None)      # ld 40 > l 37
    assert np.array_equal(_u16(got), profiles(T[:, :37], k, symbols, dims).astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("symbols,k,dims", [(20, 3, 0), (20, 3, 64), (3, 1, 0)])
def test_flag_word(nat, symbols, k, dims):
    """One token of symbols + 1 in the last row sets the word; clean data leaves it at 0.  With the bad token the other
    rows' profiles are still right, and nothing outside the rows' D counts is touched."""
    T, want = _case(symbols, k, dims, width=40)
    D = want.shape[1]
    bad = T.copy()
    bad[-1, 17] = symbols + 1
    out, flags, _ = _launch(nat, torch.tensor(T).to(nat.device()), k, symbols, dims, ldo=D + 8)
    assert flags == 0
    out, flags, _ = _launch(nat, torch.from_numpy(bad).to(nat.device()), k, symbols, dims, ldo=D + 8)
    assert flags == 1
    assert np.array_equal(_u16(out[:-1, :D]), want[:-1]) and bool((out[:, D:] == SENTINEL).all())
    bad[-1, 17] = 255
    out, flags, _ = _launch(nat, torch.from_numpy(bad).to(nat.device()), k, symbols, dims, ldo=D + 8)
    assert flags == 1 and np.array_equal(_u16(out[:-1, :D]), want[:-1]) and bool((out[:, D:] == SENTINEL).all())
    from prograph_amd.distance import spectrum
    with pytest.raises(ValueError):
        spectrum(k=k, symbols=symbols, dims=dims or None).embed(torch.from_numpy(bad).to(nat.device()))


def _bits(t):
    t = t.detach().cpu().contiguous() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return (t.numpy() if isinstance(t, torch.Tensor) else t).view(np.int32)


def _varlen(n, lo, hi, symbols, seed):
    """(n, hi) int64 tokens: rows of lengths lo..hi over `symbols` letters, zero right-padded; a few repeated rows, two rows
    with the same k-mer multiset but different order, and one row shorter than any k used."""
    rng = np.random.default_rng(seed)
    T = np.zeros((n, hi), dtype=np.int64)
    for r in range(n):
        l = int(rng.integers(lo, hi + 1))
        T[r, :l] = rng.integers(1, symbols + 1, l)
    if n > 60:
        T[40], T[n - 9] = T[3], T[3]                                      # duplicates
        T[17] = 0
        T[17, :6] = [1, 2, 1, 1, 2, 2]                                    # with k = 2: {12, 21, 11, 12, 22}
        T[55] = 0
        T[55, :6] = [1, 1, 2, 2, 1, 2]                                    # {11, 12, 22, 21, 12}: the same multiset
    return T


@pytest.mark.parametrize("symbols,k,dims", [(4, 2, 0), (20, 3, 0), (20, 3, 256)])
def test_operator_on_device_equals_operator_on_cpu(nat, symbols, k, dims):
    from prograph_amd.distance import cosine, spectrum
    dev = nat.device()
    X, Y = _varlen(120, 5, 40, symbols, seed=1), _varlen(33, 1, 64, symbols, seed=2)
    Y[4, :40], Y[4, 40:] = X[9], 0
    px, py = profiles(X, k, symbols, dims), profiles(Y, k, symbols, dims)
    for T, p in ((X, px), (Y, py)):
        e = spectrum(k=k, symbols=symbols, dims=dims or None).embed(torch.from_numpy(T).to(dev))
        assert e.is_cuda and np.array_equal(_u16(e), p.astype(np.float16).view(np.uint16))
    for sim in (False, True):
        op = spectrum(k=k, symbols=symbols, dims=dims or None, metric="euclidean")
        got = op(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), similarity=sim)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == (33, 120)
        assert np.array_equal(_bits(got), _bits(op(torch.from_numpy(X), torch.from_numpy(Y), similarity=sim)))
        want = euclid_of(d2_of(px, py))
        assert np.array_equal(_bits(got), _bits(sim_of(want) if sim else want))
        op = spectrum(k=k, symbols=symbols, dims=dims or None)
        got = op(torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), similarity=sim)
        ref = cosine(torch.from_numpy(px).to(torch.float16).to(dev), torch.from_numpy(py).to(torch.float16).to(dev), similarity=sim)
        assert got.is_cuda and np.array_equal(_bits(got), _bits(ref))
    assert float(got[4, 9]) == 1.0                                        # the same sequence at two widths


# ---------------------------------------------------------------------------------------------------------------- graphs
ALPHABETS = {4: "ACGT", 20: "ACDEFGHIKLMNPQRSTVWY"}


def _strings(T, letters):
    lut = np.array([""] + list(letters))
    return ["".join(lut[r[r > 0]]) for r in T]


def _dataset(tmp_path_factory, name, T, letters):
    from prograph_amd import Prograph
    f = tmp_path_factory.mktemp("spectrum") / f"{name}.csv"
    pd.DataFrame({"Sequence": _strings(T, letters), "Fitness": np.random.default_rng(0).uniform(0, 1, len(T))}).to_csv(f)
    pg = Prograph(file=str(f), amino_acids=letters)
    assert np.array_equal(pg.tokenized, T[:, :pg.tokenized.shape[1]])
    return pg


@pytest.fixture(scope="module")
def small(nat, tmp_path_factory):
    """300 sequences of 5..40 letters over 4 letters; spectrum(k=2, symbols=4): D = 16 and many ties."""
    T = _varlen(300, 5, 40, 4, seed=11)
    pg = _dataset(tmp_path_factory, "small", T, ALPHABETS[4])
    P = profiles(T, 2, 4)
    pg.embedding(list(P.astype(np.float32)), "ref")
    return pg, T, {0: P}


@pytest.fixture(scope="module")
def protein(nat, tmp_path_factory):
    """300 sequences of 20..60 letters over 20 letters; k = 3, exact (D = 8000) and dims = 256."""
    T = _varlen(300, 20, 60, 20, seed=12)
    pg = _dataset(tmp_path_factory, "protein", T, ALPHABETS[20])
    P = {dims: profiles(T, 3, 20, dims) for dims in (0, 256)}
    pg.embedding(list(P[0].astype(np.float32)), "ref")
    pg.embedding(list(P[256].astype(np.float32)), "ref256")
    return pg, T, P


def _same_graph(a, b):
    from prograph_amd.graph import KNNGraph
    assert type(a) is type(b) and a.final and b.final and a.ncols == b.ncols and a.similarity == b.similarity
    if isinstance(a, KNNGraph):
        assert a.dist.dtype == torch.float32 and torch.equal(a.idx, b.idx) and np.array_equal(_bits(a.dist), _bits(b.dist))
    else:
        assert a.weights.dtype == torch.float32
        assert torch.equal(a.indptr, b.indptr) and torch.equal(a.indices, b.indices) and np.array_equal(_bits(a.weights), _bits(b.weights))


def _is_knn(g, idx, w):
    assert np.array_equal(g.idx.cpu().numpy(), idx) and np.array_equal(_bits(g.dist), _bits(w))


def _is_csr(g, want):
    assert np.array_equal(g.indptr.cpu().numpy(), want[0]) and np.array_equal(g.indices.cpu().numpy(), want[1])
    assert np.array_equal(_bits(g.weights), _bits(want[2]))


def _middle(block):
    """A threshold that splits the values of a block and is one of them (so that == has hits): the middle one of those
    strictly between 0 and the largest."""
    v = np.sort(block[(block > 0) & (block < block.max())])
    return float(v[len(v) // 2])


def _splitting_eps(P):
    d = euclid_of(d2_of(P, P))
    return d, _middle(d)


def _graph_checks(pg, P, op_of, ref_name):
    from prograph_amd.distance import cosine, euclidean
    plain = {"cosine": cosine, "euclidean": euclidean}
    d2 = d2_of(P, P)
    d, eps_e = _splitting_eps(P)
    for metric in ("cosine", "euclidean"):
        op = op_of(metric)
        block = op(torch.from_numpy(pg.tokenized), torch.from_numpy(pg.tokenized)).numpy()         # (CPU: the definition)
        eps = eps_e if metric == "euclidean" else _middle(block)
        for sim in (False, True):
            for k in (5, 70):
                g = pg.build_graph(distance=op, k=k, similarity=sim, output="csr")
                _same_graph(g, pg.build_graph(representation=ref_name, distance=plain[metric], k=k, similarity=sim, output="csr"))
                if metric == "euclidean":
                    _is_knn(g, *knn_oracle(d2, k, 1, similarity=sim))
            for comp in COMPS:
                g = pg.build_graph(distance=op, eps=eps, comp=comp, similarity=sim, output="csr")
                _same_graph(g, pg.build_graph(representation=ref_name, distance=plain[metric], eps=eps, comp=comp, similarity=sim,
                                              output="csr"))
                if metric == "euclidean":
                    _is_csr(g, eps_oracle(d, comp, eps, keep_zero=False, similarity=sim))
                if not sim:
                    assert 0 < g.nnz < len(P) * (len(P) - 1) or comp is operator.eq, comp          # the threshold splits
                    if comp is operator.eq:
                        assert g.nnz > 0
    return d2, d, eps_e


def test_graphs_of_the_small_alphabet(small):
    """k = 5, k = 70 (rounds), eps under the five comparators at a threshold that splits the values; both metrics, distances
    and similarities; equal profiles are dropped from eps graphs like duplicates and rank as ties to the lower column."""
    from prograph_amd.distance import spectrum
    pg, T, P = small
    d2, d, eps = _graph_checks(pg, P[0], lambda m: spectrum(k=2, symbols=4, metric=m), "ref_embedded")
    assert d2[17, 55] == 0 and not np.array_equal(T[17], T[55])                                    # equal multisets
    rows = pg.build_graph(distance=spectrum(k=2, symbols=4, metric="euclidean"), eps=eps)
    assert 55 not in rows[17][0] and 17 not in rows[55][0] and 40 not in rows[3][0]
    knn = pg.build_graph(distance=spectrum(k=2, symbols=4, metric="euclidean"), k=1)
    # rank 0 - the lowest column at distance 0 - is dropped: row 17 then starts with its equal 55, row 55 and the duplicate
    # 40 of row 3 with themselves
    assert knn[17][0][0] == 55 and knn[17][1][0] == 0 and knn[55][0][0] == 55 and knn[40][0][0] == 40 and knn[3][0][0] == 40


@pytest.mark.parametrize("dims", [0, 256])
def test_graphs_of_the_protein_alphabet(protein, dims):
    from prograph_amd.distance import spectrum
    pg, T, P = protein
    _graph_checks(pg, P[dims], lambda m: spectrum(k=3, symbols=20, dims=dims or None, metric=m), "ref256_embedded" if dims else "ref_embedded")


def test_subgraph_and_stored_graph(small):
    """`idxs=` with a boolean mask gives the sub-graph (columns relative to the selection); `store=` keeps the device graph, and
    `degree` / `dirichlet` on it equal the column path."""
    from prograph_amd.distance import euclidean, spectrum
    pg, T, P = small
    op = spectrum(k=2, symbols=4, metric="euclidean")
    mask = np.zeros(len(T), dtype=bool)
    mask[::3] = True
    mask[55] = True
    sub = np.nonzero(mask)[0]
    d2 = d2_of(P[0][sub], P[0][sub])
    g = pg.build_graph(distance=op, k=7, idxs=mask, output="csr")
    assert g.nrows == len(sub)
    _is_knn(g, *knn_oracle(d2, 7, 1))
    _same_graph(g, pg.build_graph(representation="ref_embedded", distance=euclidean, k=7, idxs=mask, output="csr"))
    _same_graph(g, pg.build_graph(distance=op, k=7, idxs=sub - len(T), output="csr"))              # positions from the end
    d, eps = _splitting_eps(P[0][sub])
    g = pg.build_graph(distance=op, eps=eps, idxs=mask, output="csr")
    _is_csr(g, eps_oracle(d, operator.le, eps, keep_zero=False))
    for args in (dict(k=6), dict(eps=_splitting_eps(P[0])[1])):
        tuples = pg.build_graph(distance=op, store="S", **args)
        assert pg._device_graph("S") is not None and pg.csr_graphs["S"].final
        pg.graph["S_host"] = list(tuples)                                  # the same rows, no device graph behind them
        assert pg._device_graph("S_host") is None
        assert np.array_equal(pg.degree("S", boolean_weights=True), pg.degree("S_host", boolean_weights=True))
        # weighted degrees: the device sums fp32 weights in fp64, the column path in the column's own arithmetic; a
        # row of nnz weights summed in fp32 is within nnz * 2^-24 * sum|w| of the exact sum
        nnz = np.array([len(c[0]) for c in tuples], dtype=np.float64)
        s = np.array([np.abs(np.asarray(c[1], dtype=np.float64)).sum() for c in tuples])
        assert np.all(np.abs(pg.degree("S").astype(np.float64) - pg.degree("S_host").astype(np.float64)) <= nnz * 2.0 ** -24 * s)
        assert np.isclose(pg.dirichlet("S"), pg.dirichlet("S_host"), rtol=1e-6, atol=0)


# ---------------------------------------------------------------------------------------------------------------- search
def _query_tokens(strings, letters):
    width = max(len(s) for s in strings)
    Q = np.zeros((len(strings), width), dtype=np.int64)
    for r, s in enumerate(strings):
        Q[r, :len(s)] = [letters.index(c) + 1 if c in letters else 0 for c in s]
    return Q


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_search(protein, metric):
    """Strings that are not in the dataset - one shorter than k, one longer than the dataset's width, one holding a letter
    outside the alphabet - and one that is: k = 3, k = 70, eps; rank 0 and d = 0 are kept."""
    from prograph_amd.distance import cosine, euclidean, spectrum
    from prograph_amd.graph import CSRGraph, KNNGraph
    pg, T, P = protein
    letters = ALPHABETS[20]
    rng = np.random.default_rng(21)
    data = _strings(T, letters)
    long = "".join(rng.choice(list(letters), 90))
    queries = ["AC", long, data[5][:10] + "XB" + data[5][10:], data[123], data[9][3:] + "WWW", "".join(rng.choice(list(letters), 33))]
    assert len(long) > pg.tokenized.shape[1] and all(q not in pg.seq_idxs for q in queries if q != data[123])
    Q = _query_tokens(queries, letters)
    plain = {"cosine": cosine, "euclidean": euclidean}[metric]
    for dims, ref_name in ((0, "ref_embedded"), (256, "ref256_embedded")):
        op = spectrum(k=3, symbols=20, dims=dims or None, metric=metric)
        pq = profiles(Q, 3, 20, dims)
        assert pq[0].sum() == 0
        d2 = d2_of(P[dims], pq)
        d = euclid_of(d2)
        qf = pq.astype(np.float32)
        for sim in (False, True):
            for k in (3, 70):
                g = pg.search(queries, k=k, distance=op, similarity=sim, output="csr")
                assert isinstance(g, KNNGraph) and g.first == 0
                _same_graph(g, pg.search(qf, k=k, distance=plain, representation=ref_name, similarity=sim, output="csr"))
                _same_graph(g, pg.search(Q, k=k, distance=op, similarity=sim, output="csr"))          # token arrays as they are
                if metric == "euclidean":
                    _is_knn(g, *knn_oracle(d2, k, 0, similarity=sim))
            assert int(g.idx[3, 0]) == 123 and float(g.dist[3, 0]) == (1.0 if sim else 0.0)
            eps = float(np.median(d)) if metric == "euclidean" else 0.9
            g = pg.search(queries, eps=eps, distance=op, similarity=sim, output="csr")
            assert isinstance(g, CSRGraph)
            _same_graph(g, pg.search(qf, eps=eps, distance=plain, representation=ref_name, similarity=sim, output="csr"))
            if metric == "euclidean":
                _is_csr(g, eps_oracle(d, operator.le, eps, keep_zero=True, similarity=sim))
                assert 0 < g.nnz < d.size
            assert 123 in g.to_tuples()[3][0]
        if metric == "euclidean":
            rows, dmin = pg.nearest_neighbour(queries, distance=op)
            want = knn_oracle(d2, 1, 0)[0][:, 0]
            assert list(rows.index) == list(pg.graph.index[want]) and dmin == 0
            rows, dmin = pg.nearest_neighbour(long, distance=op)
            assert list(rows.index) == [pg.graph.index[want[1]]] and dmin == d[1].min()


# ------------------------------------------------------------------------------------------------- refusals, fall-backs
def test_refusals_and_fall_backs(nat, small, tmp_path_factory):
    from prograph_amd.distance import cosine, euclidean, spectrum
    pg, T, P = small
    # a token above `symbols` in the dataset: the flag word sends the call to the generic path, where the operator raises
    letters = "ACDEFGHIKLMNPQRSTVWYB"
    bad = _dataset(tmp_path_factory, "bad", _varlen(60, 5, 30, 21, seed=4), letters)
    assert bad.tokenized.max() == 21
    with pytest.raises(ValueError):
        bad.build_graph(distance=spectrum(k=3, symbols=20), k=3)
    with pytest.raises(ValueError):
        bad.search("ACDEF", distance=spectrum(k=3, symbols=20), k=3)
    g = bad.build_graph(distance=spectrum(k=2, symbols=21), k=3, output="csr")
    assert g.final and g.nrows == 60
    with pytest.raises(TypeError):
        pg.build_graph(distance=spectrum(k=2, symbols=4), k=3, min_identity=0.5)
    with pytest.raises(TypeError):
        pg.search("ACGTAC", distance=spectrum(k=2, symbols=4), k=3, min_identity=0.5)
    # any other comp takes the generic path and gives the operator's values
    op = spectrum(k=2, symbols=4, metric="euclidean")
    t = pg.build_graph(distance=op, eps=3.0, comp=lambda a, b: a <= b)
    want = eps_oracle(euclid_of(d2_of(P[0], P[0])), operator.le, 3.0, keep_zero=False)
    assert isinstance(t, list) and all(np.array_equal(t[r][0], want[1][want[0][r]:want[0][r + 1]]) for r in range(len(t)))
    # the split of _build_graph_embed_f32 changed nothing for stored embeddings: the direct native calls
    x = torch.from_numpy(P[0]).to(torch.float16).to(nat.device())
    xc = nat.cosine_prep(x)
    g = pg.build_graph(representation="ref_embedded", distance=cosine, k=9, output="csr")
    idx, w = nat.cosine_knn(xc, xc, 9, first=1)
    assert torch.equal(g.idx, idx) and np.array_equal(_bits(g.dist), _bits(w))
    g = pg.build_graph(representation="ref_embedded", distance=euclidean, eps=2.5, comp=operator.lt, similarity=True, output="csr")
    ip, ix, w = nat.euclidean_eps(xc, xc, nat.CMP_LT, 1 / (1 + 2.5), similarity=True)
    assert torch.equal(g.indptr, ip) and torch.equal(g.indices, ix) and np.array_equal(_bits(g.weights), _bits(w))
    sub = np.arange(0, 300, 7)
    g = pg.build_graph(representation="ref_embedded", distance=euclidean, k=70, idxs=sub, output="csr")
    xs = nat.cosine_prep(x[torch.as_tensor(sub, device=x.device)])
    idx, w = nat.euclidean_knn(xs, xs, min(70, len(sub) - 1), first=1)
    assert torch.equal(g.idx, idx) and np.array_equal(_bits(g.dist), _bits(w))
