"""
The graph operations `sorted`, `transpose`, `symmetrize` (pg_graph.hip) on the GPU, every case bit for bit against
the pure-Python model of tests/graph_ops_model.py.

- The raw entries (`pg_csr_sort_rows_count` / `_fill`, `pg_csr_histogram`, `pg_csr_transpose`, `pg_csr_symmetrize_count` / `_fill`
  with `pg_exclusive_scan` between them) on the edge lists of tests/csr_model.py - row lengths 0, 1, 63, 64, 65, 127, 128, 129 and
  600, a hub column named by every row from several lanes, repeated columns, `row0` 0 and 37, the same with no-edge entries - in
  all five weight dtypes, negative values, NaNs and both zeros among the floats.  Operands, outputs and workspaces lie in the
  middle of one allocation filled with a mark, each between guards, and the outputs have exactly the size the model says:
  whatever is written outside an output, or into an input, is seen.
- The seams of the sort's tiers, for the row sort and for the transpose alike: one graph whose rows have exactly 0, 1, 2, 63, 64,
  65, T2 - 1, T2, T2 + 1 and 70 000 entries, in an order in which neighbours fall into different tiers; its transpose has columns
  of exactly these in-degrees.  Transposed twice it is `sorted()`; transposed again from the same input the bytes are equal.
- Symmetrisation: both modes, both combines, on the same lists made square (self-loops absent, once and often), small graphs
  that can be read, an empty graph and one without entries; S equals S.transpose() as bytes; mutual is within sorted(G) is
  within union.
- End to end at N = 300, L = 16: the eps = 2 Hamming graph (symmetric, rows ascending) comes back unchanged from all four; the
  k = 4 kNN graph; the Dirichlet energy of the stored union graph; a cosine kNN graph and a local-alignment score graph.
- Bad arguments are refused before any launch.
"""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest
import torch

import csr_model as M
import graph_ops_model as G
from prograph_amd import _native, synth
from prograph_amd.graph import CSRGraph, KNNGraph

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

MARK = 0xA5
T1, T2 = 64, 4096                                # PG_GRAPH_T1, PG_GRAPH_T2 of prograph_amd/csrc/pg_graph.h
KINDS = {np.dtype(np.uint8): (1, 0), np.dtype(np.int16): (2, 1), np.dtype(np.int32): (4, 1), np.dtype(np.float16): (2, 2),
         np.dtype(np.float32): (4, 2)}


class Arena:
    """Arrays carved out of the middle of one device allocation of MARK bytes: 4096 bytes in front and behind, 256 between
    any two.  `check()` reads everything back: the bytes outside the carved arrays still hold the mark, the inputs what they
    held; the outputs are returned."""
    EDGE, GAP = 4096, 256

    def __init__(self):
        self.items, self.size = {}, self.EDGE

    def add(self, name, array, output=False):
        array = np.ascontiguousarray(array)
        self.items[name] = (self.size, array, output)
        self.size += -(-array.nbytes // self.GAP) * self.GAP + self.GAP
        return self

    def marked(self, name, shape, dtype):
        """An output (or a workspace) that starts as MARK bytes."""
        return self.add(name, np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, MARK, np.uint8).view(dtype).reshape(shape), True)

    def build(self):
        host = np.full(self.size + self.EDGE, MARK, dtype=np.uint8)
        for at, array, _ in self.items.values():
            host[at:at + array.nbytes] = array.reshape(-1).view(np.uint8)
        self.buf = torch.from_numpy(host).cuda()
        return self

    def ptr(self, name):
        return ctypes.c_void_p(self.buf.data_ptr() + self.items[name][0])

    def check(self):
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        outside = np.ones(len(host), dtype=bool)
        out = {}
        for name, (at, array, output) in self.items.items():
            outside[at:at + array.nbytes] = False
            now = host[at:at + array.nbytes].view(array.dtype).reshape(array.shape)
            if output:
                out[name] = now
            else:
                assert np.array_equal(now.view(np.uint8), array.view(np.uint8)), f"the input {name} was written"
        bad = np.flatnonzero(host[outside] != MARK)
        assert not len(bad), ("bytes outside the outputs were written", np.flatnonzero(outside)[bad[:8]],
                              {name: (at, array.nbytes) for name, (at, array, _) in self.items.items()})
        return out


def _ok(rc):
    assert rc == 0, _native.lib().pg_last_error()


def _scan(a, counts, n, indptr):
    _ok(_native.lib().pg_exclusive_scan(a.ptr(counts), n, a.ptr(indptr), a.ptr("scan"), _native._stream()))


def raw_sort(indptr, indices, w, ncols):
    """sorted() through the raw entries; the outputs hold exactly the number of edges."""
    lib, s = _native.lib(), _native._stream()
    nrows, nnz = len(indptr) - 1, len(indices)
    valid = int(((indices >= 0) & (indices < ncols)).sum())
    nbytes = int(lib.pg_csr_sort_workspace(nnz))
    assert nbytes == 8 * nnz
    a = (Arena().add("indptr", indptr).add("indices", indices).add("w", w).marked("counts", (nrows,), np.uint32)
         .marked("ws", (nbytes,), np.uint8).marked("scan", (int(lib.pg_scan_scratch_bytes(nrows)),), np.uint8)
         .marked("out_indptr", (nrows + 1,), np.int64).marked("out_idx", (valid,), np.int32).marked("out_w", (valid,), w.dtype).build())
    _ok(lib.pg_csr_sort_rows_count(a.ptr("indptr"), a.ptr("indices"), nrows, nnz, ncols, a.ptr("counts"), a.ptr("ws"), nbytes, s))
    _scan(a, "counts", nrows, "out_indptr")
    _ok(lib.pg_csr_sort_rows_fill(a.ptr("indptr"), a.ptr("w"), w.dtype.itemsize, nrows, nnz, a.ptr("counts"), a.ptr("out_indptr"),
                                  a.ptr("out_idx"), a.ptr("out_w"), a.ptr("ws"), nbytes, s))
    out = a.check()
    return out["out_indptr"], out["out_idx"], out["out_w"]


def raw_transpose(indptr, indices, w, ncols, row0):
    lib, s = _native.lib(), _native._stream()
    nrows, nnz = len(indptr) - 1, len(indices)
    valid = int(((indices >= 0) & (indices < ncols)).sum())
    nbytes = int(lib.pg_csr_transpose_workspace(nnz, ncols))
    assert nbytes == 8 * nnz + 4 * ncols
    a = (Arena().add("indptr", indptr).add("indices", indices).add("w", w).marked("counts", (ncols,), np.uint32)
         .marked("ws", (nbytes,), np.uint8).marked("scan", (int(lib.pg_scan_scratch_bytes(ncols)),), np.uint8)
         .marked("t_indptr", (ncols + 1,), np.int64).marked("t_idx", (valid,), np.int32).marked("t_w", (valid,), w.dtype).build())
    _ok(lib.pg_csr_histogram(a.ptr("indices"), nnz, ncols, a.ptr("counts"), s))
    _scan(a, "counts", ncols, "t_indptr")
    _ok(lib.pg_csr_transpose(a.ptr("indptr"), a.ptr("indices"), a.ptr("w"), w.dtype.itemsize, nrows, nnz, ncols, row0,
                             a.ptr("t_indptr"), a.ptr("t_idx"), a.ptr("t_w"), a.ptr("ws"), nbytes, s))
    out = a.check()
    return out["t_indptr"], out["t_idx"], out["t_w"]


def raw_symmetrize(A, Tr, n, mode, combine, nnz_out):
    """The count and fill entries on A = sorted(G), Tr = transpose(G) (host arrays, from the model); outputs of nnz_out entries."""
    lib, s = _native.lib(), _native._stream()
    eb, kind = KINDS[A[2].dtype]
    na, nt = len(A[1]), len(Tr[1])
    nbytes = int(lib.pg_csr_symmetrize_workspace(na, nt))
    assert nbytes == 10 * (na + nt)
    a = (Arena().add("a_indptr", A[0]).add("a_idx", A[1]).add("a_w", A[2]).add("t_indptr", Tr[0]).add("t_idx", Tr[1]).add("t_w", Tr[2])
         .marked("counts", (n,), np.uint32).marked("ws", (nbytes,), np.uint8).marked("scan", (int(lib.pg_scan_scratch_bytes(n)),), np.uint8)
         .marked("out_indptr", (n + 1,), np.int64).marked("out_idx", (nnz_out,), np.int32).marked("out_w", (nnz_out,), A[2].dtype).build())
    _ok(lib.pg_csr_symmetrize_count(a.ptr("a_indptr"), a.ptr("a_idx"), a.ptr("a_w"), na, a.ptr("t_indptr"), a.ptr("t_idx"), a.ptr("t_w"),
                                    nt, eb, kind, _native.SYM_MODES[mode], _native.SYM_COMBINES[combine], n, a.ptr("counts"),
                                    a.ptr("ws"), nbytes, s))
    _scan(a, "counts", n, "out_indptr")
    _ok(lib.pg_csr_symmetrize_fill(a.ptr("a_indptr"), na, a.ptr("t_indptr"), nt, eb, n, a.ptr("out_indptr"), a.ptr("out_idx"),
                                   a.ptr("out_w"), a.ptr("ws"), nbytes, s))
    out = a.check()
    return out["out_indptr"], out["out_idx"], out["out_w"]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(triple):
    return tuple(t.cpu().numpy() for t in triple)


def graph_arrays(g):
    return host((g.indptr, g.indices, g.weights))


# ---------------------------------------------------------------- the edge lists of the CSR kernels' tests
@functools.lru_cache(maxsize=None)
def _lists(nrows, row0, negative):
    indptr, indices = M.edge_lists(nrows, row0, M.SEED[nrows])
    return indptr, (M.with_negative_columns(indptr, indices) if negative else indices)


@pytest.mark.parametrize("negative", [False, True], ids=["edges", "negative_columns"])
@pytest.mark.parametrize("nrows, row0", [(n, r0) for n in M.NROWS for r0 in M.ROW0])
def test_sort_and_transpose_equal_the_model_on_the_edge_lists(nrows, row0, negative):
    indptr, indices = _lists(nrows, row0, negative)
    if nrows == 19:
        lens = np.diff(indptr)
        assert set(lens) == set(M.LENGTHS) and (indices == M.HOT).sum() > 300          # the lists are what they claim
    for dtype in G.DTYPES:
        w = G.weights_of(dtype, len(indices), nrows)
        if np.dtype(dtype).kind == "f" and len(w) > 100:
            assert np.isnan(w).any() and (w < 0).any() and np.signbit(w[w == 0]).any() and not np.signbit(w[w == 0]).all()
        G.same(raw_sort(indptr, indices, w, M.NCOLS), G.sorted_rows(indptr, indices, w, M.NCOLS))
        G.same(raw_transpose(indptr, indices, w, M.NCOLS, row0), G.transpose(indptr, indices, w, M.NCOLS, row0))
    # columns at or past ncols are no edges either; the wrappers on the same lists
    w = G.weights_of(np.float16, len(indices), nrows)
    G.same(raw_transpose(indptr, indices, w, 100, row0), G.transpose(indptr, indices, w, 100, row0))
    G.same(raw_sort(indptr, indices, w, 100), G.sorted_rows(indptr, indices, w, 100))
    G.same(host(_native.csr_sort_rows(dev(indptr), dev(indices), dev(w), M.NCOLS)), G.sorted_rows(indptr, indices, w, M.NCOLS))
    G.same(host(_native.csr_transpose(dev(indptr), dev(indices), dev(w), M.NCOLS, row0=row0)), G.transpose(indptr, indices, w, M.NCOLS, row0))


# ---------------------------------------------------------------- the seams of the tiers
SEAM_LENGTHS = (T2 + 1, 1, T1, T2 - 1, 0, T1 + 1, 70_000, 2, T2, T1 - 1)      # neighbours in different tiers
SEAM_COLS = 4500


@functools.lru_cache(maxsize=None)
def _seam_graph():
    """Rows of exactly SEAM_LENGTHS entries over 4500 columns: random columns, so they repeat within the long rows; every entry
    an edge, so the transpose has 10 columns of exactly these in-degrees."""
    rng = np.random.default_rng(21)
    indptr = np.concatenate([[0], np.cumsum(SEAM_LENGTHS)]).astype(np.int64)
    indices = rng.integers(0, SEAM_COLS, int(indptr[-1])).astype(np.int32)
    w = rng.integers(-30000, 30000, len(indices)).astype(np.int16)
    return indptr, indices, w, G.sorted_rows(indptr, indices, w, SEAM_COLS), G.transpose(indptr, indices, w, SEAM_COLS)


def test_the_row_sort_at_the_seams_of_its_tiers():
    indptr, indices, w, want, _ = _seam_graph()
    assert sorted(np.diff(indptr)) == sorted(SEAM_LENGTHS)
    G.same(raw_sort(indptr, indices, w, SEAM_COLS), want)


def test_the_transpose_at_the_seams_of_its_tiers_twice_is_sorted_and_reproducible():
    indptr, indices, w, want_sorted, want_t = _seam_graph()
    t = raw_transpose(indptr, indices, w, SEAM_COLS, 0)
    G.same(t, want_t)                                                        # 4500 short segments
    assert sorted(np.bincount(t[1], minlength=len(indptr) - 1).tolist()) == sorted(SEAM_LENGTHS)   # the in-degrees of its columns
    back = raw_transpose(*t, len(indptr) - 1, 0)                             # 10 segments of exactly the seam lengths
    G.same(back, want_sorted)
    again = raw_transpose(indptr, indices, w, SEAM_COLS, 0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(t, again))
    g = CSRGraph(dev(indptr), dev(indices), dev(w), SEAM_COLS)
    G.same(graph_arrays(g.transpose().transpose()), graph_arrays(g.sorted()))
    G.same(graph_arrays(g.sorted()), want_sorted)


# ---------------------------------------------------------------- symmetrise
def _pairs(triple):
    rows = np.repeat(np.arange(len(triple[0]) - 1), np.diff(triple[0]))
    return set(zip(rows.tolist(), triple[1].tolist()))


@pytest.mark.parametrize("negative", [False, True], ids=["edges", "negative_columns"])
@pytest.mark.parametrize("nrows", M.NROWS)
def test_symmetrize_equals_the_model_on_the_square_lists(nrows, negative):
    indptr, indices = G.square_lists(nrows, negative)
    rows = np.repeat(np.arange(nrows), np.diff(indptr))
    if nrows == 19:
        loops = np.bincount(rows[indices == rows], minlength=nrows)
        assert (loops == 0).any() and (loops >= 2).any()                       # once: the graphs small enough to read
    for dtype in G.DTYPES:
        w = G.weights_of(dtype, len(indices), nrows)
        A, Tr = G.sorted_rows(indptr, indices, w, nrows), G.transpose(indptr, indices, w, nrows)
        got = {}
        for mode in ("union", "mutual"):
            for combine in ("min", "max"):
                want = G.symmetrize(indptr, indices, w, mode, combine)
                got[mode, combine] = raw_symmetrize(A, Tr, nrows, mode, combine, len(want[1]))
                G.same(got[mode, combine], want)
        assert _pairs(got["mutual", "min"]) <= _pairs(A) <= _pairs(got["union", "min"])
        # the wrapper (its own sort and transpose, untrimmed) and the container; S equals S.transpose() as bytes
        g = CSRGraph(dev(indptr), dev(indices), dev(w), nrows)
        for (mode, combine), want in got.items():
            s = g.symmetrize(mode, combine)
            G.same(graph_arrays(s), want)
            G.same(graph_arrays(s.transpose()), want)
            G.same(graph_arrays(s.sorted()), want)


def test_symmetrize_on_graphs_small_enough_to_read():
    # 0 -> 1 (5), 1 -> 0 (3) and (8): an asymmetric pair; 0 -> 2 (7): one direction only; 2 -> 2 (4) and (9): a self-loop twice
    indptr = np.array([0, 3, 5, 7], dtype=np.int64)
    indices = np.array([2, -1, 1, 0, 0, 2, 2], dtype=np.int32)
    for dtype in G.DTYPES:
        w = np.array([7, 99, 5, 3, 8, 4, 9]).astype(dtype)
        g = CSRGraph(dev(indptr), dev(indices), dev(w), 3)
        u, m = graph_arrays(g.symmetrize("union")), graph_arrays(g.symmetrize("mutual", combine="max"))
        G.same(u, (np.array([0, 2, 3, 5]), np.array([1, 2, 0, 0, 2], np.int32), np.array([3, 7, 3, 7, 4]).astype(dtype)))
        G.same(m, (np.array([0, 1, 2, 3]), np.array([1, 0, 2], np.int32), np.array([8, 8, 9]).astype(dtype)))
    # NaN against a number, -0 against +0, two NaNs: both directions get the same bits
    bits = np.array([0x7FC00000, 0x3F800000, 0x80000000, 0x00000000, 0xFFC00000, 0x7FC00001], dtype=np.uint32).view(np.float32)
    indptr = np.array([0, 1, 2, 3, 4, 5, 6], dtype=np.int64)
    indices = np.array([1, 0, 3, 2, 5, 4], dtype=np.int32)
    g = CSRGraph(dev(indptr), dev(indices), dev(bits), 6)
    for combine in ("min", "max"):
        s = graph_arrays(g.symmetrize("mutual", combine=combine))
        assert s[2].view(np.uint32).tolist() == [0x3F800000, 0x3F800000, 0, 0, 0x7FC00001, 0x7FC00001], combine
        G.same(s, G.symmetrize(indptr, indices, bits, "mutual", combine))


def test_empty_graphs_come_back_empty():
    none = CSRGraph(torch.zeros(1, dtype=torch.int64).cuda(), torch.zeros(0, dtype=torch.int32).cuda(), torch.zeros(0, dtype=torch.uint8).cuda(), 0)
    bare = CSRGraph(torch.zeros(6, dtype=torch.int64).cuda(), torch.zeros(0, dtype=torch.int32).cuda(), torch.zeros(0, dtype=torch.float16).cuda(), 5)
    slots = KNNGraph(torch.full((5, 3), -1, dtype=torch.int32).cuda(), torch.zeros((5, 3), dtype=torch.int16).cuda(), 5)
    for g, n in ((none, 0), (bare, 5), (slots, 5)):
        for out in (g.sorted(), g.transpose(), g.symmetrize("union"), g.symmetrize("mutual", combine="max")):
            assert (out.nrows, out.ncols, out.nnz) == (n, n, 0) and out.indptr.cpu().tolist() == [0] * (n + 1)
            assert out.weights.dtype == (g.dist if isinstance(g, KNNGraph) else g.weights).dtype and out.indices.dtype == torch.int32
    # a table of empty slots only, as -1 entries of a CSR, through the raw entries
    indptr, indices, w = np.arange(0, 5 * 70 + 1, 70, dtype=np.int64), np.full(350, -1, np.int32), np.full(350, 3, np.uint8)
    empty = (np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint8))
    G.same(raw_sort(indptr, indices, w, 5), empty)
    G.same(raw_transpose(indptr, indices, w, 5, 0), empty)


# ---------------------------------------------------------------- end to end, N = 300, L = 16
N, L, A = 300, 16, 21


@functools.lru_cache(maxsize=None)
def _tokens():
    return synth.clustered_tokens(N, L, seed=7, members=20)


def _knn_arrays(K):
    """(indptr, indices int32, weights in the table's dtype) from `host()`."""
    idx, w = K.host()
    idx, w = np.asarray(idx), np.asarray(w)
    assert idx.shape == (K.nrows, idx.shape[1]) and (idx >= 0).all()
    indptr = np.arange(0, idx.size + 1, idx.shape[1], dtype=np.int64)
    return indptr, idx.reshape(-1).astype(np.int32), w.reshape(-1).astype(K.dist.cpu().numpy().dtype)


def test_a_symmetric_eps_graph_comes_back_unchanged():
    planes = _native.pack(torch.from_numpy(_tokens()), bits=5)
    e = CSRGraph(*_native.eps_graph(planes, planes, _native.CMP_LE, 2, cap=32), N)
    src = graph_arrays(e)
    assert len(src[1]) > 2 * N and _pairs(src) == {(c, r) for r, c in _pairs(src)}
    for out in (e.transpose(), e.sorted(), e.symmetrize("union"), e.symmetrize("mutual"), e.symmetrize("union", combine="max")):
        G.same(graph_arrays(out), src)


def test_the_knn_graph_symmetrised_equals_the_model():
    planes = _native.pack(torch.from_numpy(_tokens()), bits=5)
    K = KNNGraph(*_native.knn_graph(planes, planes, 4), N)
    src = _knn_arrays(K)
    u, m = K.symmetrize("union"), K.symmetrize("mutual")
    G.same(graph_arrays(u), G.symmetrize(*src, "union", "min"))
    G.same(graph_arrays(m), G.symmetrize(*src, "mutual", "min"))
    G.same(graph_arrays(K.transpose()), G.transpose(*src, N))
    G.same(graph_arrays(K.sorted()), G.sorted_rows(*src, N))
    assert m.nnz < 4 * N < u.nnz                                            # a kNN graph is directed


def _prograph(tmp_path):
    from prograph_amd import Prograph
    f = tmp_path / "ops.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(_tokens()), "Fitness": M.exact_values(N)}).to_csv(f)
    P = Prograph(file=str(f))
    P.graph["Fitness"] = M.exact_values(N)                                  # the file's decimal digits need not parse back to the bits
    assert np.array_equal(P.tokenized, _tokens()) and np.array_equal(P("Fitness").to_numpy(), M.exact_values(N))
    return P


def test_the_dirichlet_energy_of_the_stored_union_graph_is_the_smoothness_functional(tmp_path):
    """f: multiples of 2^-20 in [0, 1), weights: Hamming distances up to 16.  A term f_i (D_i f_i - sum_j w_ij f_j) is a multiple of
    2^-40; the sum of the terms' magnitudes is checked to stay below 2^13, so every partial sum of the device's float64 reduction,
    in any order, has at most 53 bits and is exact.  The energy is then half the sum of w (f_i - f_j)^2 over the stored entries
    plus w_ii f_i^2 for a self-loop (the Laplacian's diagonal is overwritten by the degree, which counts the loop), evaluated
    here in integers: equality."""
    P = _prograph(tmp_path)
    P.build_graph(k=4, store="K")
    for mode, combine in (("union", "min"), ("mutual", "max")):
        S = P.symmetrize("K", mode=mode, combine=combine, store="U")
        assert P._device_graph("U") is S and S.nnz > N
        indptr, idx, w = S.host()
        G.same((indptr, idx.astype(np.int32), w.astype(np.uint8)), G.symmetrize(*_knn_arrays(P.csr_graphs["K"]), mode, combine))
        F = [int(v) for v in np.round(M.exact_values(N) * (1 << 20))]
        rows = np.repeat(np.arange(N), np.diff(indptr)).tolist()
        total = sum(int(wt) * (F[r] - F[c]) ** 2 + (2 * int(wt) * F[r] ** 2 if r == c else 0) for r, c, wt in zip(rows, idx.tolist(), w.tolist()))
        deg = np.zeros(N, dtype=np.int64)
        np.add.at(deg, rows, w)
        off = np.zeros(N, dtype=np.int64)
        np.add.at(off, rows, w * np.array(F)[idx])
        magnitudes = sum(abs(F[i] * (int(deg[i]) * F[i] - int(off[i]))) for i in range(N))
        assert magnitudes < (1 << 13) << 40, magnitudes / 2.0 ** 40
        got = float(np.asarray(P.dirichlet("U", scaler=None)).reshape(-1)[0])
        print(f"\n{mode}: dirichlet {got!r}, model {total / 2.0 ** 41!r}")
        assert Fraction(got) == Fraction(total, 1 << 41)
        m = M.analytics(indptr, idx, w.astype(np.float64), M.exact_values(N), N)
        assert np.array_equal(P.degree("U"), m["degree"]) and got == m["dirichlet"]["outdegree"]


def _score_table(seed):
    rng = np.random.default_rng(seed)
    S = rng.integers(-4, 2, (A, A))
    S = np.triu(S) + np.triu(S, 1).T
    S[np.arange(A), np.arange(A)] = rng.integers(2, 6, A)
    return S


def test_a_cosine_and_a_local_alignment_knn_graph(tmp_path):
    from prograph_amd.distance import cosine, local_alignment
    P = _prograph(tmp_path)
    rng = np.random.default_rng(12)
    P.graph["Embedded"] = list((rng.normal(0, 1, (5, 24))[np.arange(N) % 5] + rng.normal(0, 0.3, (N, 24))).astype(np.float32))
    C = P.build_graph(k=4, distance=cosine, representation="Embedded", output="csr")
    assert isinstance(C, KNNGraph) and C.dist.dtype == torch.float32 and C.final
    S = P.build_graph(k=4, distance=local_alignment(_score_table(3), 3, gap_open=2), output="csr")
    assert isinstance(S, KNNGraph) and S.dist.dtype in (torch.int16, torch.int32) and not S.similarity
    for K, combine in ((C, "min"), (S, "max")):
        src = _knn_arrays(K)
        for mode in ("union", "mutual"):
            s = K.symmetrize(mode, combine=combine)
            assert (s.final, s.similarity, s.weights.dtype) == (K.final, K.similarity, K.dist.dtype)
            G.same(graph_arrays(s), G.symmetrize(*src, mode, combine))
            G.same(graph_arrays(s.transpose()), graph_arrays(s))
        G.same(graph_arrays(K.transpose()), G.transpose(*src, N))


# ---------------------------------------------------------------- bad arguments
def test_bad_arguments_return_before_any_launch():
    lib, s = _native.lib(), _native._stream()
    p = ctypes.c_void_p(4096)                                               # never dereferenced
    assert lib.pg_csr_sort_rows_count(p, p, 4, 10, 4, p, p, 79, s) == -1
    assert lib.pg_csr_sort_rows_count(None, p, 4, 10, 4, p, p, 80, s) == -1
    assert lib.pg_csr_sort_rows_fill(p, p, 3, 4, 10, p, p, p, p, p, 80, s) == -1
    assert lib.pg_csr_histogram(p, -1, 4, p, s) == -1 and lib.pg_csr_histogram(None, 10, 4, p, s) == -1
    assert lib.pg_csr_transpose(p, p, p, 2, 4, 10, 4, -1, p, p, p, p, 96, s) == -1
    assert lib.pg_csr_transpose(p, p, p, 2, 4, 10, 4, 0, p, p, p, p, 95, s) == -1
    assert lib.pg_csr_transpose(p, p, p, 8, 4, 10, 4, 0, p, p, p, p, 96, s) == -1
    for eb, kind, mode, combine, nbytes in ((3, 0, 0, 0, 200), (1, 2, 0, 0, 200), (4, 3, 0, 0, 200), (4, 2, 2, 0, 200), (4, 2, 0, 2, 200),
                                            (4, 2, 0, 0, 199)):
        assert lib.pg_csr_symmetrize_count(p, p, p, 10, p, p, p, 10, eb, kind, mode, combine, 4, p, p, nbytes, s) == -1
        assert b"pg_csr_symmetrize_count" in lib.pg_last_error()
    assert lib.pg_csr_symmetrize_fill(p, 10, p, 10, 4, 4, p, p, p, None, 200, s) == -1
    torch.cuda.synchronize()
    g = CSRGraph(torch.zeros(4, dtype=torch.int64).cuda(), torch.zeros(0, dtype=torch.int32).cuda(), torch.zeros(0).cuda(), 5)
    with pytest.raises(ValueError):
        g.symmetrize()
    with pytest.raises(TypeError):
        _native.csr_sort_rows(g.indptr, g.indices, torch.zeros(0, dtype=torch.float64).cuda(), 5)
