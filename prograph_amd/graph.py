"""
Result containers of the graph-construction path.

The reference hands back a Python list of N `(indices, weights)` tuples per graph
(prograph/prograph.py:751-753, :764) and stores it in a DataFrame column.  The HIP path
produces CSR / (N,k) arrays on the device; these classes keep that form (device resident,
no per-row Python objects) and materialise the reference's tuples only on request, as
zero-copy views into two host arrays.

Weights are Hamming distances (uint8 / int16 / float32; similarities are formed on the host) or fp16 Minkowski values
(distances or similarities as the kernels computed them: those are final and pass through unchanged).  `final=True`
marks weights of any dtype as final values in the same way - the fp32 cosine or Euclidean distances or similarities.
"""
import numpy as np
import torch

from . import _native


class CSRGraph:
    """epsilon-neighbourhood graph: indptr int64 [n+1], indices int32 [nnz], weights uint8|int16|int32|float32|float16 [nnz].
    final=True: the weights are final values (not Hamming distances) whatever their dtype.  Integer weights reach the
    analytics as float32, which is exact up to 2^24 (the int32 weights of alignments beyond 128 positions stay below 2^16)."""

    def __init__(self, indptr, indices, weights, ncols, similarity=False, row0=0, final=False):
        self.indptr, self.indices, self.weights = indptr, indices, weights
        self.ncols, self.similarity, self.row0 = int(ncols), bool(similarity), int(row0)
        self.final = bool(final)

    def _passes_through(self):
        return self.final or self.weights.dtype == torch.float16

    @property
    def nrows(self):
        return int(self.indptr.numel() - 1)

    @property
    def nnz(self):
        return int(self.indices.numel())

    def host(self):
        """(indptr, indices int64, weights) as numpy, weights in the reference's dtype:
        int64 Hamming distances, float32 similarities 1/(1+d) (hamming.py:38), or the fp16 Minkowski values as they are
        (minkowski.py:36-40)."""
        indptr = self.indptr.cpu().numpy()
        idx = self.indices.to(torch.int64).cpu().numpy()
        if self._passes_through():
            w = self.weights.cpu().numpy()
        elif self.similarity:
            w = (1 / (1 + self.weights.to(torch.int64))).cpu().numpy()
        else:
            w = self.weights.to(torch.int64).cpu().numpy()
        return indptr, idx, w

    def to_tuples(self):
        """list of N (np.int64 indices ascending, weights) — the reference's `Neighbours` format.
        Rows without neighbours get `(array([], int), array([], int))` (prograph.py:753); all such rows
        share ONE pair of zero-length arrays (nothing can be written into them), the others are
        views into the two host arrays."""
        indptr, idx, w = self.host()
        nothing = (np.array([], dtype=int), np.array([], dtype=int))
        a, b = indptr[:-1].tolist(), indptr[1:].tolist()
        return [(idx[i:j], w[i:j]) if j > i else nothing for i, j in zip(a, b)]

    def _w(self, boolean_weights):
        if boolean_weights:
            return None
        if self._passes_through():
            return self.weights.to(torch.float32)           # final values (Minkowski fp16: exact in float32)
        if self.similarity:
            return (1 / (1 + self.weights.to(torch.int64))).to(torch.float32)
        if self.weights.dtype not in (torch.uint8, torch.float32):
            return self.weights.to(torch.float32)          # int16 / int32 distances of long sequences: exact up to 2^24
        return self.weights

    def row_stats(self, f=None, boolean_weights=False, want=("deg",)):
        """Device reductions (pg_csr_row_stats): per row deg = sum w, sum_f = sum f[col], sum_wf = sum w f[col],
        self_w = weight of the row's own node in its list; per column col_sum = sum of the column's weights."""
        return _native.csr_row_stats(self.indptr, self.indices, self._w(boolean_weights), f=f, want=want,
                                     row0=self.row0, ncols=self.ncols)

    def degree(self, boolean_weights=False):
        """Out-degree per row as float32 (prograph.py:797-822) without touching Python tuples."""
        if boolean_weights:
            return (self.indptr[1:] - self.indptr[:-1]).to(torch.float32).cpu().numpy()
        return self.row_stats(want=("deg",))["deg"].to(torch.float32).cpu().numpy()

    def _degree_vector(self, st, mode):
        """The Laplacian's diagonal D as the reference builds it (prograph.py:887-896): out-degree = row
        sums kept in float32 (`degree()`), in-degree = column sums of the float32 adjacency."""
        if mode == "outdegree":
            return st["deg"].to(torch.float32).to(torch.float64)
        if mode == "indegree":
            return st["col_sum"][self.row0:self.row0 + self.nrows].to(torch.float32).to(torch.float64)
        raise ValueError("Not a valid degree mode.")

    def laplacian_diagonal(self, boolean_weights=False, mode="outdegree"):
        want = ("deg",) if mode == "outdegree" else ("col_sum",)
        if mode not in ("outdegree", "indegree"):
            raise ValueError("Not a valid degree mode.")
        return self._degree_vector(self.row_stats(boolean_weights=boolean_weights, want=want), mode).cpu().numpy()

    def dirichlet(self, f, boolean_weights=False, mode="outdegree"):
        """f^T L f with L = -A, diagonal OVERWRITTEN by D (`L.setdiag(D)`, prograph.py:887-896): a row's own
        node in its neighbour list (kNN with duplicated sequences) does not enter the off-diagonal sum.
        f = per-node values of the ROWS' nodes (square graph: nrows == ncols)."""
        if mode not in ("outdegree", "indegree"):
            raise ValueError("Not a valid degree mode.")
        fd = torch.as_tensor(np.asarray(f, dtype=np.float64).reshape(-1), device=self.indptr.device)
        want = ("deg", "sum_wf", "self_w") + (("col_sum",) if mode == "indegree" else ())
        st = self.row_stats(f=fd, boolean_weights=boolean_weights, want=want)
        fr = fd[self.row0:self.row0 + self.nrows]
        D = self._degree_vector(st, mode)
        off = st["sum_wf"] - st["self_w"] * fr                # sum over j != r of A_rj f_j
        return float((fr * (D * fr - off)).sum().item())

    def local_variance(self, f):
        """mean_j (f_r - f_j) over the row's neighbours (prograph.py:924-946); NaN for empty rows."""
        fd = torch.as_tensor(np.asarray(f, dtype=np.float64).reshape(-1), device=self.indptr.device)
        st = self.row_stats(f=fd, boolean_weights=True, want=("sum_f",))
        cnt = (self.indptr[1:] - self.indptr[:-1]).to(torch.float64)
        fr = fd[self.row0:self.row0 + self.nrows]
        out = torch.where(cnt > 0, fr - st["sum_f"] / cnt.clamp(min=1), torch.full_like(fr, float("nan")))
        return out.cpu().numpy()

    # ------------------------------------------------------------------ undirected graphs (pg_graph.hip)
    # An entry whose column is outside 0..ncols-1 is no edge (the rule of `row_stats`).  The results are ordinary CSRGraphs
    # on the device: `similarity`, `final` and the weight dtype carry over, the weights' bits are never changed.
    def _like(self, arrays, ncols, row0):
        return CSRGraph(*arrays, ncols, similarity=self.similarity, row0=row0, final=self.final)

    def sorted(self):
        """The same rows with each row's edges ascending by column; equal columns stay in storage order (a stable sort),
        weights travel with their entries, no-edge entries are dropped."""
        return self._like(_native.csr_sort_rows(self.indptr, self.indices, self.weights, self.ncols), self.ncols, self.row0)

    def transpose(self):
        """T with T.nrows = ncols, T.ncols = row0 + nrows, T.row0 = 0: row c of T lists (row0 + r, w) for every edge
        (r, c, w), in storage order - so T's rows are ascending by column and duplicates keep their order.  The reverse
        neighbour lists: of a `fit_alignment` graph "what does row c contain?", of `search` results "which queries hit
        this dataset row?".  Rectangular graphs and shards (`row0 != 0`) are legal.  Bitwise reproducible."""
        return self._like(_native.csr_transpose(self.indptr, self.indices, self.weights, self.ncols, row0=self.row0),
                          self.row0 + self.nrows, 0)

    def symmetrize(self, mode="union", combine="min"):
        """The undirected graph S of a square graph (`row0 == 0`, `nrows == ncols`; `ValueError` otherwise): rows ascending
        by column, each column at most once per row.  mode="union": (r, c) is in S iff (r, c) or (c, r) is an edge (the
        undirected kNN graph); "mutual": iff both are (the mutual-kNN graph).  S[r, c] is `combine` ("min" | "max") over
        the weights of all occurrences of (r, c) and (c, r); a self-loop is its own reverse.  "min", the default, lets the
        nearer of two distances win; graphs of raw SCORES (`local_alignment` and the like, built with similarity=False)
        want combine="max" - the container cannot know that larger is nearer.  Integers compare as integers, floats as
        floats; a NaN loses to a number, and of two NaNs or of -0 and +0 the smaller bit pattern wins, so S equals
        S.transpose() bit for bit."""
        if mode not in _native.SYM_MODES:
            raise ValueError("mode is 'union' or 'mutual'")
        if combine not in _native.SYM_COMBINES:
            raise ValueError("combine is 'min' or 'max'")
        if self.row0 != 0 or self.nrows != self.ncols:
            raise ValueError("symmetrize needs a square graph: row0 == 0 and nrows == ncols")
        return self._like(_native.csr_symmetrize(self.indptr, self.indices, self.weights, mode=mode, combine=combine), self.ncols, 0)

    def coords(self, boolean_weights=False):
        """(I, J, V) of prograph.py:824-857 straight from CSR."""
        indptr, idx, w = self.host()
        I = np.repeat(np.arange(self.nrows, dtype=int) + self.row0, np.diff(indptr))
        if boolean_weights:
            return I, idx, np.ones(I.shape)
        return I, idx, w.astype(np.float32)


class KNNGraph:
    """k nearest neighbours: idx int32 (n,k), dist uint8|int16|int32 (n,k) or fp16 Minkowski values; canonical (distance, index)
    order (descending values for Minkowski similarities).  final=True: the values are final (cosine / Euclidean fp32) whatever
    their dtype.  first: the rank of column 0 - 1 for self-graphs (rank 0 dropped, ranks beyond N-1 do not exist), 0 for
    query results (`Prograph.search`: rank 0 kept, min(k, N) ranks).  idx < 0: an empty slot, no edge (`host`, `to_tuples`
    and `as_csr` leave it out; `_without_empty_slots`)."""

    def __init__(self, idx, dist, ncols, similarity=False, row0=0, final=False, first=1):
        self.idx, self.dist = idx, dist
        self.ncols, self.similarity, self.row0 = int(ncols), bool(similarity), int(row0)
        self.final = bool(final)
        self.first = int(first)
        self._csr = None             # the CSR without the empty slots, once `_without_empty_slots` has looked

    @property
    def nrows(self):
        return int(self.idx.shape[0])

    def _ranks(self):
        return min(self.idx.shape[1], max(self.ncols - self.first, 0))   # ranks beyond N-1 do not exist ([:,1:k+1])

    def _without_empty_slots(self):
        """A slot with idx < 0 holds no neighbour (`rescore(k=)`: a row with fewer than k candidates) and is no edge for
        any consumer.  False when the ranks that exist are all filled - the usual table; one device reduction, made
        once -, else the CSRGraph of the filled slots: `indptr` from the per-row counts, order and weights as in the
        table."""
        if self._csr is None:
            kk = self._ranks()
            idx = self.idx[:, :kk]
            real = idx >= 0
            if not idx.numel() or bool(real.all()):
                self._csr = False
            else:
                indptr = torch.zeros(self.nrows + 1, dtype=torch.int64, device=idx.device)
                indptr[1:] = torch.cumsum(real.sum(dim=1), 0)
                self._csr = CSRGraph(indptr, idx[real], self.dist[:, :kk][real], self.ncols, similarity=self.similarity,
                                     row0=self.row0, final=self.final)
        return self._csr

    def host(self):
        """(idx int64, weights in the reference's dtype) as numpy, (n, ranks) each; a table with empty slots: two lists
        of n ragged rows without them (views into two flat arrays)."""
        g = self._without_empty_slots()
        if g:
            indptr, idx, w = g.host()
            return np.split(idx, indptr[1:-1]), np.split(w, indptr[1:-1])
        kk = self._ranks()
        idx = self.idx[:, :kk].to(torch.int64).cpu().numpy()
        if self.final or self.dist.dtype == torch.float16:
            return idx, self.dist[:, :kk].cpu().numpy()
        d = self.dist[:, :kk].to(torch.int64)
        w = (1 / (1 + d)).cpu().numpy() if self.similarity else d.cpu().numpy()
        return idx, w

    def to_tuples(self):
        idx, w = self.host()
        return list(zip(list(idx), list(w)))

    def as_csr(self):
        """The same graph as a CSRGraph: a view of the table (k entries per row; ranks beyond N-1 do not exist), or,
        where the table has empty slots, the CSR without them."""
        g = self._without_empty_slots()
        if g:
            return g
        kk = self._ranks()
        n = self.nrows
        indptr = torch.arange(0, n * kk + 1, kk, dtype=torch.int64, device=self.idx.device) if kk else \
            torch.zeros(n + 1, dtype=torch.int64, device=self.idx.device)
        return CSRGraph(indptr, self.idx[:, :kk].reshape(-1).contiguous(), self.dist[:, :kk].reshape(-1).contiguous(),
                        self.ncols, similarity=self.similarity, row0=self.row0, final=self.final)

    def sorted(self):
        """`as_csr().sorted()`: a CSRGraph, every row ascending by column."""
        return self.as_csr().sorted()

    def transpose(self):
        """`as_csr().transpose()`: the reverse-neighbour lists, a CSRGraph."""
        return self.as_csr().transpose()

    def symmetrize(self, mode="union", combine="min"):
        """`as_csr().symmetrize(...)`: the undirected (union) or mutual kNN graph, a CSRGraph."""
        return self.as_csr().symmetrize(mode=mode, combine=combine)


# ----------------------------------------------------------------------------------------------
# Persistence of device graphs without per-row Python objects.  The reference
# pickles the DataFrame, `Neighbours` column of N tuples included (prograph/utils/save.py:5-39);
# at N = 1M that is a million small arrays.  A graph is three flat arrays: they go into one .npz.
# ----------------------------------------------------------------------------------------------
def fingerprint(tokens):
    """64-bit fingerprint of a token matrix (shape + an order-sensitive checksum): what ties a graph side-car to the
    data it was built from."""
    t = np.ascontiguousarray(np.asarray(tokens)).astype(np.uint8, copy=False)
    h = np.uint64(1469598103934665603)
    with np.errstate(over="ignore"):
        w = (np.arange(1, t.shape[1] + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))[None, :] if t.ndim == 2 and t.size else np.zeros((1, 0), np.uint64)
        rows = (t.astype(np.uint64) * w).sum(axis=1) if t.size else np.zeros(0, np.uint64)
        idx = np.arange(1, len(rows) + 1, dtype=np.uint64) * np.uint64(0xBF58476D1CE4E5B9)
        h = h ^ np.uint64((rows * idx).sum()) ^ (np.uint64(t.shape[0]) << np.uint64(32)) ^ np.uint64(t.shape[1] if t.ndim == 2 else 0)
    return int(h)


def save_graphs(path, graphs, tokens_fingerprint=None):
    """{name: CSRGraph | KNNGraph} -> one .npz (arrays `<name>/indptr|indices|weights` or `<name>/idx|dist`
    plus a small meta vector [kind, ncols, similarity, row0, final]); `__fingerprint__` = fingerprint of the token matrix."""
    out = {}
    if tokens_fingerprint is not None:
        out["__fingerprint__"] = np.array([tokens_fingerprint], dtype=np.uint64)
    for name, g in graphs.items():
        if isinstance(g, KNNGraph):
            out[f"{name}/idx"] = g.idx.cpu().numpy()
            out[f"{name}/dist"] = g.dist.cpu().numpy()
            out[f"{name}/meta"] = np.array([1, g.ncols, int(g.similarity), g.row0, int(g.final)], dtype=np.int64)
        else:
            out[f"{name}/indptr"] = g.indptr.cpu().numpy()
            out[f"{name}/indices"] = g.indices.cpu().numpy()
            out[f"{name}/weights"] = g.weights.cpu().numpy()
            out[f"{name}/meta"] = np.array([0, g.ncols, int(g.similarity), g.row0, int(g.final)], dtype=np.int64)
    np.savez(path, **out)


def load_graphs(path, device=None, tokens_fingerprint=None):
    """Inverse of save_graphs (no pickled objects inside: plain arrays, `allow_pickle=False`).  With
    `tokens_fingerprint` a side-car written for other data (or by a version without fingerprints) yields nothing;
    graphs whose arrays are not a well-formed CSR / kNN table over `ncols` columns are skipped (device kernels index
    by these columns)."""
    device = _native.device() if device is None else device
    z = np.load(path, allow_pickle=False)
    graphs = {}
    if tokens_fingerprint is not None:
        if "__fingerprint__" not in z.files or int(z["__fingerprint__"][0]) != int(tokens_fingerprint):
            return graphs
    for key in z.files:
        if not key.endswith("/meta"):
            continue
        name = key[:-5]
        meta = [int(v) for v in z[key]]
        if len(meta) not in (4, 5):
            continue
        kind, ncols, sim, row0 = meta[:4]
        final = bool(meta[4]) if len(meta) == 5 else False           # side-cars written before `final` have 4 entries
        if kind == 1:
            idx = z[f"{name}/idx"]
            if idx.ndim != 2 or z[f"{name}/dist"].shape != idx.shape or (idx.size and (idx.min() < -1 or idx.max() >= ncols)):
                continue
        else:
            ip, ix = z[f"{name}/indptr"], z[f"{name}/indices"]
            if (ip.ndim != 1 or len(ip) < 1 or ip[0] != 0 or np.any(np.diff(ip) < 0) or int(ip[-1]) != len(ix)
                    or len(z[f"{name}/weights"]) != len(ix) or (len(ix) and (ix.min() < 0 or ix.max() >= ncols))):
                continue
        t = lambda a: torch.from_numpy(np.ascontiguousarray(z[f"{name}/{a}"])).to(device)
        if kind == 1:
            graphs[name] = KNNGraph(t("idx"), t("dist"), ncols, similarity=bool(sim), row0=row0, final=final)
        else:
            graphs[name] = CSRGraph(t("indptr"), t("indices"), t("weights"), ncols, similarity=bool(sim), row0=row0,
                                    final=final)
    return graphs
