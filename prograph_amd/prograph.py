"""
`Prograph` — host-side mirror of the reference's class (prograph/prograph.py of
acmater/prograph) with the graph-construction hot path running on hand-written HIP kernels.

Same constructor, same methods, same return conventions, so code written against the
reference keeps working; what changed is *where the work happens*:

  reference (prograph/prograph.py)                     here
  -----------------------------------------------      ------------------------------------
  :726  list-of-arrays -> fp16 tensor on cuda:0        int8 plane layout, packed on device once
  :731-739 batches of 8: broadcast !=, sum, where,     one `pg_eps_slots` launch + scan +
           3 D->H copies and a sync per batch          `pg_eps_compact`; one sync in total
  :756-762 full torch.sort per row                     `pg_knn_hamming` (in-register top-(k+1))
  :298-325 1xN hamming + numpy set logic               `pg_index_flags` + `pg_compact_flags`

There is no CPU fallback for that path: without the HIP library or a GPU the calls raise
`prograph_amd._native.NativeUnavailable`.  A custom `distance` callable, a `comp` outside the
five orderings, non-byte representations (e.g. fp16 embeddings with `minkowski`), k > 63 or
L > 128 go through `_build_graph_generic`, which is the reference's batch loop kept on torch
ops on the GPU — the distance-operator protocol stays pluggable.

kNN tie rule: the reference's `torch.sort` (:758-760) is unstable, so with integer distances
its neighbour *indices* are implementation defined.  This implementation fixes the canonical
order (distance, index) == `torch.sort(stable=True)`, drops rank 0 like the reference does
and returns ranks 1..k.  Weights are bit-identical to the reference either way.
"""
import copy
import operator
import os

import numpy as np
import pandas as pd
import torch

from . import _native
from . import alignments as _alignments
from .distance import (alignment, cosine, euclidean, fit_alignment, hamming, levenshtein, local_alignment, minkowski, profile_alignment,
                       semiglobal_alignment, spectrum, substitution)
from .distance.profile_alignment import Profiles

_EMBED_F32 = {cosine: "cosine", euclidean: "euclidean"}      # fp32 embedding metrics of pg_cos.hip -> their _native prefix

_SCORES = (local_alignment, semiglobal_alignment, fit_alignment)      # similarities: ranked largest first (`_local_select`)
from .graph import CSRGraph, KNNGraph
from .protein import Protein
from .utils import Dataset, flatten

_CMP_CODE = {operator.le: _native.CMP_LE, operator.lt: _native.CMP_LT, operator.eq: _native.CMP_EQ,
             operator.ge: _native.CMP_GE, operator.gt: _native.CMP_GT}
# comp(t, s) as a test on s: what the fp16 eps kernels, which compare (value, threshold), are given for a score
_CMP_MIRROR = {_native.CMP_LE: _native.CMP_GE, _native.CMP_LT: _native.CMP_GT, _native.CMP_EQ: _native.CMP_EQ,
               _native.CMP_GE: _native.CMP_LE, _native.CMP_GT: _native.CMP_LT}
_DEFAULT_SCALER = object()      # "use sklearn's MinMaxScaler" without importing sklearn at module import


class Prograph:
    def __init__(self, file, seed_seq=None, seqs_col="Sequence", columns=["Fitness"], index_col=0,
                 amino_acids="ACDEFGHIKLMNPQRSTVWY"):
        try:
            ext = file.split(".")[-1]
            if ext == "csv":
                self.graph = self.csvDataLoader(file, seqs_col=seqs_col, columns=columns, index_col=index_col)
            elif ext == "pkl":
                self.graph = pd.read_pickle(file)
            else:
                raise ValueError(ext)
        except Exception:
            # the reference turns every load problem (missing file, file=None, file=2, ...) into this
            raise FileNotFoundError("File could not be opened")

        self.file, self.seed_seq, self.seqs_col = file, seed_seq, seqs_col
        self.columns, self.index_col, self.amino_acids = columns, index_col, amino_acids

        self.seed = Protein(seed_seq) if seed_seq else Protein(**self.graph.loc[0])
        self.seq_len = len(self.seed)
        self.len = len(self)

        self.tokens = {aa.encode("utf-8"): i for i, aa in enumerate(self.amino_acids, start=1)}
        self._planes = {}            # device-resident plane layouts, keyed by representation
        self.tokenized = self._ingest_tokens(self.graph[seqs_col])
        self._token_dict = None
        self.seq_idxs = dict(zip(self.graph[seqs_col], range(len(self.graph))))   # last duplicate wins

        self.mutated_positions = self.calc_mutated_positions()
        self.sequence_mutation_locations = self.boolean_mutant_array(self.seed.Sequence)
        self.mutation_arrays = self.gen_mutation_arrays()
        self.csr_graphs = {}         # name -> CSRGraph / KNNGraph kept on the device
        self._csr_rows = {}          # name -> row objects of the column the device graph answers for

        if "Tokenized" not in self.graph:
            self.graph["Tokenized"] = list(self.tokenized)
        if isinstance(file, str) and ext == "pkl":
            self._restore_graphs(os.path.splitext(file)[0] + ".graphs.npz")
        if "Neighbours" not in self.graph:
            self.graph["Neighbours"] = self.build_graph(eps=1, _keep="Neighbours")

        self.learners = {}
        print(self)

    # ------------------------------------------------------------------ dunder / query surface
    def __str__(self):
        hist = self._distance_histogram(self.seed.Sequence)
        present = np.nonzero(hist)[0]
        longest = max((len(s) for s in self("Sequence")), default=0)
        return f"""
            Prograph
            Number of Sequences : {len(self)}
            Max Distance        : {int(present[-1])}
            Longest Sequence    : {longest}
            Number of Distances : {len(present)}
            Seed Sequence       : {self.coloured_seed_string()}
                Modified positions are shown in green"""

    def __repr__(self):
        return (f"Prograph(file={self.file},\n seed_seq='{self.seed.Sequence}',\n seqs_col='{self.seqs_col}',\n"
                f" columns={self.columns},\n index_col={self.index_col},\n amino_acids='{self.amino_acids}')")

    def __len__(self):
        return len(self.graph)

    def __getitem__(self, idx):
        return self.graph.iloc[self.query(idx)]

    def __call__(self, label=None, **kwargs):
        return self.label_iter(label, **kwargs)

    def label_iter(self, label, **kwargs):
        """`pgraph("Sequence")`, `pgraph("sklearn", ...)`, `pgraph("pytorch", ...)`, `pgraph()`; copies."""
        if label == "pytorch":
            return self.pytorch_dataloaders(**kwargs)
        if label == "sklearn":
            return self.sklearn_data(**kwargs)
        if label is None:
            return self.graph.copy()
        return self.graph[label].copy()

    @property
    def token_dict(self):
        """{tuple(tokens): index}; built on first use (O(N*L) Python objects, unused by the hot path)."""
        if self._token_dict is None:
            self._token_dict = {tuple(seq): i for i, seq in enumerate(self.tokenized)}
        return self._token_dict

    def query(self, sequence):
        """int / str / token tuple / list or array of those -> positional index (reference :204-240)."""
        missing = "This sequence is not in the dataset."
        if isinstance(sequence, (int, np.integer)):
            assert sequence <= self.len, "Index exceeds bounds of dataset"
            return sequence
        if isinstance(sequence, (np.ndarray, list)):
            first = sequence[0]
            if isinstance(first, (int, np.integer, np.bool_)):
                return sequence
            if isinstance(first, str):
                return [self.seq_idxs.get(s, missing) for s in sequence]
            print("Wrong data format in numpy array or list iterable.")
            return None
        if isinstance(sequence, str):
            return self.seq_idxs.get(sequence, missing)
        if isinstance(sequence, tuple):
            assert len(sequence) == self.seq_len, "Tuple not valid length for dataset."
            hits = np.where(np.all(np.asarray(sequence) == self.tokenized, axis=1))[0]
            assert len(hits) > 0, "Not a valid tuple representation of a protein in this dataset."
            return int(hits[0]) if len(hits) == 1 else int(hits)
        raise ValueError("Input format not understood.")

    # ------------------------------------------------------------------ ingest / tokenisation
    @staticmethod
    def csvDataLoader(csvfile, seqs_col, columns="all", index_col=None):
        data = pd.read_csv(csvfile, index_col=index_col)
        if columns == "all":
            columns = [c for c in data.keys() if c != seqs_col]
        wanted = [seqs_col] + list(columns)
        if "Neighbours" in data:
            wanted.append("Neighbours")
        return data[wanted]

    def _byte_view(self, sequences):
        """The fixed-width byte view of the strings ((N, Lmax) uint8, NUL padded: numpy 'S' storage) and the
        256-entry letter table (letter j of `amino_acids` -> j+1, everything else -> 0; reference :127)."""
        arr = np.array(sequences, dtype="bytes").reshape(-1)
        width = max(arr.dtype.itemsize, 1)
        table = np.zeros(256, dtype=int)
        for ch, tok in self.tokens.items():
            if len(ch) == 1:
                table[ch[0]] = tok
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(len(arr), width) if (len(arr) and arr.dtype.itemsize) else \
            np.zeros((len(arr), width), dtype=np.uint8)
        return raw, table

    def tokenize(self, sequences):
        """
        Strings -> (N, Lmax) int tokens: letter j of `amino_acids` -> j+1, padding / unknown -> 0
        (reference :454-474).  One table lookup over the fixed-width byte view instead of one
        masked pass per letter.
        """
        raw, table = self._byte_view(sequences)
        return table[raw]

    def _ingest_tokens(self, sequences):
        """
        The constructor's tokenisation.  With a GPU the byte view goes to the device once and ONE
        kernel (`pg_pack_bytes`) applies the letter table, bit-slices the tokens into the plane layout the graph
        kernels read and writes the token matrix: the planes are cached for `build_graph` / `indexing`, the host's
        `self.tokenized` is that matrix copied back (uint8) and widened - the table pass over N x L bytes on the
        host is gone.  Without a device (the host-logic tests' fake backend), or beyond the kernels' widths, the host
        table lookup of `tokenize` is used.
        """
        raw, table = self._byte_view(sequences)
        bits = _native.BITS_5 if len(self.amino_acids) <= 31 else _native.BITS_8
        limit = _native.MAX_L_5BIT if bits == _native.BITS_5 else _native.MAX_L
        try:
            on_gpu = _native.device().type == "cuda" and hasattr(_native, "pack_bytes")
        except _native.NativeUnavailable:
            on_gpu = False
        if not on_gpu or raw.shape[0] == 0 or raw.shape[1] > limit or len(self.amino_acids) > 255:
            return table[raw]
        planes, tok = _native.pack_bytes(raw, table.astype(np.uint8), bits=bits, want_tokens=True)
        self._planes["Tokenized"] = planes
        self._tok_u8_dev = tok
        return tok.cpu().numpy().astype(int)

    def custom_tokenize(self, seq, tokenizer=None):
        if tokenizer is None:
            return np.array([self.tokens[aa.encode("utf-8")] for aa in seq])
        return "This feature is not ready yet"

    def embedding(self, embedded, name):
        self.graph[f"{name}_embedded"] = embedded

    def boolean_mutant_array(self, seq=None):
        return self.tokenized != self.tokenized[self.query(seq)]

    def calc_mutated_positions(self):
        seed = self.tokenize(self.seed.Sequence)
        if seed.shape[1] < self.tokenized.shape[1]:                      # variable-length data: the seed is padded like every row
            seed = np.pad(seed, ((0, 0), (0, self.tokenized.shape[1] - seed.shape[1])))
        varies = ~np.all(self.tokenized == seed, axis=0)
        return np.nonzero(varies[: len(self.seed)])[0]

    def coloured_seed_string(self):
        try:
            from colorama import Fore, Style
            on, off = Fore.GREEN, Style.RESET_ALL
        except ImportError:
            on = off = ""
        marked = set(int(i) for i in self.mutated_positions)
        return "".join(f"{on}{c}{off}" if i in marked else c for i, c in enumerate(self.seed.Sequence))

    def gen_mutation_arrays(self):
        n_aa = len(self.amino_acids)
        xs = np.arange(self.seq_len * n_aa)
        ys = np.repeat(np.arange(self.seq_len), n_aa)
        modifiers = np.tile(np.arange(n_aa), self.seq_len)
        return xs, ys, modifiers

    def generate_mutations(self, seq):
        seq = self.tokenized[self.query(seq)]
        xs, ys, mutations = self.mutation_arrays
        variants = np.tile(np.asarray(seq, dtype=float), (len(xs), 1))
        variants[xs, ys] = mutations
        return variants[~np.all(variants == seq, axis=1)]

    def get_mutated_positions(self, positions):
        for pos in positions:
            assert pos in self.mutated_positions, "{} is not a position that was mutated in this dataset".format(pos)
        constants = np.setdiff1d(self.mutated_positions, positions)
        return np.all(~self.sequence_mutation_locations[:, constants], axis=1)

    def get_data(self, tokenized=False):
        if tokenized:
            return np.array([x[["Sequence", "Fitness"]] for x in self.graph])
        return copy.copy(self.tokenized)

    # ------------------------------------------------------------------ device residency
    def _byte_planes(self, representation="Tokenized", idxs=None):
        """Plane layout of a byte-token representation on the GPU.  Only the token matrix of the
        constructor is cached (`self.tokenized` never changes); any other representation is a
        DataFrame column the user may reassign (`embedding()`, `pg.graph[name] = ...`) and is read and
        packed on every call, as the reference re-reads `self(representation)` (prograph.py:726)."""
        key = representation
        if idxs is None and key == "Tokenized" and key in self._planes:
            return self._planes[key]
        if representation == "Tokenized":
            mat = self.tokenized
        else:
            mat = np.vstack(self(representation))
        mat = np.asarray(mat)
        if not np.issubdtype(mat.dtype, np.integer):
            raise ValueError("not an integer representation")
        if mat.size and mat.min() >= 0 and mat.max() <= 255:
            mat = mat.astype(np.uint8)               # 8x less PCIe traffic than the int64 token matrix
        # tokens of the built-in tokeniser are 0..len(amino_acids): 5 bit planes cover 31 letters
        bits = _native.BITS_5 if (representation == "Tokenized" and len(self.amino_acids) <= 31) else None
        planes = _native.pack(torch.from_numpy(np.ascontiguousarray(mat)), rows=idxs, bits=bits)
        if idxs is None and key == "Tokenized":
            self._planes[key] = planes
        return planes

    def _planes_or_none(self):
        """The cached plane layout, or None when the token matrix is beyond the fused kernels' limits
        (more than 255 positions, 128 for alphabets above 31 symbols): the queries below then run on
        the native dense operator (`hamming`, any length) plus torch ops on the GPU."""
        try:
            return self._byte_planes()
        except (ValueError, TypeError):
            return None

    def _tokens_dev(self):
        if getattr(self, "_tok_dev", None) is None:
            self._tok_dev = torch.as_tensor(np.ascontiguousarray(self.tokenized), device=_native.device())
        return self._tok_dev

    def _row_distances_long(self, ref):
        """(N,) int64 Hamming distances of every sequence to row `ref`, long-sequence path."""
        T = self._tokens_dev()
        return hamming(T, T[ref:ref + 1]).reshape(-1)

    def _distance_histogram(self, reference_seq):
        planes = self._planes_or_none()
        ref = int(self.query(reference_seq))
        if planes is None:
            return torch.bincount(self._row_distances_long(ref)).cpu().numpy()
        _, hist, _ = _native.index_flags(planes, ref, want_dist_out=False, want_flags=False)
        return hist.cpu().numpy()

    # ------------------------------------------------------------------ indexing
    def positions(self, positions):
        return self.indexing(positions=positions)

    def distances(self, distances):
        return self.indexing(distances=distances)

    def indexing(self, reference_seq=None, distances=None, positions=None, percentage=None, Bool="or",
                 complement=False):
        """
        Distance-k / mutated-position index queries (reference :254-343), evaluated in one fused
        1xN HIP pass: Hamming distance of every sequence to the reference row, membership of that
        distance in `distances`, the position logic, then a device stream compaction to the
        ascending index array.  `percentage` / `complement` are the reference's numpy post-steps.
        """
        assert Bool == "or" or Bool == "and", "Not a valid boolean value."
        if reference_seq is None:
            reference_seq = self.seed.Sequence
        ref = int(self.query(reference_seq))
        planes = self._planes_or_none()

        want = None
        if distances is not None:
            if type(distances) == int:
                distances = [distances]
            assert type(distances) == list, "Distances must be provided as integer or list"
            hist = self._distance_histogram(reference_seq)
            for d in distances:
                assert isinstance(d, (int, np.integer)) and 0 <= d < len(hist) and hist[d] > 0, f"{d} is not a valid distance"
            want = distances

        pos_mode, pos_mask, not_mask = 0, None, None
        if positions is not None:
            ref_len = len(self[reference_seq]["Sequence"])
            ncol = self.tokenized.shape[1]
            for p in positions:
                if not -ncol <= p < ncol:
                    raise IndexError(f"index {p} is out of bounds for axis 1 with size {ncol}")
            pos_mask = [p % ncol for p in positions]
            not_mask = [p for p in range(ref_len) if p not in positions]
            if len(positions) == 0:
                raise TypeError("reduce() of empty sequence with no initial value")
            pos_mode = 1 if Bool == "or" else 2

        if want is None and pos_mode == 0:
            idxs = np.array(range(len(self)))
        elif planes is None:
            # long sequences: the same logic (reference :298-325) with torch ops on the GPU
            T = self._tokens_dev()
            keep = torch.ones(len(self), dtype=torch.bool, device=T.device)
            if want is not None:
                keep &= torch.isin(self._row_distances_long(ref), torch.as_tensor(want, device=T.device))
            if pos_mode:
                mut = T != T[ref:ref + 1]
                sel = mut[:, pos_mask]
                working = sel.any(dim=1) if pos_mode == 1 else sel.all(dim=1)
                if not_mask:
                    working &= ~mut[:, not_mask].any(dim=1)
                keep &= working
            idxs = torch.nonzero(keep).reshape(-1).cpu().numpy()
        else:
            _, _, flags = _native.index_flags(planes, ref, want=want, pos_mode=pos_mode, pos_mask=pos_mask,
                                              not_mask=not_mask, want_dist_out=False, want_hist=False)
            idxs = _native.compact_flags(flags).cpu().numpy()

        if percentage is not None:
            assert 0 <= percentage <= 1, "Percentage must be between 0 and 1"
            keep = np.zeros(len(idxs), dtype=bool)
            keep[np.random.choice(np.arange(len(idxs)), size=int(len(idxs) * percentage), replace=False)] = 1
            return idxs[keep]

        assert len(idxs) != 0, "No possible valid indices have been provided."
        if complement:
            return idxs, np.setdiff1d(np.arange(self.len), idxs)
        return idxs

    def calc_neighbours(self, seq, eps=1, distance=hamming, comp=operator.eq, weights=False):
        """Column indices with comp(distance to `seq`, eps) (reference :526-544)."""
        if distance is hamming and comp in _CMP_CODE:
            planes = self._planes_or_none()
            if planes is None:
                d = self._row_distances_long(int(self.query(seq)))
                return torch.nonzero(comp(d, eps)).reshape(-1).cpu().numpy()
            want = [d for d in range(256) if comp(d, eps)]
            _, _, flags = _native.index_flags(planes, int(self.query(seq)), want=want,
                                              want_dist_out=False, want_hist=False)
            return _native.compact_flags(flags).cpu().numpy()
        if (distance is levenshtein or isinstance(distance, alignment)) and comp in _CMP_CODE:
            return self.search(self._lev_query(seq), eps=eps, distance=distance, comp=comp)[0][0]
        d = distance(self.tokenized, self.tokenized[self.query(seq)].reshape(1, -1))
        return np.where(comp(d, eps))[1]

    def neighbourhood(self, seq, eps, distance=hamming):
        """All rows within `eps` of `seq`, the row itself included (reference :571-588).  A string that is not in the
        dataset is answered by `search(seq, eps=eps)`: the dataset rows within `eps` of it.  `distance=levenshtein`: the rows
        within `eps` edits, for a string of any length up to 2048; an `alignment` instance likewise."""
        if distance is levenshtein or isinstance(distance, alignment):
            hit = np.zeros(len(self), dtype=bool)
            hit[self.search(self._lev_query(seq), eps=eps, distance=distance)[0][0]] = True
            return self[hit]
        if isinstance(seq, str) and seq not in self.seq_idxs:
            hit = np.zeros(len(self), dtype=bool)
            hit[self.search(seq, eps=eps)[0][0]] = True
            return self[hit]
        planes = self._planes_or_none()
        if planes is None:
            dist = self._row_distances_long(int(self.query(seq)))
        else:
            dist, _, _ = _native.index_flags(planes, int(self.query(seq)), want_hist=False, want_flags=False)
        return self[(dist <= eps).cpu().numpy().flatten()]

    def _lev_query(self, seq):
        """A sequence as `search` takes it: a string as it is, anything `query` resolves as that row's tokens."""
        return seq if isinstance(seq, str) else np.asarray(self.tokenized[self.query(seq)])

    def neighbourhood_clustering(self, eps, distance=hamming):
        clusters, seen = {}, set()
        for i, seq in enumerate(self("Sequence")):
            if i not in seen:
                members = self.neighbourhood(seq, eps, distance)
                clusters[i] = members
                seen |= set(members.index)
        return clusters

    # ------------------------------------------------------------------ queries against the dataset
    def nearest_neighbour(self, seq, distance=hamming, batch_size=8, representation="Tokenized"):
        """(the nearest dataset row of every query, as `self[idx]`; the smallest of their distances) - the reference's
        documented return line (prograph/prograph.py:546-569), on `search(seq, k=1)`.  `batch_size` is accepted for
        compatibility, as in `build_graph`."""
        res = self.search(seq, 1, distance=distance, representation=representation)
        idx = np.array([int(i[0]) for i, _ in res], dtype=np.int64)
        distances = np.array([w[0] for _, w in res])
        return self[idx], np.min(distances)

    def search(self, queries, k=None, eps=None, distance=hamming, representation="Tokenized", similarity=False,
               output="tuples", comp=operator.le, min_identity=None, min_columns=0, candidates=None, pool=None):
        """
        The k nearest dataset rows (`k`), or the dataset rows within a radius (`eps`), of sequences or embeddings that
        need not be in the dataset; exactly one of the two.
        `k`: for the dataset
        representation X (N rows) and the queries Y, staged as `build_graph` stages them, ranks 0..min(k, N)-1 of
        `torch.sort(distance(X, Y, similarity=similarity), dim=1, stable=True, descending=similarity)` per query - rank
        0 is kept (a query equal to a dataset row has that row first), ties go to the lower dataset index.
        `eps` (0 is a valid radius: exact matches): per query the dataset rows j with `comp(distance(X, Y)[q, j], eps)` in
        ascending j, the order `torch.where` yields; no pair is excluded for d = 0.  With `similarity=True` the test is
        `comp(1/(1+eps), s)` as in `build_graph` and the weights are the similarities.  The five orderings of `operator`
        run on the device, any other `comp` takes the generic loop.  Returns a list of Q `(indices, weights)` tuples with
        the dtypes of `build_graph(eps=)` (queries without a hit share one empty pair), or with `output="csr"` a device
        `CSRGraph` with Q rows and `ncols = N`.
        `queries`: a string or a list of strings (the dataset's letter table; unknown letters and padding -> 0), a 1-D or
        2-D integer token array, or for embeddings a 1-D or 2-D float array / tensor (cast to fp16); the shorter of
        queries and dataset is right-padded with zeros.  Returns a list of Q `(indices, weights)` tuples in rank order,
        or with `output="csr"` a device `KNNGraph` with Q rows whose columns are dataset rows.
        Hamming runs the fused query kernels (`pg_query_knn_hamming`, `pg_query_eps_*`), sequences beyond one record the
        dense kernel plus the fp16 selection; Minkowski, cosine and Euclidean the fused embedding kernels; Levenshtein (queries of
        any length up to 2048, not only the dataset's) blocks of `pg_levenshtein_dense`, or of `pg_levenshtein_long_dense`
        when queries or dataset are wider than 128 positions, plus the fp16 selection; a
        `substitution` distance blocks of `pg_substitution_dense` plus the fp16 selection; an `alignment` distance (queries
        of any length up to 128) blocks of `pg_alignment_dense` plus the fp16 selection; a `spectrum` distance (strings or
        token arrays of any width up to 2048, wider or narrower than the dataset) `pg_spectrum_profile` on both sides
        and then the fused cosine / Euclidean kernels; any other `distance` the generic loop.
        A `local_alignment` instance is a score, not a distance: `similarity` is not consulted, `k` gives the LARGEST scores
        first (ties to the lower dataset index), `eps` the rows with `s > 0 and comp(eps, s)` - the default comp reads
        `s >= eps` - and the weights are the scores (blocks of `pg_alignment_local_dense` plus the fp16 selection).  A
        `semiglobal_alignment` instance behaves in the same way on its own kernels (`pg_alignment_semiglobal_dense`), and so
        does a `fit_alignment` instance (`pg_alignment_fit_dense`), which is NOT symmetric: the QUERY is aligned whole within
        any stretch of a dataset row - a hit (q, c) reads "query q, whole, placed in row c" -, its scores may be negative
        (a `k` list ranks them), and `eps` keeps `s > 0`.
        A `profile_alignment` instance takes PROFILES as `queries` - one (L, A) array, a (Q, L, A) array or a list of (L_q, A)
        arrays (distance/profile_alignment.py) - and otherwise behaves as the score of its mode: largest first, `eps` keeps
        `s > 0 and comp(eps, s)`, the weights are the scores, in fit mode a hit (q, c) reads "profile q, whole, in row c"
        (blocks of `pg_alignment_profile_dense` / `pg_alignment_profile_long_dense`); it takes no identity cut.
        `min_identity=` (0..1) / `min_columns=`: as in `build_graph` - the hits are found as above, each is aligned with
        its query (`align(..., queries=, ops=False)`), and those below the cut are dropped; the result is a `CSRGraph`
        (`output="csr"`, also for `k`: a query may keep fewer than k hits) or the filtered tuple list.
        `candidates=` / `pool=`: FILTER AND REFINE, as in `build_graph` - `distance` must be one of the four alignment
        operators, the pool of a query is `search(queries, k=pool, distance=candidates)` (or `candidates` is a ready search
        result and `pool` None), and `rescore(..., queries=queries)` ranks it: exact within the pool, approximate overall.
        `similarity=True` raises `ValueError`.
        """
        if self._identity_cut_asked("search", distance, min_identity, min_columns):
            g = self.search(queries, k=k, eps=eps, distance=distance, representation=representation, similarity=similarity,
                            output="csr", comp=comp, candidates=candidates, pool=pool)
            g = self._identity_cut(g, distance, min_identity, min_columns, representation, queries=queries)
            return g if output == "csr" else g.to_tuples()
        if candidates is not None or pool is not None:
            return self._search_candidates(queries, k, eps, comp, similarity, representation, distance, output, candidates, pool)
        if eps is None:
            if not k:                                                      # build_graph's errors for k
                raise ValueError("Epsilon or K must be provided, but both cannot be as they are different methods of graph construction.")
            if not isinstance(k, int):
                raise TypeError("K must be provided as an integer.")
            if k < 1:
                raise ValueError("K must be at least 1.")
        else:
            if k is not None:
                raise ValueError("Epsilon or K must be provided, but both cannot be as they are different methods of graph construction.")
            if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)):
                raise TypeError("Epsilon must be provided as a number.")
            if eps != eps:
                raise ValueError("Epsilon must not be NaN.")
        if isinstance(distance, profile_alignment):                        # the queries are profiles, not sequences
            g = self._search_profile(queries, k, eps, comp, representation, distance)
            return g if output == "csr" else g.to_tuples()
        strings = None
        if isinstance(queries, str):
            strings = [queries]
        elif isinstance(queries, (list, tuple)) and len(queries) and all(isinstance(q, str) for q in queries):
            strings = list(queries)
        if strings is None:
            Y = queries if isinstance(queries, torch.Tensor) else torch.as_tensor(np.asarray(queries))
            if Y.dim() == 1:
                Y = Y.reshape(1, -1)
            if Y.dim() != 2 or Y.shape[0] == 0 or Y.shape[1] == 0:
                raise ValueError("queries must be a non-empty string, list of strings or 1-D / 2-D array")
        elif len(strings) == 0:
            raise ValueError("queries must be a non-empty string, list of strings or 1-D / 2-D array")
        else:
            Y = None
        route = self._route(distance, comp if eps is not None else operator.le, k)      # a `k` search does not consult `comp`
        g = None
        if route is not None and route[1]:
            g = getattr(self, route[1])(strings, Y, k, eps, comp, similarity, representation, distance)
        if g is None and eps is None:
            return self._search_generic(strings, Y, k, similarity, representation, distance, output)     # tuples itself
        if g is None:
            g = self._search_eps_generic(strings, Y, eps, comp, similarity, representation, distance)
        return g if output == "csr" else g.to_tuples()

    # The device routes in the order `build_graph` and `search` ask them: (does `distance` take it; does it need `comp`
    # among the five orderings and k within the selection's rounds; build_graph's method; search's method).  The methods
    # are looked up by name on `self` at every call; a method's None means "the generic loop".  Graph methods are called
    # (idxs, eps, k, similarity, representation, comp, cap=, distance=), search methods (strings, Y, k, eps, comp,
    # similarity, representation, distance).  Hamming graphs have no entry of their own: `build_graph` tries the fused
    # engine and `_build_graph_long` after this list.
    _ROUTES = (
        (lambda d: d is hamming, True, None, "_search_hamming"),
        (lambda d: d is minkowski, True, "_build_graph_minkowski", "_search_embedded"),
        (lambda d: d is cosine, True, "_build_graph_cosine", "_search_embedded"),
        (lambda d: d is euclidean, True, "_build_graph_euclidean", "_search_embedded"),
        (lambda d: isinstance(d, spectrum), True, "_build_graph_spectrum", "_search_spectrum"),
        (lambda d: d is levenshtein, True, "_build_graph_levenshtein", "_search_levenshtein"),
        (lambda d: isinstance(d, substitution), True, "_build_graph_substitution", "_search_substitution"),
        (lambda d: isinstance(d, alignment), True, "_build_graph_alignment", "_search_alignment"),
        (lambda d: isinstance(d, _SCORES), False, "_build_graph_local", "_search_local"),
    )

    def _route(self, distance, comp, k):
        """(build_graph's method, search's method) of the entry of `_ROUTES` that takes `distance`; None when there is
        none, or when it needs the device selection and `comp` or `k` is outside what that covers."""
        for takes, limited, graph, query in self._ROUTES:
            if takes(distance):
                if limited and not (comp in _CMP_CODE and (k is None or k <= _native.MAX_K_ROUNDS)):
                    return None
                return graph, query
        return None

    def _dataset_matrix(self, representation):
        return self.tokenized if representation == "Tokenized" else np.vstack(self(representation))

    def _query_tokens(self, strings, Y):
        """The queries as an integer token matrix: strings through the dataset's letter table at their own width (unknown
        letters and padding -> 0), an array or tensor as a host array."""
        if strings is not None:
            raw, table = self._byte_view(strings)
            return table[raw]
        return Y.cpu().numpy() if isinstance(Y, torch.Tensor) else np.asarray(Y)

    def _search_hamming(self, strings, Y, k, eps, comp, similarity, representation, distance=None):
        """Byte-token queries on the device: the fused query kernels within one record (`pg_query_knn_hamming`,
        `pg_query_eps_*`: uint8 weights), the staged frame on `_hamming_segments` up to 2048 positions (int16 weights, as
        `_build_graph_long` gives them).  Similarities: comp(1/(1+eps), 1/(1+d)) is the same integer test on d (as in
        `build_graph`); the container forms them.  None when dataset or queries are not byte tokens (the generic loop)."""
        ops = self._hamming_operands(strings, Y, representation, _native.MAX_N_KNN if k is not None else 1 << 31)
        if ops is None:
            return None
        n, bits, X, T, qp, dp = ops
        if qp is None:
            dev, width = _native.device(), max(X.shape[1], T.shape[1])
            Xd = torch.zeros((X.shape[0], width), dtype=torch.uint8, device=dev)
            Xd[:, :X.shape[1]] = torch.as_tensor(X.astype(np.uint8), device=dev)
            Td = torch.zeros((T.shape[0], width), dtype=torch.uint8, device=dev)
            Td[:, :T.shape[1]] = torch.as_tensor(T.astype(np.uint8), device=dev)
            # the blocks of this route hold at least 64 queries, a graph's floor, not 1
            return self._staged(n, Td.shape[0], self._hamming_segments(Xd, Td, bits), "f16", torch.int16, k, eps, comp,
                                similarity, True, floor=64)
        if k is not None:
            idx, dist = _native.query_knn(qp, dp, min(k, n))
            return KNNGraph(idx, dist, n, similarity=similarity, first=0)
        eps = min(max(float(eps), -1.0), 4096.0)                         # (the same test on every d in 0..2048)
        indptr, indices, wts = _native.query_eps(qp, dp, _CMP_CODE[comp], eps)
        return CSRGraph(indptr, indices, wts, n, similarity=similarity)

    def _hamming_operands(self, strings, Y, representation, max_n):
        """The staging of byte-token queries: (n, bits, X, T, query planes, dataset planes) within one record (the
        dataset's cached planes when they fit, else the dataset packed at the queries' width for this call), planes of
        None for the staged path up to 2048 positions.  None when dataset or queries are not byte tokens, or the
        dataset has `max_n` rows or more (the generic loop then)."""
        try:
            X = np.asarray(self._dataset_matrix(representation))
        except (ValueError, TypeError):
            return None
        raw = table = None
        if strings is not None:
            raw, table = self._byte_view(strings)
            if len(self.amino_acids) > 255:
                return None
            T = table[raw]
        else:
            T = self._query_tokens(None, Y)
        if X.ndim != 2 or X.shape[0] == 0 or X.shape[1] == 0 or not np.issubdtype(X.dtype, np.integer):
            return None
        if not np.issubdtype(T.dtype, np.integer) or T.min() < 0 or T.max() > 255 or X.min() < 0 or X.max() > 255:
            return None
        n, width = X.shape[0], max(X.shape[1], T.shape[1])
        if n >= max_n or width > self._LONG_MAX_L:
            return None
        bits = _native.BITS_5 if max(int(X.max()), int(T.max())) <= 31 else _native.BITS_8
        limit = _native.MAX_L_5BIT if bits == _native.BITS_5 else _native.MAX_L
        if width > limit:
            return n, bits, X, T, None, None
        dp = self._planes_or_none() if representation == "Tokenized" else None
        if dp is None or dp.l != width or dp.bits != bits:
            dp = _native.pack(torch.from_numpy(np.ascontiguousarray(X.astype(np.uint8))), bits=bits, width=width)
        if raw is not None:
            wide = np.zeros((raw.shape[0], width), dtype=np.uint8)        # NUL padding: token 0, as clean_input pads
            wide[:, :raw.shape[1]] = raw
            qp, _ = _native.pack_bytes(wide, table.astype(np.uint8), bits=bits, want_tokens=False)
        else:
            qp = _native.pack(torch.from_numpy(np.ascontiguousarray(T.astype(np.uint8))), bits=bits, width=width)
        return n, bits, X, T, qp, dp

    _BLOCK_ELEMS = 1 << 27        # elements of a staged distance block: <= 256 MB of fp16 at a time

    def _block_rows(self, n, rows, floor, elem_bytes=2):
        """Rows per staged block of distances to n columns: `floor` is 64 for self graphs, 1 for queries.  Blocks of
        4-byte elements (the int32 blocks of the alignment kernels beyond 128 positions) hold half as many."""
        return max(floor, min(rows, self._BLOCK_ELEMS * 2 // elem_bytes // n))

    # the two kinds of staged block: the `_native` selection wrappers by name (looked up at every call) and bytes per element
    _BLOCK_KINDS = {"f16": ("f16_knn", "f16_eps", 2), "i32": ("i32_knn", "i32_eps", 4)}

    @staticmethod
    def _select_blocks(blocks, kind, knn=None, eps=None, wdtype=None):
        """The selection over an iterator of distance blocks (row blocks of one matrix) of one kind of `_BLOCK_KINDS`, one
        block alive at a time: knn = (k, first, descending) -> (idx, w) of `f16_knn` / `i32_knn`, or eps = (cmp, thr,
        similarity, keep_zero) -> the CSR (indptr, indices, w) of `f16_eps` / `i32_eps` (which takes an integer thr and no
        similarity), the blocks' results concatenated.  wdtype: what the weights are cast to."""
        knn_name, eps_name, _ = Prograph._BLOCK_KINDS[kind]
        parts = []
        for block in blocks:
            if knn is not None:
                part = getattr(_native, knn_name)(block, knn[0], first=knn[1], descending=knn[2])
            else:
                cmp, thr, similarity, keep_zero = eps
                kw = {"similarity": similarity} if kind == "f16" else {}
                if keep_zero:                                             # self graphs call without keep_zero, as ever
                    kw["keep_zero"] = True
                part = getattr(_native, eps_name)(block, cmp, thr, **kw)
            del block
            parts.append(part if wdtype is None else part[:-1] + (part[-1].to(wdtype),))
        if knn is None:
            return _native.cat_csr(parts)
        return torch.cat([p_[0] for p_ in parts]), torch.cat([p_[1] for p_ in parts])

    def _staged(self, n, q, dense, kind, wdtype, k, eps, comp, similarity, query, floor=None, raw=False, score=None):
        """
        The frame of every staged route: q rows against n columns, cut into row blocks that
        `dense(r0, r1)` computes as blocks of `kind`, the selection of `_select_blocks` over them, the container.
        `query` False is a self graph (q == n), True a search; what follows from it:
                       self graph                                    search
          ranks        1..min(k, n-1); none left: `_empty_knn`       0..min(k, n)-1, the container told first=0
          d = 0        dropped                                       kept
          eps          to `_integer_threshold` as it is              clamped to -1..4096 first
          block rows   `_block_rows(n, n, 64, ...)`                  `_block_rows(n, q, 1, ...)` (`floor` overrides)
          k or eps?    `if k` (`build_graph` has rejected 0)         `k is not None` (eps = 0 is a radius)
        int32 blocks take their threshold from `_long_threshold`, which clamps to -1..2^31 for both.
        `raw`: the blocks hold final fp16 values, similarities included (Minkowski): `eps` is the threshold as given, the
        kernels are told `similarity` and rank similarities largest first.  Else the values are integers, thresholds are
        integer tests and the container forms similarities.
        `score=(K, diagonal)`: the blocks hold scores + K (`_local_select`): largest first, comp(eps, s) as the mirrored
        test of (s + K, eps + K), clamped for graphs too; an entry of value 0 is kept iff K, K comes off the weights on
        the device, then `s > 0` is applied (`_unshift`), and the entries (r, r) go unless `diagonal`.
        """
        _, _, elem_bytes = self._BLOCK_KINDS[kind]
        first = 0 if query else 1
        K, diagonal = (0, True) if score is None else score
        rows = self._block_rows(n, q, floor or (1 if query else 64), elem_bytes)
        blocks = (dense(r0, min(q, r0 + rows)) for r0 in range(0, q, rows))
        if (k is not None) if query else k:
            kk = min(k, n - first)
            if not kk:
                return self._empty_knn(n, wdtype, _native.device(), similarity)
            descending = score is not None or (raw and similarity)
            idx, w = self._select_blocks(blocks, kind, knn=(kk, first, descending), wdtype=wdtype)
            return KNNGraph(idx, w - K if K else w, n, similarity=similarity, first=first)
        cmp = _CMP_CODE[comp] if score is None else _CMP_MIRROR[_CMP_CODE[comp]]
        if raw:
            thr = eps
        elif kind == "i32":
            thr = self._long_threshold(cmp, float(eps) + K)
        elif query or score is not None:
            thr = self._integer_threshold(cmp, min(max(float(eps) + K, -1.0), 4096.0))
        else:
            thr = self._integer_threshold(cmp, eps)
        keep_zero = query if score is None else bool(K)
        csr = self._select_blocks(blocks, kind, eps=(cmp, thr, raw and similarity, keep_zero), wdtype=wdtype)
        if K:
            csr = self._unshift(*csr, K, diagonal)
        elif not diagonal:
            csr = self._drop_diagonal(*csr)
        return CSRGraph(*csr, n, similarity=similarity)

    @staticmethod
    def _empty_knn(n, wdtype, dev, similarity, final=False):
        """The kNN graph of k = 0 (after clamping to n - 1)."""
        return KNNGraph(torch.zeros((n, 0), dtype=torch.int32, device=dev), torch.zeros((n, 0), dtype=wdtype, device=dev), n,
                        similarity=similarity, final=final)

    @staticmethod
    def _empty_csr(n, wdtype, dev, similarity):
        """The epsilon graph without an edge."""
        return CSRGraph(torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                        torch.zeros(0, dtype=wdtype, device=dev), n, similarity=similarity)

    @staticmethod
    def _nothing_within(cmp, thr):
        """Does the integer test (cmp, thr) of a self graph admit no distance at all: none of 1, 2, ...?"""
        return cmp in (_native.CMP_LE, _native.CMP_LT, _native.CMP_EQ) and thr - (cmp == _native.CMP_LT) < 1

    @staticmethod
    def _hamming_segments(Xd, Yd, bits):
        """`dense(r0, r1)` for byte tokens beyond one record of the fused engines: the fp16 block of rows r0..r1 of Yd
        against Xd (uint8 device matrices of one width), the sequence cut into column segments of whole records and their
        distances accumulated in place (`pg_hamming_dense`, `out=`)."""
        width = Xd.shape[1]
        w = (_native.MAX_L_5BIT if bits == _native.BITS_5 else _native.MAX_L) // 32 * 32     # whole 32-token groups
        segs = [(a, min(width, a + w)) for a in range(0, width, w)]
        xs = [_native.pack(Xd[:, a:b], bits=bits) for a, b in segs]

        def dense(r0, r1):
            block = None
            for (a, b), xp in zip(segs, xs):
                block = _native.hamming_dense(xp, _native.pack(Yd[r0:r1, a:b], bits=bits), out_bytes=2, out=block)
            return block
        return dense

    _MINK_STAGED_ROWS = 4096      # fewer Minkowski queries: dense block + selection (the fused kernel: 16 queries per CU)

    def _search_embedded(self, strings, Y, k, eps, comp, similarity, representation, distance):
        """The embedding entries of `_ROUTES` for `search`: arrays only (strings take the generic loop)."""
        if strings is not None:
            return None
        if k is not None:
            return self._search_embedding(Y, k, similarity, representation, distance)
        return self._search_eps_embedding(Y, eps, comp, similarity, representation, distance)

    def _search_embedding(self, Y, k, similarity, representation, distance):
        """Minkowski / cosine / Euclidean queries on the fused kernels with first = 0 (fp16 staging of both operands, as
        `build_graph` stages the column).  Few Minkowski queries take the staged dense + selection path instead, which
        gives the same values bit for bit.  None (the generic loop) when an operand is not a non-empty 2-D fp16 device
        tensor, or for cosine and Euclidean when one holds an inf or nan."""
        ops = self._embedding_operands(Y, representation)
        if ops is None:
            return None
        return self._search_embedding_staged(*ops, k, similarity, distance)

    def _search_embedding_staged(self, X, Y, k, similarity, distance):
        """`_search_embedding` from the staged operands on: X (N, D) and Y (Q, D) fp16 device tensors."""
        n, kk = X.shape[0], min(k, X.shape[0])
        if distance is minkowski:
            xp = _native.pack_f16(X)
            if Y.shape[0] < self._MINK_STAGED_ROWS:
                return self._mink_staged(xp, Y, k, None, None, similarity)
            idx, w = _native.minkowski_knn(xp, _native.pack_f16(Y), kk, first=0, similarity=similarity)
            return KNNGraph(idx, w, n, similarity=similarity, first=0)
        xc, yc = _native.cosine_prep(X), _native.cosine_prep(Y)
        if xc.nonfinite() or yc.nonfinite():
            return None
        knn = getattr(_native, _EMBED_F32[distance] + "_knn")
        idx, w = knn(xc, yc, kk, first=0, similarity=similarity)
        return KNNGraph(idx, w, n, similarity=similarity, final=True, first=0)

    def _mink_staged(self, xp, Y, k, eps, comp, similarity):
        """The staged Minkowski path of few queries: their dense fp16 blocks against the packed dataset on the frame; the
        blocks hold the final values (`raw`), `eps` is the threshold on them."""
        dense = lambda r0, r1: _native.minkowski_dense(xp, _native.pack_f16(Y[r0:r1]), similarity=similarity)     # noqa: E731
        return self._staged(xp.n, Y.shape[0], dense, "f16", torch.float16, k, eps, comp, similarity, True, raw=True)

    def _embedding_operands(self, Y, representation):
        """The fp16 device staging of dataset and queries (X, Y), the narrower one right-padded with zeros; None when the
        dataset is not a non-empty 2-D fp16 device tensor."""
        try:
            X = torch.as_tensor(np.vstack(self(representation)), dtype=torch.float16, device=_native.device())
            Y = torch.as_tensor(Y, dtype=torch.float16, device=X.device)
        except (ValueError, TypeError, RuntimeError):
            return None
        if X.dim() != 2 or X.shape[0] == 0 or X.shape[1] == 0 or not X.is_cuda:
            return None
        if X.shape[1] != Y.shape[1]:                                     # clean_input's zero right-padding
            d = max(X.shape[1], Y.shape[1])
            X = torch.nn.functional.pad(X, (0, d - X.shape[1]))
            Y = torch.nn.functional.pad(Y, (0, d - Y.shape[1]))
        return X, Y

    @staticmethod
    def _lev_operand(mat):
        """LevOperand of an integer token matrix the exact Levenshtein kernels take (at most 128 positions, tokens up to
        31, zeros only as trailing padding; one host sync for the last two), else None."""
        mat = np.asarray(mat)
        if mat.ndim != 2 or mat.shape[0] == 0 or not 1 <= mat.shape[1] <= 128 or not np.issubdtype(mat.dtype, np.integer):
            return None
        if mat.min() < 0 or mat.max() > 31:
            return None
        op = _native.lev_operand(torch.from_numpy(np.ascontiguousarray(mat.astype(np.uint8))))
        return op if op.valid() else None

    @staticmethod
    def _lev_long_operand(mat):
        """LevLongOperand of an integer token matrix the Levenshtein kernel beyond 128 positions takes (at most 2048
        positions, tokens up to 31, zeros only as trailing padding; one host sync for the last two), else None."""
        mat = np.asarray(mat)
        if (mat.ndim != 2 or mat.shape[0] == 0 or not 1 <= mat.shape[1] <= _native.LEV_LONG_MAX_L
                or not np.issubdtype(mat.dtype, np.integer)):
            return None
        if mat.min() < 0 or mat.max() > 31:
            return None
        op = _native.lev_long_operand(torch.from_numpy(np.ascontiguousarray(mat.astype(np.uint8))))
        return op if op.valid() else None

    def _search_levenshtein(self, strings, Y, k, eps, comp, similarity, representation, distance=None):
        """Edit-distance queries: blocks of `pg_levenshtein_dense` (uint8 weights: distances are at most 128), or of
        `pg_levenshtein_long_dense` (int16 weights) when the dataset or the queries are wider than 128 positions (up to
        2048 each, the two widths need not agree).  None (the generic loop with the operator) when dataset or queries
        are not what the kernels take."""
        try:
            X = self._dataset_matrix(representation)
            xw = np.shape(X)[1] if np.ndim(X) == 2 else 0
        except (ValueError, TypeError):
            return None
        T = self._query_tokens(strings, Y)
        long = max(xw, T.shape[1]) > _native.MAX_L
        if long and not _native.lev_long_ready():
            return None
        stage, dense, wdtype = ((self._lev_long_operand, _native.levenshtein_long_dense, torch.int16) if long else
                                (self._lev_operand, _native.levenshtein_dense, torch.uint8))
        try:
            xo = stage(X)
        except (ValueError, TypeError):
            return None
        qo = stage(T) if xo is not None else None
        if qo is None:
            return None
        return self._staged(xo.n, qo.n, lambda r0, r1: dense(xo, qo, out_bytes=2, rows=(r0, r1)), "f16", wdtype, k, eps, comp,
                            similarity, True)

    def _sub_tokens(self, mat, distance):
        """The uint8 form of an integer token matrix whose tokens all index the table of `distance`, else None."""
        mat = np.asarray(mat)
        if mat.ndim != 2 or mat.shape[0] == 0 or mat.shape[1] == 0 or not np.issubdtype(mat.dtype, np.integer):
            return None
        if mat.min() < 0 or mat.max() >= distance.symbols:
            return None
        return mat.astype(np.uint8)

    def _sub_native(self, width, distance):
        """Does a width take the kernel route?  One call covers it, and every distance - at most width * max(C) - is an
        integer that is exact in fp16."""
        return width <= _native.SUB_MAX_L and width * distance.max_cost <= self._LONG_MAX_L

    def _search_substitution(self, strings, Y, k, eps, comp, similarity, representation, distance):
        """Queries under a `substitution` distance: blocks of `pg_substitution_dense` in fp16, int16 weights; the narrower
        of queries and dataset is right-padded with zeros.  None (the generic loop with the operator) when dataset or
        queries are not integer tokens of the table, or a distance could exceed 2048."""
        try:
            X = self._sub_tokens(self._dataset_matrix(representation), distance)
        except (ValueError, TypeError):
            return None
        T = self._sub_tokens(self._query_tokens(strings, Y), distance) if X is not None else None
        if T is None:
            return None
        width = max(X.shape[1], T.shape[1])
        if not self._sub_native(width, distance):
            return None
        wide = [np.zeros((M.shape[0], width), dtype=np.uint8) for M in (X, T)]     # clean_input's zero right-padding
        wide[0][:, :X.shape[1]], wide[1][:, :T.shape[1]] = X, T
        xo, qo = (_native.sub_operand(torch.from_numpy(M), distance.symbols) for M in wide)
        cost = distance.device_cost()
        dense = lambda r0, r1: _native.substitution_dense(xo, qo, cost, out_bytes=2, rows=(r0, r1))     # noqa: E731
        return self._staged(xo.n, qo.n, dense, "f16", torch.int16, k, eps, comp, similarity, True)

    def _aln_native(self, width, distance):
        """Does a width take the alignment kernel route?  At most 128 positions, and every distance - at most
        width * max(max C, gap) + gap_open: align the shorter sequence, gap the rest in one run - is an integer that is
        exact in fp16."""
        return width <= _native.ALN_MAX_L and width * distance.max_cost + distance.gap_open <= self._LONG_MAX_L

    @staticmethod
    def _aln_long(width, distance):
        """Does a width beyond `_aln_native` take the strip-mined kernel (`pg_alignment_long_dense`, int32 blocks)?  With
        a device, 129..2048 positions, and inside the kernel's 16-bit cells: width * max(max C, gap) + 2 gap_open +
        2 gap <= 65 535 (`_native.aln_long_fits`).  Narrower operands beyond the fp16 bound keep the generic loop."""
        return (width > _native.ALN_MAX_L and _native.aln_long_ready()
                and _native.aln_long_fits(width, distance.max_cost, distance.gap, distance.gap_open))

    @staticmethod
    def _long_threshold(cmp, eps):
        """`_integer_threshold` for int32 values: the same comparison with an integer threshold, clamped to -1..2^31."""
        return int(Prograph._integer_threshold(cmp, min(max(float(eps), -1.0), float(1 << 31)), top=1 << 31))

    def _aln_staged(self, distance, X, T, k, eps, comp, similarity):
        """The frame under an `alignment` distance, for the token matrix X against itself (T None: a self graph) or the
        queries T against it, each at its own width.  Within `_aln_native`: fp16 blocks of `pg_alignment_dense`
        (`pg_alignment_affine_dense` with a gap-open penalty), int16 weights.  Beyond 128 positions inside `_aln_long`:
        int32 blocks of `pg_alignment_long_dense`, int32 weights - exact as float32 for the analytics up to 2^24, and
        the route's distances stay below 2^16.  Else None."""
        width = X.shape[1] if T is None else max(X.shape[1], T.shape[1])
        if self._aln_native(width, distance):
            kind, wdtype, operand = "f16", torch.int16, _native.aln_operand
        elif self._aln_long(width, distance):
            kind, wdtype, operand = "i32", torch.int32, _native.aln_long_operand
        else:
            return None
        xo = operand(torch.from_numpy(np.ascontiguousarray(X)), distance.symbols)
        yo = xo if T is None else operand(torch.from_numpy(np.ascontiguousarray(T)), distance.symbols)
        cost, gap, gap_open = distance.device_cost(), distance.gap, distance.gap_open
        if kind == "i32":
            dense = lambda r0, r1: _native.alignment_long_dense(xo, yo, cost, gap, gap_open, out_bytes=4, rows=(r0, r1))     # noqa: E731
        elif gap_open:
            dense = lambda r0, r1: _native.alignment_affine_dense(xo, yo, cost, gap, gap_open, out_bytes=2, rows=(r0, r1))     # noqa: E731
        else:
            dense = lambda r0, r1: _native.alignment_dense(xo, yo, cost, gap, out_bytes=2, rows=(r0, r1))     # noqa: E731
        return self._staged(xo.n, yo.n, dense, kind, wdtype, k, eps, comp, similarity, T is not None)

    def _search_alignment(self, strings, Y, k, eps, comp, similarity, representation, distance):
        """Queries under an `alignment` distance (`_aln_staged`): strings of any length up to the kernels'; dataset and
        queries keep their own widths.  None (the generic loop with the operator) when dataset or queries are not integer
        tokens of the table, or no kernel route takes the wider of the two."""
        try:
            X = self._sub_tokens(self._dataset_matrix(representation), distance)
        except (ValueError, TypeError):
            return None
        T = self._sub_tokens(self._query_tokens(strings, Y), distance) if X is not None else None
        if T is None:
            return None
        return self._aln_staged(distance, X, T, k, eps, comp, similarity)

    # ---- local and semi-global alignment scores (`_SCORES`): similarities - largest first, whatever `similarity` says; the
    # two share every route below and differ in the kernels their instances name (`_native_dense`, `_native_long_dense`)
    def _local_native(self, width, distance, width_y=None):
        """Does a width take the local alignment kernel's fp16 route?  At most 128 positions, and every score - at most
        width * max(S) - is an integer that is exact in fp16.  With `width_y`, the rows' / queries' width apart from the
        columns' `width`, the instance answers (`_f16_route`): `fit_alignment` counts its shift in."""
        if width_y is not None:
            return distance._f16_route(width, width_y)
        return width <= _native.ALN_MAX_L and width * distance.max_score <= self._LONG_MAX_L

    def _local_tokens(self, mat, distance):
        """`_sub_tokens`, with the operator's error instead of None: no generic loop ranks scores the right way round."""
        T = self._sub_tokens(mat, distance)
        if T is None:
            raise ValueError(f"{type(distance).__name__}: the tokens must be integers of the score table "
                             f"(0..{distance.symbols - 1})")
        return T

    def _local_select(self, distance, X, T, k, eps, comp):
        """The graph of `_SCORES` scores of the rows of T (all of X when T is None: a self graph) against X: ranks first..
        first+k-1 (k already clamped) of the stable descending (score, column) order, or the CSR of {(r, c): s > 0,
        comp(eps, s)} with ascending columns, a self graph without its entries c == r.  The frame in its `score` form,
        on the kernels the instance names: within `_local_native` fp16 blocks (`_native_dense`), int16 scores; beyond 128
        and up to 2048 positions, inside the instance's bound (`_i32_route`), int32 blocks (`_native_long_dense`), int32
        scores - both only within the device selection's limits (k rounds, the five orderings).  Outside them: the same
        selection in torch over the operator's int64 blocks.
        `fit_alignment` scores go below 0 and the selection kernels sort non-negative values, so such an instance names a
        shift too (`_select_bias`: K = gap_open + gap * the rows' width, minus the least score), which its kernels add to
        every entry of a block and the frame takes off again.  Its fp16 route holds while K + width * max(S) <= 2048, its
        int32 route everywhere else inside `_native.aln_fit_fits`."""
        Y, query = (X, False) if T is None else (T, True)
        n, q = X.shape[0], Y.shape[0]
        K = distance._select_bias(Y.shape[1])                                # 0 but for `fit_alignment`
        on_device = k <= _native.MAX_K_ROUNDS if k is not None else comp in _CMP_CODE
        f16 = self._local_native(X.shape[1], distance, Y.shape[1]) if K else \
            self._local_native(max(X.shape[1], Y.shape[1]), distance)
        if on_device and (f16 or distance._i32_route(X.shape[1], Y.shape[1])):
            kind, wdtype, operand, kernel, out_bytes = ("f16", torch.int16, _native.aln_operand, distance._native_dense, 2) if f16 else \
                ("i32", torch.int32, _native.aln_long_operand, distance._native_long_dense, 4)
            xo = operand(torch.from_numpy(np.ascontiguousarray(X)), distance.symbols)
            yo = xo if T is None else operand(torch.from_numpy(np.ascontiguousarray(T)), distance.symbols)
            bias = {"bias": K} if K else {}
            return self._staged(n, q, lambda r0, r1: kernel(xo, yo, out_bytes, rows=(r0, r1), **bias), kind, wdtype, k, eps, comp,
                                False, query, score=(K, query))
        dev = _native.device()
        Xd, Yd = torch.as_tensor(X, device=dev), torch.as_tensor(Y, device=dev)
        return self._score_select_torch(n, q, lambda r0, r1: distance(Xd, Yd[r0:r1]), k, eps, comp, query, dev)

    def _score_select_torch(self, n, q, scores, k, eps, comp, query, dev):
        """`_local_select`'s selection in torch over the int64 blocks `scores(r0, r1)` of the operator, for what the device
        selection does not cover."""
        first = 0 if query else 1
        rows = self._block_rows(n, q, 1 if query else 64)
        parts = []
        for r0 in range(0, q, rows):
            s = scores(r0, min(q, r0 + rows))
            if k is not None:
                o = torch.sort(s, dim=1, descending=True, stable=True)
                parts.append((o[1][:, first:first + k].to(torch.int32), o[0][:, first:first + k]))
                continue
            keep = (s > 0) & comp(eps, s)
            if not query:
                keep[torch.arange(s.shape[0], device=dev), torch.arange(r0, r0 + s.shape[0], device=dev)] = False
            loc = torch.where(keep)
            indptr = torch.zeros(s.shape[0] + 1, dtype=torch.int64, device=dev)
            indptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
            parts.append((indptr, loc[1].to(torch.int32), s[loc]))
        if k is not None:
            return KNNGraph(torch.cat([p_[0] for p_ in parts]), torch.cat([p_[1] for p_ in parts]), n, similarity=False, first=first)
        return CSRGraph(*_native.cat_csr(parts), n, similarity=False)

    @staticmethod
    def _drop_diagonal(indptr, indices, wts):
        """A square CSR without its entries (r, r), on the device."""
        n = indptr.numel() - 1
        rows = torch.repeat_interleave(torch.arange(n, device=indptr.device), indptr[1:] - indptr[:-1])
        keep = indices != rows
        out = torch.zeros_like(indptr)
        out[1:] = torch.cumsum(torch.bincount(rows[keep], minlength=n), 0)
        return out, indices[keep], wts[keep]

    @staticmethod
    def _unshift(indptr, indices, wts, K, diagonal):
        """A CSR selected from blocks shifted by K: the scores themselves, the entries s <= 0 dropped - the selection's own
        `> 0` test saw s + K - and, when `diagonal` is False, the entries (r, r) too; on the device, as `_drop_diagonal`."""
        n = indptr.numel() - 1
        rows = torch.repeat_interleave(torch.arange(n, device=indptr.device), indptr[1:] - indptr[:-1])
        wts = wts - K
        keep = wts > 0
        if not diagonal:
            keep &= indices != rows
        out = torch.zeros_like(indptr)
        out[1:] = torch.cumsum(torch.bincount(rows[keep], minlength=n), 0)
        return out, indices[keep], wts[keep]

    def _search_local(self, strings, Y, k, eps, comp, similarity, representation, distance):
        """Queries under a score of `_SCORES`: `k` -> ranks 0..min(k, N)-1 of the stable descending (score, dataset row)
        order; `eps` -> per query the dataset rows with s > 0 and comp(eps, s), ascending.  Dataset and queries keep their
        own widths, as in `_search_alignment`.  `similarity` is not consulted.  The weights are the scores."""
        X = self._local_tokens(self._dataset_matrix(representation), distance)
        T = self._local_tokens(self._query_tokens(strings, Y), distance)
        return self._local_select(distance, X, T, None if k is None else min(k, X.shape[0]), eps, comp)

    def _search_profile(self, queries, k, eps, comp, representation, distance):
        """Profiles as queries under a `profile_alignment`: the contract of `_search_local` - `k` -> ranks 0..min(k, N)-1 of
        the stable descending (score, dataset row) order, `eps` -> the rows with s > 0 and comp(eps, s), ascending, the weights
        the scores - on the routes of `_local_select`: fp16 blocks of `pg_alignment_profile_dense` up to 128 positions while
        the shifted values stay within 0..2048 (`_f16_route`), int32 blocks of `pg_alignment_profile_long_dense` beyond
        (`_i32_route`), fit scores shifted by `_select_bias` and taken back by the frame; outside the device selection's
        limits, and without a device, the same selection in torch over the operator's int64 blocks."""
        prof = Profiles(queries)
        X = self._sub_tokens(self._dataset_matrix(representation), prof)
        if X is None:
            raise ValueError(f"profile_alignment: the tokens must be integers of the profiles' symbols (0..{prof.symbols - 1})")
        n, q, wx, wy = X.shape[0], len(prof), X.shape[1], prof.width
        k = None if k is None else min(k, n)
        device = _native.aln_long_ready()
        on_device = device and (k <= _native.MAX_K_ROUNDS if k is not None else comp in _CMP_CODE)
        f16 = on_device and distance._f16_route(wx, wy, prof.top)
        if f16 or (on_device and distance._i32_route(wx, wy, prof.top)):
            K = distance._select_bias(wy)
            kind, wdtype, operand, kernel, out_bytes = ("f16", torch.int16, _native.aln_operand, distance._native_dense, 2) if f16 else \
                ("i32", torch.int32, _native.aln_long_operand, distance._native_long_dense, 4)
            xo = operand(torch.from_numpy(np.ascontiguousarray(X)), prof.symbols)
            po = _native.profile_operand(prof.list)
            return self._staged(n, q, lambda r0, r1: kernel(xo, po, out_bytes, rows=(r0, r1), bias=K), kind, wdtype, k, eps, comp,
                                False, True, score=(K, True))
        dev = _native.device() if device else torch.device("cpu")
        Xd = torch.as_tensor(X, device=dev)
        return self._score_select_torch(n, q, lambda r0, r1: distance(Xd, prof.list[r0:r1]), k, eps, comp, True, dev)

    _PROFILE_QUERIES_ONLY = ("{}: a profile_alignment scores profiles, and profiles are queries only: pass them to "
                             "search(profiles, k= | eps=, distance=...)")

    def _build_graph_local(self, idxs, eps, k, similarity, representation, comp, distance, cap=None):
        """
        `build_graph(distance=local_alignment(S, gap[, gap_open]))`, `semiglobal_alignment(...)` or `fit_alignment(...)`.
        Such a score is a similarity, so the graph ranks largest first and `similarity` is not consulted; the weights are
        the raw scores (the containers are built with similarity=False, so nothing turns them into 1/(1+w)).
        k: ranks 1..k of the stable descending (score, column) order; rank 0 is dropped, as the reference drops it for
        every distance (:761-763) - it is the row itself unless a row of lower index contains it.  eps: the reference's
        similarity form (:734) - the edges {(r, c): c != r, s > 0, comp(eps, s)}, so the default comp reads s >= eps -
        with ascending columns.  The routes are `_local_select`'s.  Returns a KNNGraph / CSRGraph.
        """
        if k is not None and k < 1:
            raise ValueError("K must be at least 1.")
        mat = np.asarray(self._dataset_matrix(representation))
        if idxs is not None:
            mat = mat[np.asarray(idxs)]
        T = self._local_tokens(mat, distance)
        n = T.shape[0]
        if k and not min(k, n - 1):                                          # int16 whichever route would have run
            return self._empty_knn(n, torch.int16, _native.device(), False)
        return self._local_select(distance, T, None, min(k, n - 1) if k else None, eps, comp)

    # ---- alignment tracebacks (prograph_amd/alignments.py)
    def _edge_lists(self, graph):
        """(rows, columns) int64 numpy of the edges of a CSRGraph, a KNNGraph, a stored graph's name or a list of
        (indices, weights) tuples, in the graph's order, `row0` added to the rows; kNN slots without a neighbour (-1) are
        no edges."""
        if isinstance(graph, str):
            g = self._device_graph_any(graph)
            if g is None:
                indptr, indices, _ = self._column_csr(graph)
                return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr)), np.asarray(indices, dtype=np.int64)
            graph = g
        if isinstance(graph, KNNGraph):
            graph = graph.as_csr()
        if isinstance(graph, CSRGraph):
            indptr, c = graph.indptr.cpu().numpy(), graph.indices.cpu().numpy().astype(np.int64)
            r = np.repeat(np.arange(graph.nrows, dtype=np.int64) + graph.row0, np.diff(indptr))
            return r[c >= 0], c[c >= 0]
        if isinstance(graph, (list, tuple)) and all(isinstance(e, tuple) and len(e) == 2 for e in graph):
            counts = np.fromiter((len(e[0]) for e in graph), dtype=np.int64, count=len(graph))
            c = np.concatenate([np.asarray(e[0], dtype=np.int64) for e in graph]) if counts.sum() else np.zeros(0, dtype=np.int64)
            return np.repeat(np.arange(len(graph), dtype=np.int64), counts), c
        raise TypeError("align: graph must be a CSRGraph, a KNNGraph, the name of a stored graph or a list of (indices, weights) tuples")

    def _edge_queries(self, queries, distance):
        """What `search` was given, as the token matrix whose rows a search result's rows name (`align`, `rescore`)."""
        if isinstance(queries, str) or (isinstance(queries, (list, tuple)) and len(queries)
                                        and all(isinstance(q, str) for q in queries)):
            raw, table = self._byte_view([queries] if isinstance(queries, str) else list(queries))
            Q = table[raw]
        else:
            Q = queries.cpu().numpy() if isinstance(queries, torch.Tensor) else np.asarray(queries)
            Q = Q.reshape(1, -1) if Q.ndim == 1 else Q
        return self._local_tokens(Q, distance)

    def align(self, graph=None, rows=None, cols=None, queries=None, idxs=None, distance=None, representation="Tokenized",
              workspace_bytes=None, ops=True):
        """
        The canonical optimal alignments (`Alignments`, prograph_amd/alignments.py) of dataset pairs under
        `distance`, which must be an `alignment`, `local_alignment`, `semiglobal_alignment` or `fit_alignment` instance (`TypeError`
        otherwise): which residues pair, where a fragment sits in its parent, how many columns are identical.
        `graph`: a `CSRGraph`, a `KNNGraph`, a stored graph's name or the tuple list `build_graph` returns - one alignment
        per edge in the graph's order, x the edge's row (`row0` honoured) and y its column; with `idxs`, the row selection
        the graph was built over, both go through it.  `rows=` / `cols=`: explicit dataset pairs instead of a graph.
        `queries=` (what `search` was given): the graph is a `search` result, x is the query and y the dataset row.
        At most 128 positions run on the HIP kernel `pg_alignment_trace`, wider data and queries up to 2048 positions on
        `pg_alignment_trace_long` (either: one host sync for the index check, launches split so that their waves' shares
        fit `workspace_bytes`; None: 256 MiB for the first, what the edges need up to 2 GiB for the second); beyond 2048
        positions, or without a device, the exact, slow host expression.
        A `fit_alignment` instance is asymmetric - the edge's row, or the query, is aligned WHOLE within its column - and
        the tracer's x is the sequence with the free ends, so there x is the edge's COLUMN and y its row or query:
        `tb.x_*` speak of the containing dataset sequence (`x_begin:x_end` is where the row sits in it), `tb.y_*` of the
        fitted one (`y_begin` = 0, `y_end` = its length), and `tb.score` equals the edge's weight.
        `ops=False`: the same seven fields per edge without the columns (`tb.ops` is None, `cigar` / `gapped` raise) - what
        an identity cut needs.  At most 128 positions that is `pg_alignment_stats`, a forward pass that stores and walks
        nothing (32 bytes per edge, no workspace); 129..2048 positions the strip kernel in slices of the edge list with
        one ops buffer of at most 256 MiB.
        """
        if isinstance(distance, profile_alignment):                         # no traceback against a profile
            raise ValueError(self._PROFILE_QUERIES_ONLY.format("align"))
        mode = _alignments._mode_of(distance)                               # TypeError for anything else
        X = self._local_tokens(self._dataset_matrix(representation), distance)
        if graph is not None:
            if rows is not None or cols is not None:
                raise ValueError("align: a graph or rows= / cols=, not both")
            r, c = self._edge_lists(graph)
        elif rows is not None and cols is not None:
            r, c = np.asarray(rows, dtype=np.int64).reshape(-1), np.asarray(cols, dtype=np.int64).reshape(-1)
            if len(r) != len(c):
                raise ValueError("align: rows= and cols= must have one length")
        else:
            raise ValueError("align: give a graph, or rows= and cols=")
        if idxs is not None:
            idxs = np.arange(len(self))[idxs] if isinstance(idxs, slice) else np.asarray(idxs)
            idxs = np.nonzero(idxs)[0] if idxs.dtype == bool else idxs.astype(np.int64)
            c = idxs[c]
            if queries is None:
                r = idxs[r]
        if queries is None:
            Q = X
        else:
            Q = self._edge_queries(queries, distance)
        if len(r) and (r.min() < 0 or r.max() >= Q.shape[0] or c.min() < 0 or c.max() >= X.shape[0]):
            raise IndexError("align: an edge names a row outside the data")
        letters = "?" + "".join(self.amino_acids) if all(len(a) == 1 for a in self.amino_acids) else None
        dev = _native.device() if _native.aln_long_ready() else torch.device("cpu")
        Xt = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        Qt = Xt if Q is X else torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
        width = max(X.shape[1], Q.shape[1])
        native = _native.aln_long_ready() and width <= _native.ALN_MAX_L
        native_long = _native.aln_trace_long_ready() and _native.ALN_MAX_L < width <= _native.ALN_LONG_MAX_L
        if mode == _alignments.FIT:                                         # the tracer's x has the free ends: the column
            return _alignments.trace(distance, Xt, Qt, torch.from_numpy(c), torch.from_numpy(r), workspace_bytes=workspace_bytes,
                                     letters=letters, native=native, native_long=native_long, ops=ops)
        return _alignments.trace(distance, Qt, Xt, torch.from_numpy(r), torch.from_numpy(c), workspace_bytes=workspace_bytes,
                                 letters=letters, native=native, native_long=native_long, ops=ops)

    # ---- filter and refine: the alignment values of candidate edges
    def _candidate_csr(self, graph):
        """A candidate graph - what `_edge_lists` takes - as CSR tensors where the graph lives (a device graph stays on the
        device): (indptr int64 [nrows + 1], columns int64, row0).  kNN slots without a neighbour (-1) are no edges."""
        if isinstance(graph, str):
            graph = self._device_graph_any(graph) or graph
        if isinstance(graph, KNNGraph):
            graph = graph.as_csr()
        if isinstance(graph, CSRGraph):
            indptr, c = graph.indptr.to(torch.int64), graph.indices.to(torch.int64)
            real = c >= 0
            if not bool(real.all()):
                rows = torch.repeat_interleave(torch.arange(graph.nrows, device=c.device), indptr[1:] - indptr[:-1])
                indptr = torch.zeros_like(indptr)
                indptr[1:] = torch.cumsum(torch.bincount(rows[real], minlength=graph.nrows), 0)
                c = c[real]
            return indptr, c, graph.row0
        r, c = self._edge_lists(graph)                                      # a name without a device graph, a tuple list
        nrows = len(self) if isinstance(graph, str) else len(graph)
        if len(r) and (r.min() < 0 or r.max() >= nrows or np.any(np.diff(r) < 0)):
            raise ValueError("rescore: the graph's edges must come row by row")
        indptr = np.zeros(nrows + 1, dtype=np.int64)
        indptr[1:] = np.cumsum(np.bincount(r, minlength=nrows))
        return torch.from_numpy(indptr), torch.from_numpy(c), 0

    @staticmethod
    def _rescore_knn_torch(rs, cs, ss, indptr, nrows, k, descending):
        """`rescore`'s kNN selection in torch: edges (rs, cs, ss) sorted by (row, column) -> (idx, w) (nrows, k), per row the
        first k of the stable (value, column) order, -1 / 0 beyond a row's candidates."""
        dev = ss.device
        by_value = torch.sort(ss, stable=True, descending=descending)[1]
        order = by_value[torch.sort(rs[by_value], stable=True)[1]]         # by (row, value, column)
        rank = torch.arange(order.numel(), device=dev) - indptr[rs]       # rs is sorted: the sorted rows are rs itself
        keep = rank < k
        idx = torch.full((nrows, k), -1, dtype=torch.int32, device=dev)
        w = torch.zeros((nrows, k), dtype=torch.int32, device=dev)
        idx[rs[keep], rank[keep]] = cs[order][keep].to(torch.int32)
        w[rs[keep], rank[keep]] = ss[order][keep]
        return idx, w

    def _rescore_select_device(self, rs, cs, ss, indptr, indptr_host, nrows, k, eps, cmp, K, keep_zero, descending):
        """`rescore`'s selection on the int32 selection kernels: (rows, P) blocks whose columns are a row's candidates in
        column order - so that a tie of positions is a tie of columns -, P the longest list (k if that is more), the rest of
        a row padded with what takes no rank from an edge (behind the edges a tie goes to the edge: 0 under largest first,
        2^31 - 1 under smallest first; -1, which no radius admits).  Values are shifted by K >= 0 (`fit_alignment`: the
        blocks of `_local_select`).  Selected positions go back to columns by a gather; a position past its row's list is
        no neighbour.  Returns (idx, w) or the CSR triple."""
        dev = ss.device
        lens_host = np.diff(indptr_host)
        lens = indptr[1:] - indptr[:-1]
        P = max(int(lens_host.max()) if nrows else 1, k or 1, 1)
        pos = torch.arange(ss.numel(), device=dev) - indptr[rs]
        pad = -1 if k is None else (0 if descending else (1 << 31) - 1)
        per = max(1, self._BLOCK_ELEMS // 2 // P)
        parts = []
        for r0 in range(0, nrows, per):
            r1 = min(nrows, r0 + per)
            e0, e1 = int(indptr_host[r0]), int(indptr_host[r1])
            block = torch.full((r1 - r0, P), pad, dtype=torch.int32, device=dev)
            block[rs[e0:e1] - r0, pos[e0:e1]] = ss[e0:e1] + K
            base, ln = indptr[r0:r1], lens[r0:r1]
            if k is not None:
                at, w = _native.i32_knn(block, k, first=0, descending=descending)
                at = at.to(torch.int64)
                real = (at >= 0) & (at < ln[:, None])
                col = cs[(base[:, None] + at.clamp(min=0)).clamp(max=max(cs.numel() - 1, 0))] if cs.numel() else at
                parts.append((torch.where(real, col, torch.full_like(col, -1)).to(torch.int32),
                              torch.where(real, w - K, torch.zeros_like(w))))
                continue
            ip, at, w = _native.i32_eps(block, cmp, self._long_threshold(cmp, float(eps) + K), keep_zero=keep_zero)
            at = at.to(torch.int64)
            rows = torch.repeat_interleave(torch.arange(r1 - r0, device=dev), ip[1:] - ip[:-1])
            w = w - K
            real = at < ln[rows]
            if K:
                real &= w > 0
            out = torch.zeros_like(ip)
            out[1:] = torch.cumsum(torch.bincount(rows[real], minlength=r1 - r0), 0)
            parts.append((out, cs[base[rows[real]] + at[real]].to(torch.int32), w[real]))
        if k is not None:
            return torch.cat([p_[0] for p_ in parts]), torch.cat([p_[1] for p_ in parts])
        return _native.cat_csr(parts)

    def rescore(self, graph, distance, k=None, eps=None, comp=operator.le, queries=None, idxs=None,
                representation="Tokenized", output="csr", store=None):
        """
        The REFINE half of filter-and-refine: the edges of a candidate graph scored with an alignment operator, and the best
        of every row kept.  `graph`: a `CSRGraph`, a `KNNGraph`, a stored graph's name or a tuple list, read as `align`
        reads it (`row0` honoured, kNN slots of -1 are no edges; with `idxs`, the selection the graph was built over, rows
        and columns go through it; with `queries`, what `search` was given, the rows are the queries).  `distance`: an
        `alignment`, `local_alignment`, `semiglobal_alignment` or `fit_alignment` instance (`TypeError` otherwise; a
        `profile_alignment` raises the queries-only `ValueError`).  Every edge (r, c) gets the operator's value
        `distance(T, T[r:r+1])[0, c]` (with `queries` the query row against T; `fit_alignment`: the row or query whole,
        within column c, as in `build_graph`).
        Neither `k` nor `eps`: a `CSRGraph` of the same edges in the same order with int32 weights.  `k`: a `KNNGraph` with
        int32 values - per row the first k candidates of the stable (value, column) order, largest first for the scores,
        smallest first for `alignment`; idx -1, weight 0 where a row has fewer than k candidates (built with first=1, with
        `queries` first=0).  `eps`: a `CSRGraph` with ascending columns under `build_graph`'s contract - distances
        `comp(d, eps) & d > 0`, scores `s > 0 & comp(eps, s)` - or with `queries` under `search`'s, which keeps d = 0.
        Nothing is dropped on its own: an edge c == r is scored like any other.  `output="tuples"` and `store=` as in
        `build_graph`.
        Exact within the candidates, approximate as a graph: an edge the candidate graph lacks is never found.
        On the device, at up to 128 positions and for `fit_alignment` inside its 16-bit bound, the values come from
        `pg_alignment_list_scores` - the dense kernels' row routines over the edge list, one launch - and the selection
        from the int32 selection kernels over (rows, longest list) blocks.  At 129..2048 positions, inside the mode's
        16-bit bound (`aln_long_fits`, `aln_local_long_fits`, `aln_semiglobal_long_fits`, `aln_fit_fits`), the values come
        from `pg_alignment_list_long_scores` - the long dense kernels' strip routines over the edge list - and the
        selection is the same.  Wider operands still, a mode outside its bound, a `comp` outside the five orderings, k
        beyond the selection's rounds, or no device: the scores of `align(..., ops=False)` and the same selection in torch
        - the same graph.
        """
        if isinstance(distance, profile_alignment):
            raise ValueError(self._PROFILE_QUERIES_ONLY.format("rescore"))
        mode = _alignments._mode_of(distance)                               # TypeError for anything else
        if k is not None and eps is not None:
            raise ValueError("rescore: k or eps, not both")
        if k is not None and (isinstance(k, bool) or not isinstance(k, (int, np.integer))):
            raise TypeError("K must be provided as an integer.")
        if k is not None and k < 1:
            raise ValueError("K must be at least 1.")
        if eps is not None and (isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating))):
            raise TypeError("Epsilon must be provided as a number.")
        if eps is not None and eps != eps:
            raise ValueError("Epsilon must not be NaN.")
        k = None if k is None else int(k)
        X = self._local_tokens(self._dataset_matrix(representation), distance)
        if idxs is not None:
            idxs = np.arange(len(self))[idxs] if isinstance(idxs, slice) else np.asarray(idxs)
            idxs = np.nonzero(idxs)[0] if idxs.dtype == bool else idxs.astype(np.int64)
            X = X[idxs]
        indptr, cols, row0 = self._candidate_csr(graph)
        indptr_host = indptr.cpu().numpy()
        nrows, n, query = len(indptr_host) - 1, X.shape[0], queries is not None
        Q = self._edge_queries(queries, distance) if query else X
        if row0 < 0 or row0 + nrows > Q.shape[0] or (cols.numel() and (int(cols.min()) < 0 or int(cols.max()) >= n)):
            raise IndexError("rescore: an edge names a row outside the data")
        whole = not query and row0 == 0 and nrows == n
        Y = Q if whole else Q[row0:row0 + nrows]
        score = mode != _alignments.GLOBAL
        width = max(X.shape[1], Y.shape[1])
        kernel = (_native.aln_list_ready() and nrows > 0 and width <= _native.ALN_MAX_L
                  and (mode != _alignments.FIT
                       or _native.aln_fit_fits(X.shape[1], Y.shape[1], distance.max_score, distance.gap, distance.gap_open)))
        # 129..2048 positions: the long list kernel, inside the mode's own 16-bit bound (the long dense kernels')
        long = (nrows > 0 and _native.ALN_MAX_L < width <= _native.ALN_LONG_MAX_L and _native.aln_list_long_ready()
                and (_native.aln_long_fits(width, distance.max_cost, distance.gap, distance.gap_open) if mode == _alignments.GLOBAL
                     else distance._long_fits(X.shape[1], Y.shape[1])))
        selects = k <= _native.MAX_K_ROUNDS if k is not None else (eps is None or comp in _CMP_CODE)
        fast = (kernel or long) and selects
        if fast:
            dev = _native.device()
            operand, scores = (_native.aln_long_operand, _native.alignment_list_long_scores) if long else \
                (_native.aln_operand, _native.alignment_list_scores)
            xo = operand(torch.from_numpy(np.ascontiguousarray(X)), distance.symbols)
            yo = xo if whole else operand(torch.from_numpy(np.ascontiguousarray(Y)), distance.symbols)
            indptr, cols = indptr.to(dev), cols.to(dev)
            ss = scores(xo, yo, indptr, cols.to(torch.int32), mode, _alignments._device_table(distance, mode), distance.gap,
                        distance.gap_open)
        else:
            g0 = CSRGraph(indptr.cpu(), cols.cpu().to(torch.int32), torch.zeros(cols.numel(), dtype=torch.int32), n, row0=row0)
            tb = self.align(g0, queries=queries, idxs=idxs, distance=distance, representation=representation, ops=False)
            ss = tb.score.to(torch.int32)
            dev = ss.device
            indptr, cols = indptr.to(dev), cols.to(dev)
        if k is None and eps is None:
            g = CSRGraph(indptr, cols.to(torch.int32), ss, n, similarity=False, row0=row0)
            return self._graph_result(g, idxs, store, None, output)
        rs = torch.repeat_interleave(torch.arange(nrows, device=dev), indptr[1:] - indptr[:-1])
        order = torch.sort(rs * n + cols, stable=True)[1]                   # a row's candidates in column order
        cs, ss = cols[order], ss[order]
        K = distance._select_bias(Y.shape[1]) if score else 0               # 0 but for `fit_alignment`
        if k is not None:
            idx, w = self._rescore_select_device(rs, cs, ss, indptr, indptr_host, nrows, k, None, None, K, False, score) if fast \
                else self._rescore_knn_torch(rs, cs, ss, indptr, nrows, k, score)
            g = KNNGraph(idx, w, n, similarity=False, row0=row0, first=0 if query else 1)
        else:
            if fast:
                cmp = _CMP_MIRROR[_CMP_CODE[comp]] if score else _CMP_CODE[comp]
                csr = self._rescore_select_device(rs, cs, ss, indptr, indptr_host, nrows, None, eps, cmp, K,
                                                  bool(K) if score else query, score)
            else:
                keep = ((ss > 0) & comp(eps, ss)) if score else (comp(ss, eps) & ((ss > 0) | query))
                out = torch.zeros_like(indptr)
                out[1:] = torch.cumsum(torch.bincount(rs[keep], minlength=nrows), 0)
                csr = (out, cs[keep].to(torch.int32), ss[keep])
            g = CSRGraph(*csr, n, similarity=False, row0=row0)
        return self._graph_result(g, idxs, store, None, output)

    _GRAPH_TYPES = (CSRGraph, KNNGraph, str, list, tuple)                   # what `candidates=` takes for a ready graph

    @staticmethod
    def _pool_checked(who, candidates, pool, k):
        """The checks of `candidates=` / `pool=` (`build_graph`, `search`): True when `candidates` is a ready graph."""
        if candidates is None:
            raise ValueError(f"{who}: pool= goes with candidates=")
        if isinstance(candidates, Prograph._GRAPH_TYPES):
            if pool is not None:
                raise ValueError(f"{who}: candidates= is a graph already, pool= must be None")
            return True
        if pool is None:
            raise ValueError(f"{who}: candidates= is a distance, so pool= (candidates per row) must be given")
        if isinstance(pool, bool) or not isinstance(pool, (int, np.integer)):
            raise TypeError(f"{who}: pool must be an integer")
        if k is not None and isinstance(k, (int, np.integer)) and pool < k:
            raise ValueError(f"{who}: pool must be at least k")
        if not 1 <= pool <= _native.MAX_K_ROUNDS:
            raise ValueError(f"{who}: pool must be in max(k, 1)..{_native.MAX_K_ROUNDS}")
        return False

    def _build_graph_candidates(self, idxs, eps, k, similarity, representation, distance, comp, output, store, candidates, pool):
        """`build_graph(candidates=, pool=)`: the pool per row - `build_graph(k=pool, distance=candidates)` over the same
        `idxs` and `representation`, or a ready graph -, without its entries c == r, through `rescore`."""
        if similarity:
            raise ValueError("build_graph: candidates= ranks the values of an alignment operator; similarity=True has no meaning there")
        if isinstance(distance, profile_alignment):
            raise ValueError(self._PROFILE_QUERIES_ONLY.format("build_graph"))
        _alignments._mode_of(distance)                                      # TypeError for anything but the four operators
        if operator.xor(bool(eps), bool(k)) is False:
            raise ValueError("Epsilon or K must be provided, but both cannot be as they are different methods of graph construction.")
        if not self._pool_checked("build_graph", candidates, pool, k):
            candidates = self.build_graph(idxs=idxs, k=int(pool), distance=candidates, representation=representation, output="csr")
        indptr, c, row0 = self._candidate_csr(candidates)
        nrows = indptr.numel() - 1
        r = torch.repeat_interleave(torch.arange(nrows, device=c.device), indptr[1:] - indptr[:-1])
        keep = c != r + row0
        kept = torch.zeros_like(indptr)
        kept[1:] = torch.cumsum(torch.bincount(r[keep], minlength=nrows), 0)
        ncols = candidates.ncols if isinstance(candidates, (CSRGraph, KNNGraph)) else len(self) if idxs is None else \
            len(np.arange(len(self))[idxs] if isinstance(idxs, slice) else
                (np.nonzero(idxs)[0] if np.asarray(idxs).dtype == bool else np.asarray(idxs)))
        pool_graph = CSRGraph(kept, c[keep].to(torch.int32), torch.zeros(int(kept[-1]), dtype=torch.int32, device=c.device), ncols,
                              row0=row0)
        return self.rescore(pool_graph, distance, k=k, eps=eps if eps else None, comp=comp, idxs=idxs, representation=representation,
                            output=output, store=store)

    def _search_candidates(self, queries, k, eps, comp, similarity, representation, distance, output, candidates, pool):
        """`search(candidates=, pool=)`: the pool per query - `search(k=pool, distance=candidates)`, or a ready graph -
        through `rescore(queries=)`."""
        if similarity:
            raise ValueError("search: candidates= ranks the values of an alignment operator; similarity=True has no meaning there")
        if isinstance(distance, profile_alignment):
            raise ValueError(self._PROFILE_QUERIES_ONLY.format("search(candidates=)"))
        _alignments._mode_of(distance)
        if (k is None) == (eps is None):
            raise ValueError("Epsilon or K must be provided, but both cannot be as they are different methods of graph construction.")
        if not self._pool_checked("search", candidates, pool, k):
            candidates = self.search(queries, k=int(pool), distance=candidates, representation=representation, output="csr")
        return self.rescore(candidates, distance, k=k, eps=eps, comp=comp, queries=queries, representation=representation,
                            output=output)

    # ---- percent-identity cuts of a graph's edges
    @staticmethod
    def _identity_cut_asked(who, distance, min_identity, min_columns):
        """False for the defaults (nothing changes); else the checks of `min_identity=` / `min_columns=`."""
        if min_identity is None and not min_columns:
            return False
        if isinstance(distance, profile_alignment):
            raise ValueError(Prograph._PROFILE_QUERIES_ONLY.format(f"{who}(min_identity= / min_columns=)"))
        _alignments._mode_of(distance)                                      # TypeError for anything but the four operators
        if min_identity is not None and not 0 <= float(min_identity) <= 1:
            raise ValueError(f"{who}: min_identity must be in 0..1")
        if int(min_columns) != min_columns or min_columns < 0:
            raise ValueError(f"{who}: min_columns must be a non-negative integer")
        return True

    def _identity_cut(self, g, distance, min_identity, min_columns, representation, queries=None, idxs=None):
        """The edges of `g` (a CSRGraph, a KNNGraph or a tuple list over `ncols` = the dataset or selection) whose canonical
        alignment has at least `min_columns` columns and, with a threshold, `identities / max(n_ops, 1) >= min_identity`
        in float64 on the alignments' device: a CSRGraph of the survivors in their order with their weights.  Every edge
        is aligned with `ops=False`; `indptr` comes from the mask's cumulative sum, no row is visited by Python."""
        if isinstance(g, KNNGraph):
            g = g.as_csr()
        elif not isinstance(g, CSRGraph):                                   # the generic loop's tuple list
            counts = np.fromiter((len(e[0]) for e in g), dtype=np.int64, count=len(g))
            cat = lambda k, dt: np.concatenate([np.asarray(e[k]) for e in g]) if counts.sum() else np.zeros(0, dtype=dt)
            ncols = len(self) if idxs is None else len(idxs)
            g = CSRGraph(torch.from_numpy(np.concatenate([[0], np.cumsum(counts)])), torch.from_numpy(cat(0, np.int64)).to(torch.int32),
                         torch.from_numpy(cat(1, np.float32)), ncols, final=True)
        tb = self.align(g, queries=queries, idxs=idxs, distance=distance, representation=representation, ops=False)
        dev = g.indptr.device
        n_ops = tb.n_ops.to(dev)
        keep = n_ops >= int(min_columns)
        if min_identity is not None:
            keep &= tb.identities.to(dev).double() / n_ops.double().clamp(min=1) >= float(min_identity)
        mask = g.indices >= 0                                               # kNN slots without a neighbour are no edges
        mask[mask.clone()] = keep
        before = torch.zeros(g.nnz + 1, dtype=torch.int64, device=dev)
        before[1:] = torch.cumsum(mask, 0)
        return CSRGraph(before[g.indptr], g.indices[mask], g.weights[mask], g.ncols, similarity=g.similarity, row0=g.row0,
                        final=g.final)

    # ---- radius (eps) search: a CSRGraph with one row per query, d = 0 kept
    def _search_eps_embedding(self, Y, eps, comp, similarity, representation, distance):
        """Minkowski / cosine / Euclidean queries on the fused eps kernels with d = 0 (s = 1) kept; fewer than `_MINK_STAGED_ROWS`
        Minkowski queries take the dense block + fp16 selection, which gives the same CSR bit for bit.  None (the
        generic loop) as in `_search_embedding`."""
        ops = self._embedding_operands(Y, representation)
        if ops is None:
            return None
        return self._search_eps_embedding_staged(*ops, eps, comp, similarity, distance)

    def _search_eps_embedding_staged(self, X, Y, eps, comp, similarity, distance):
        """`_search_eps_embedding` from the staged operands on: X (N, D) and Y (Q, D) fp16 device tensors."""
        n, cmp = X.shape[0], _CMP_CODE[comp]
        if similarity:
            eps = 1 / (1 + eps)                                          # :720-721
        if distance is minkowski:
            xp = _native.pack_f16(X)
            if Y.shape[0] < self._MINK_STAGED_ROWS:
                return self._mink_staged(xp, Y, None, eps, comp, similarity)
            indptr, indices, wts = _native.minkowski_eps(xp, _native.pack_f16(Y), cmp, eps, similarity=similarity,
                                                         keep_zero=True)
            return CSRGraph(indptr, indices, wts, n, similarity=similarity)
        xc, yc = _native.cosine_prep(X), _native.cosine_prep(Y)
        if xc.nonfinite() or yc.nonfinite():
            return None
        sweep = getattr(_native, _EMBED_F32[distance] + "_eps")
        indptr, indices, wts = sweep(xc, yc, cmp, eps, similarity=similarity, keep_zero=True)
        return CSRGraph(indptr, indices, wts, n, similarity=similarity, final=True)

    def _search_eps_generic(self, strings, Y, eps, comp, similarity, representation, distance):
        """Any `distance(X, Y, similarity=...) -> (Q, N)` operator and any `comp`: `_search_generic`'s staging, the queries
        in row blocks, `torch.where(comp(d, eps))` (similarities: `comp(1/(1+eps), s)`), no pair excluded.  The
        weights are the operator's values as they are."""
        dev = _native.device()
        X = torch.as_tensor(np.vstack(self(representation)), dtype=torch.float16, device=dev)
        if strings is not None:
            Y = self.tokenize(strings)
        Y = torch.as_tensor(Y if isinstance(Y, torch.Tensor) else np.asarray(Y), dtype=torch.float16, device=dev)
        n = X.shape[0]
        if similarity:
            eps = 1 / (1 + eps)
        rows = max(1, min(Y.shape[0], (1 << 26) // max(n, 1)))
        parts = []
        for r0 in range(0, Y.shape[0], rows):
            d = distance(X, Y[r0:r0 + rows], similarity=similarity)
            keep = comp(eps, d) if similarity else comp(d, eps)
            loc = torch.where(keep)
            indptr = torch.zeros(d.shape[0] + 1, dtype=torch.int64, device=d.device)
            indptr[1:] = torch.cumsum(torch.bincount(loc[0], minlength=d.shape[0]), 0)
            parts.append((indptr, loc[1].to(torch.int32), d[loc]))
        indptr, indices, wts = _native.cat_csr(parts)
        return CSRGraph(indptr, indices, wts, n, similarity=similarity, final=True)

    def _search_generic(self, strings, Y, k, similarity, representation, distance, output):
        """Any `distance(X, Y, similarity=...) -> (Q, N)` operator: `_build_graph_generic`'s fp16 staging on the GPU, the
        queries in row blocks, a stable sort, ranks 0..min(k, N)-1."""
        dev = _native.device()
        X = torch.as_tensor(np.vstack(self(representation)), dtype=torch.float16, device=dev)
        if strings is not None:
            Y = self.tokenize(strings)
        Y = torch.as_tensor(Y if isinstance(Y, torch.Tensor) else np.asarray(Y), dtype=torch.float16, device=dev)
        n = X.shape[0]
        kk = min(k, n)
        rows = max(1, min(Y.shape[0], (1 << 26) // max(n, 1)))
        idx, wts = [], []
        for r0 in range(0, Y.shape[0], rows):
            s = torch.sort(distance(X, Y[r0:r0 + rows], similarity=similarity), dim=1, descending=bool(similarity), stable=True)
            idx.append(s[1][:, :kk])
            wts.append(s[0][:, :kk])
        idx, wts = torch.cat(idx), torch.cat(wts)
        if output == "csr":
            return KNNGraph(idx.to(torch.int32), wts, n, similarity=similarity, final=True, first=0)
        idx, wts = idx.cpu().numpy(), wts.cpu().numpy()
        return list(zip(list(idx), list(wts)))

    @staticmethod
    def get_every_n(a, n=2):
        for start in range(0, a.shape[0], n):
            yield a[start:start + n]

    @staticmethod
    def prod_neighbours(index, out, batch_size, weights=None):
        """COO of one batch -> {row: (cols, weights)} (reference :626-654); only the generic path needs it."""
        row, col = out
        row = row + index * batch_size
        if weights is None:
            weights = np.ones(col.shape)
        result = {}
        if len(row):
            cuts = np.nonzero(np.diff(row))[0] + 1          # rows arrive grouped and ascending from where()
            for r, c, w in zip(row[np.r_[0, cuts]], np.split(col, cuts), np.split(weights, cuts)):
                result[r] = (c, w)
        return result

    # ------------------------------------------------------------------ graph construction
    def build_graph(self, idxs=None, batch_size=8, eps=None, k=None, weighted=False, similarity=False,
                    representation="Tokenized", distance=hamming, comp=operator.le, output="tuples", cap=256,
                    store=None, _keep=None, min_identity=None, min_columns=0, candidates=None, pool=None):
        """
        epsilon-neighbourhood (`eps`) or kNN (`k`) graph over all pairwise distances
        (reference :656-765).  Returns the reference's list of N `(indices, weights)` tuples;
        `output="csr"` returns the device-resident `CSRGraph` / `KNNGraph` instead (no per-row
        Python objects — what large N wants).  `batch_size` is accepted for compatibility: the
        HIP path tiles the pair space itself.  `cap` = slot capacity per row of the fused pass
        (rows with more matches are recomputed exactly, so it only affects speed).  `store="Name"`
        also assigns the result to `self.graph["Name"]` and keeps the device CSR, so that `degree`,
        `dirichlet`, `local_variance`, `adjacency` on that name run from the CSR on the GPU.
        `distance=local_alignment(...)` or `semiglobal_alignment(...)` is a score, not a distance: `similarity` is not consulted, `k` keeps the largest
        scores, `eps` the pairs with `s > 0 and comp(eps, s)`, and the weights are the scores (`_build_graph_local`).
        `distance=fit_alignment(...)` is such a score too, and DIRECTED: an edge (r, c) carries the score of row r aligned
        WHOLE within any stretch of column c, so row r lists the sequences that contain it best, (r, c) and (c, r) differ,
        and a `k` list may hold negative scores; rank 0 - the row itself or a row of lower index that contains it - is
        dropped as for every distance.
        `distance=spectrum(...)` compares the sequences of the token column by their k-mer counts (`_build_graph_spectrum`):
        profiles from `pg_spectrum_profile`, then the run of a stored embedding under the operator's metric - final fp32
        weights, k up to 1023, `eps` under the five orderings; sequences with equal k-mer multisets are at distance 0 and
        are dropped from `eps` graphs like duplicates.
        A `profile_alignment` instance raises `ValueError`: profiles are queries only (`search`).
        `min_identity=` (0..1) and `min_columns=` cut the graph by PERCENT IDENTITY; `distance` must then be one of the four
        alignment operators (`TypeError`).  The graph is built exactly as without them; then every edge is aligned
        (`align(..., ops=False)`: `pg_alignment_stats` at up to 128 positions) and kept iff its canonical alignment has
        `n_ops >= min_columns` columns and `identities / max(n_ops, 1) >= min_identity` (None: the column cut alone; an
        empty local alignment has identity 0).  Survivors keep their order and their weights; the result is a `CSRGraph`
        (`output="csr"`, also for `k`: a row may keep fewer than k edges) or the filtered tuple list, and `store=` stores
        the filtered graph.
        `candidates=` / `pool=`: FILTER AND REFINE - an alignment graph without the quadratic dynamic programming.
        `distance` must be one of the four alignment operators; `candidates` is any distance `build_graph(k=)` accepts
        (`spectrum(k=3, symbols=20)` is the usual one) with `pool` = candidates per row, an integer in max(k, 1)..1023
        (`ValueError` without it or below k), or a ready graph (`rescore` says which) with `pool` None.  The pool is
        `build_graph(idxs=idxs, k=pool, distance=candidates, representation=representation)`; its entries c == r are
        removed, and `rescore` scores the rest with `distance` and keeps the best `k`, or the `eps` edges, of every row.
        EXACT WITHIN THE POOL, APPROXIMATE OVERALL: a neighbour outside a row's pool is never found (profiles/aln_list.txt
        has a recall table).  With duplicated sequences it also differs from the exact route in what it leaves out: that
        one drops rank 0, whatever it is; this one drops the row itself.  `similarity=True` raises `ValueError`;
        `min_identity=` / `min_columns=` cut the rescored graph.
        """
        if isinstance(distance, profile_alignment):
            raise ValueError(self._PROFILE_QUERIES_ONLY.format("build_graph"))
        if self._identity_cut_asked("build_graph", distance, min_identity, min_columns):
            g = self.build_graph(idxs=idxs, batch_size=batch_size, eps=eps, k=k, weighted=weighted, similarity=similarity,
                                 representation=representation, distance=distance, comp=comp, output="csr", cap=cap,
                                 candidates=candidates, pool=pool)
            if idxs is not None:                                            # the positions `align` maps edges through
                idxs = np.arange(len(self))[idxs] if isinstance(idxs, slice) else np.asarray(idxs)
                idxs = np.nonzero(idxs)[0] if idxs.dtype == bool else idxs
            g = self._identity_cut(g, distance, min_identity, min_columns, representation, idxs=idxs)
            return self._graph_result(g, idxs, store, _keep, output)
        if candidates is not None or pool is not None:
            return self._build_graph_candidates(idxs, eps, k, similarity, representation, distance, comp, output, store, candidates,
                                                pool)
        if operator.xor(bool(eps), bool(k)) is False:
            raise ValueError("Epsilon or K must be provided, but both cannot be as they are different methods of graph construction.")
        if k is not None and not isinstance(k, int):
            raise TypeError("K must be provided as an integer.")

        if idxs is not None:
            # the reference indexes a tensor with `idxs` (prograph.py:726): integer lists, boolean
            # masks and slices all select rows; normalise to integer positions
            if isinstance(idxs, slice):
                idxs = np.arange(len(self))[idxs]
            else:
                idxs = np.asarray(idxs)
                if idxs.dtype == bool:
                    idxs = np.nonzero(idxs)[0]
        route = self._route(distance, comp, k)
        g = None
        if route is not None and route[0]:
            g = getattr(self, route[0])(idxs, eps, k, similarity, representation, comp, cap=cap, distance=distance)
        native = hamming_route = g is None and distance is hamming and route is not None
        planes = None
        if native:
            try:
                planes = self._byte_planes(representation, idxs)
            except (ValueError, TypeError):
                native = False                      # not byte tokens / L > 128: generic torch path
        if native and k and planes.n > _native.MAX_N_KNN:
            native = False
        if hamming_route and not native:
            g = self._build_graph_long(idxs, eps, k, similarity, representation, comp)
        if not native and g is None:
            return self._build_graph_generic(idxs, batch_size, eps, k, similarity, representation, distance, comp)

        if g is not None:
            pass                                    # Minkowski / cosine / Euclidean embeddings, or sequences beyond one record: built above
        elif eps:
            # similarity: comp(1/(1+eps), 1/(1+d)) & (s < 1) is the mirrored integer test on d
            # (:720-721, :734); both sides are the same correctly rounded float32 quotient when d == eps
            indptr, indices, wts = _native.eps_graph(planes, planes, _CMP_CODE[comp], eps, cap=cap)
            g = CSRGraph(indptr, indices, wts, planes.n, similarity=similarity)
        else:
            idx, dist = _native.knn_graph(planes, planes, k)
            g = KNNGraph(idx, dist, planes.n, similarity=similarity)
        return self._graph_result(g, idxs, store, _keep, output)

    def _graph_result(self, g, idxs, store, _keep, output):
        """What `build_graph` hands back for the device graph `g`: stored under `store` / kept under `_keep` (whole-dataset
        graphs only), as the container or as the tuple list."""
        tuples = None
        if store is not None and idxs is None:
            tuples = g.to_tuples()
            self.graph[store] = tuples
            _keep = store
        if _keep is not None and idxs is None:
            if tuples is None:
                tuples = g.to_tuples()
            self.csr_graphs[_keep] = g
            # the device CSR answers for the column only while the column still holds THESE row objects
            self._csr_rows[_keep] = self._row_ids(tuples)
        if output == "csr":
            return g
        return tuples if tuples is not None else g.to_tuples()

    _LONG_MAX_L = 2048                               # integers up to here are exact in fp16

    @staticmethod
    def _integer_threshold(cmp, eps, top=4096):
        """comp(d, eps) on integer distances d in 0..2048 as the same comparison with an integer threshold, which is
        exact in fp16 whatever eps is (-1: an `==` that nothing satisfies).  `top`: the clamp, beyond every value the
        block can hold (2^31 for the int32 blocks of the alignment kernels beyond 128 positions)."""
        e = float(eps)
        lo, hi = int(np.floor(e)), int(np.ceil(e))
        thr = {_native.CMP_LE: lo, _native.CMP_LT: hi, _native.CMP_GE: hi, _native.CMP_GT: lo}.get(cmp, lo if lo == hi else -1)
        return float(min(max(thr, -1), top))

    def _build_graph_long(self, idxs, eps, k, similarity, representation, comp):
        """
        Graphs of byte-token sequences LONGER than one record of the fused engines (more than 255 positions,
        128 for alphabets above 31 symbols; the reference has no limit: hamming.py:32-34 is a broadcast).
        The frame (`_staged`) on the fp16 blocks of `_hamming_segments`: integers up to 2048 are exact.  Returns a
        KNNGraph / CSRGraph with int16 weights, or None when the representation is not byte tokens or longer than
        2048 positions (the generic batch loop then).
        """
        try:
            mat = self.tokenized if representation == "Tokenized" else np.vstack(self(representation))
            mat = np.asarray(mat)
        except (ValueError, TypeError):
            return None
        if mat.ndim != 2 or not np.issubdtype(mat.dtype, np.integer) or mat.shape[0] == 0 or mat.shape[1] == 0:
            return None
        if mat.shape[1] > self._LONG_MAX_L or mat.min() < 0 or mat.max() > 255:
            return None
        if idxs is not None:
            mat = mat[np.asarray(idxs)]
        T = torch.as_tensor(np.ascontiguousarray(mat.astype(np.uint8)), device=_native.device())
        bits = _native.BITS_5 if int(mat.max()) <= 31 else _native.BITS_8
        # similarity graphs: comp(1/(1+eps), 1/(1+d)) & (s < 1) is the same integer test on d (:720-721, :734)
        return self._staged(T.shape[0], T.shape[0], self._hamming_segments(T, T, bits), "f16", torch.int16, k, eps, comp,
                            similarity, False)

    def _build_graph_minkowski(self, idxs, eps, k, similarity, representation, comp, cap=256, distance=None):
        """
        `build_graph(representation=<embedding>, distance=minkowski)` on the HIP kernels:
        the fp16 staging of the reference (:726), then the fused sweeps that compute the fp16 distances
        (rounding like the reference's fp16 tensor ops) and select from them on the device - the canonical
        (value, column) ranks 1..k (`pg_minkowski_knn`, k > 63 one more sweep per 64 ranks: `pg_minkowski_knn_round`;
        the reference drops sorted rank 0, :761-763) or the
        thresholded CSR (`pg_minkowski_eps_*`; :734-739) - without an (N, N) block in HBM.  Returns a KNNGraph /
        CSRGraph with fp16 weights, or None when the staged embedding is not a non-empty 2-D fp16 device tensor
        (the generic path then reports as the reference would).
        """
        try:
            mat = np.vstack(self(representation))
            X = torch.as_tensor(mat, dtype=torch.float16, device=_native.device())
        except (ValueError, TypeError):
            return None
        if X.dim() != 2 or X.shape[0] == 0 or X.shape[1] == 0 or not X.is_cuda:
            return None
        if idxs is not None:
            X = X[torch.as_tensor(np.asarray(idxs), device=X.device)]
        n = X.shape[0]
        if similarity and eps:
            eps = 1 / (1 + eps)                                          # :720-721
        xp = _native.pack_f16(X)
        if k:
            kk = min(k, n - 1)
            if not kk:
                return self._empty_knn(n, torch.float16, X.device, similarity)
            idx, w = _native.minkowski_knn(xp, xp, kk, first=1, similarity=similarity)
            return KNNGraph(idx, w, n, similarity=similarity)
        indptr, indices, wts = _native.minkowski_eps(xp, xp, _CMP_CODE[comp], eps, similarity=similarity, cap=cap)
        return CSRGraph(indptr, indices, wts, n, similarity=similarity)

    def _build_graph_cosine(self, idxs, eps, k, similarity, representation, comp, cap=256, distance=None):
        """
        `build_graph(representation=<embedding>, distance=cosine)` on the matrix-core kernels: the fp16 staging
        (:726), norms and the non-finite check (`pg_cosine_prep`), then the fused sweeps that compute the fp32
        cosine values and select from them on the device - the (value, column) ranks 1..k (`pg_cosine_knn`, k > 63 in
        rounds: `pg_cosine_knn_round`; rank
        0 dropped as in :761-763) or the thresholded CSR (`pg_cosine_eps_*`; :734-739).  Returns a KNNGraph /
        CSRGraph with final fp32 weights, or None (the generic path then) when the staged embedding is not a
        non-empty 2-D fp16 device tensor or holds an inf or nan.
        """
        return self._build_graph_embed_f32("cosine", idxs, eps, k, similarity, representation, comp, cap)

    def _build_graph_euclidean(self, idxs, eps, k, similarity, representation, comp, cap=256, distance=None):
        """
        `build_graph(representation=<embedding>, distance=euclidean)`: `_build_graph_cosine` with the Euclidean
        epilogue (`pg_euclidean_knn`, `pg_euclidean_knn_round`, `pg_euclidean_eps_*`) - the same
        staging, norms and non-finite check, final fp32 weights, and None under the same conditions.
        """
        return self._build_graph_embed_f32("euclidean", idxs, eps, k, similarity, representation, comp, cap)

    def _build_graph_embed_f32(self, metric, idxs, eps, k, similarity, representation, comp, cap):
        """The body `_build_graph_cosine` and `_build_graph_euclidean` share; `metric` names the `_native` wrappers."""
        try:
            mat = np.vstack(self(representation))
            X = torch.as_tensor(mat, dtype=torch.float16, device=_native.device())
        except (ValueError, TypeError):
            return None
        if X.dim() != 2 or X.shape[0] == 0 or X.shape[1] == 0 or not X.is_cuda:
            return None
        if idxs is not None:
            X = X[torch.as_tensor(np.asarray(idxs), device=X.device)]
        return self._build_graph_staged_f32(metric, X, eps, k, similarity, comp, cap)

    def _build_graph_staged_f32(self, metric, X, eps, k, similarity, comp, cap):
        """`_build_graph_embed_f32` from the staged vectors on: X a non-empty (n, D) fp16 device tensor."""
        n = X.shape[0]
        xc = _native.cosine_prep(X)
        if xc.nonfinite():
            return None
        if similarity and eps:
            eps = 1 / (1 + eps)                                          # :720-721
        if k:
            kk = min(k, n - 1)
            if not kk:
                return self._empty_knn(n, torch.float32, X.device, similarity, final=True)
            idx, w = getattr(_native, metric + "_knn")(xc, xc, kk, first=1, similarity=similarity)
            return KNNGraph(idx, w, n, similarity=similarity, final=True)
        indptr, indices, wts = getattr(_native, metric + "_eps")(xc, xc, _CMP_CODE[comp], eps, similarity=similarity, cap=cap)
        return CSRGraph(indptr, indices, wts, n, similarity=similarity, final=True)

    def _spectrum_tokens(self, representation):
        """The token column as `pg_spectrum_profile` takes it - a non-empty (N, L <= 2048) uint8 device tensor: the
        constructor's device copy of the token matrix when there is one, else the column staged now.  None when the
        column is not a matrix of integers in 0..255 of that width."""
        tok = getattr(self, "_tok_u8_dev", None)
        if representation == "Tokenized" and tok is not None:
            return tok
        try:
            mat = np.asarray(self._dataset_matrix(representation))
        except (ValueError, TypeError):
            return None
        if (mat.ndim != 2 or mat.shape[0] == 0 or not 1 <= mat.shape[1] <= _native.SPECTRUM_MAX_L
                or not np.issubdtype(mat.dtype, np.integer) or mat.min() < 0 or mat.max() > 255):
            return None
        return torch.from_numpy(np.ascontiguousarray(mat.astype(np.uint8))).to(_native.device())

    def _build_graph_spectrum(self, idxs, eps, k, similarity, representation, comp, cap, distance):
        """
        `build_graph(distance=spectrum(...))`: the token column staged as uint8 on the device, its k-mer
        count profiles from `pg_spectrum_profile` (`idxs` as the kernel's gather list), the flag word read once, and from
        the fp16 profiles on exactly the run of `_build_graph_embed_f32` for a stored embedding under the operator's
        metric - a KNNGraph / CSRGraph with final fp32 weights.  None (the generic path, where the operator raises for bad
        tokens) when the column is not byte tokens of at most 2048 positions or holds a token above `symbols`.
        """
        tok = self._spectrum_tokens(representation)
        if tok is None or (idxs is not None and len(idxs) == 0):
            return None
        rows = None if idxs is None else np.asarray(idxs, dtype=np.int64)
        if rows is not None:
            rows = np.where(rows < 0, rows + tok.shape[0], rows)           # negative positions count from the end
        prof, flags = _native.spectrum_profile(tok, distance.k, distance.symbols, distance.dims, rows=rows)
        if int(flags.item()):
            return None
        return self._build_graph_staged_f32(distance.metric, prof, eps, k, similarity, comp, cap)

    def _search_spectrum(self, strings, Y, k, eps, comp, similarity, representation, distance):
        """Queries under a `spectrum` distance: dataset and queries through `pg_spectrum_profile`, each at its own width
        (strings are tokenised with the dataset's letter table; the two widths need not agree, and no padding is needed:
        a window holding a 0 does not count), the two flag words read once, then the cosine / Euclidean query paths from
        the staged profiles on, rank 0 and d = 0 kept.  None (the generic loop with the operator, which raises for bad
        tokens) when dataset or queries are not byte tokens of at most 2048 positions or hold a token above `symbols`."""
        tok = self._spectrum_tokens(representation)
        if tok is None:
            return None
        T = self._query_tokens(strings, Y)
        if (T.ndim != 2 or T.shape[0] == 0 or not 1 <= T.shape[1] <= _native.SPECTRUM_MAX_L
                or not np.issubdtype(T.dtype, np.integer) or T.min() < 0 or T.max() > 255):
            return None
        px, fx = _native.spectrum_profile(tok, distance.k, distance.symbols, distance.dims)
        py, fy = _native.spectrum_profile(np.ascontiguousarray(T.astype(np.uint8)), distance.k, distance.symbols, distance.dims)
        if int((fx | fy).item()):
            return None
        if k is not None:
            return self._search_embedding_staged(px, py, k, similarity, distance.plain)
        return self._search_eps_embedding_staged(px, py, eps, comp, similarity, distance.plain)

    _LEV_FUSED_MAX = _native.LEV_MAX_BAND            # thresholds the fused epsilon graph (and the banded first kNN pass) cover

    def _build_graph_levenshtein(self, idxs, eps, k, similarity, representation, comp, cap=256, distance=None):
        """
        `build_graph(distance=levenshtein)` on the HIP kernels, for token matrices they take (tokens up to 31, zeros
        only as trailing padding; else None: the generic loop with the operator).  Up to 128 positions the routes below;
        129..2048 positions `_build_graph_levenshtein_long`; beyond 2048 None.
        eps, comp le / lt / eq with an integer threshold of 1..8: the fused graph (`_native.levenshtein_eps`: bag
        filter, every candidate pair's banded distance once, count / scan / fill).  Any other threshold or ordering:
        row blocks of `pg_levenshtein_dense` in fp16 and the thresholded CSR of `pg_f16_eps_*`.
        k: ranks 1..k of the (d, column) order of exact distances.  Up to k = 63 the banded kNN (band 8) runs first: it
        lists every column within the band in canonical order, so a row whose k-th entry is within the band has its
        exact ranks; the other rows (all rows beyond k = 63) are Y rows of the dense kernel + `pg_f16_knn`.
        PG_LEV_ROUTE=dense takes the dense kernel for everything (A/B comparisons; the graphs are identical).
        Returns a CSRGraph / KNNGraph with uint8 weights whichever route ran; similarities as for Hamming: the same
        integer test on d, formed by the container.
        """
        try:
            mat = np.asarray(self._dataset_matrix(representation))
            if idxs is not None:
                mat = mat[np.asarray(idxs)]
            if mat.ndim == 2 and mat.shape[1] > _native.MAX_L:
                return self._build_graph_levenshtein_long(mat, eps, k, similarity, comp)
            op = self._lev_operand(mat)
        except (ValueError, TypeError):
            return None
        if op is None or op.n >= (1 << 27):
            return None
        n, dev = op.n, op.tokens.device
        dense_only = os.environ.get("PG_LEV_ROUTE", "") == "dense"
        if k:
            block_rows = self._block_rows(n, n, 64)
            kk = min(k, n - 1)
            if not kk:
                return self._empty_knn(n, torch.uint8, dev, similarity)
            if kk <= _native.MAX_K and n <= _native.MAX_N_KNN and not dense_only:
                idx, dist = _native.levenshtein_knn(op.tokens, kk, band=self._LEV_FUSED_MAX)
                todo = torch.nonzero(dist[:, kk - 1] > self._LEV_FUSED_MAX).reshape(-1)
                yo = _native.lev_operand(op.tokens[todo]) if 0 < todo.numel() < n else op
            else:
                idx = torch.empty((n, kk), dtype=torch.int32, device=dev)
                dist = torch.empty((n, kk), dtype=torch.uint8, device=dev)
                todo, yo = None, op
            m = yo.n if (todo is None or todo.numel()) else 0
            for r0 in range(0, m, block_rows):
                r1 = min(m, r0 + block_rows)
                bi, bw = _native.f16_knn(_native.levenshtein_dense(op, yo, out_bytes=2, rows=(r0, r1)), kk, first=1, descending=False)
                where = slice(r0, r1) if todo is None else todo[r0:r1]
                idx[where], dist[where] = bi, bw.to(torch.uint8)
            return KNNGraph(idx, dist, n, similarity=similarity)
        cmp = _CMP_CODE[comp]
        thr = int(self._integer_threshold(cmp, eps))
        if self._nothing_within(cmp, thr):
            return self._empty_csr(n, torch.uint8, dev, similarity)
        if cmp in (_native.CMP_LE, _native.CMP_LT, _native.CMP_EQ) and thr <= self._LEV_FUSED_MAX and not dense_only:
            indptr, indices, wts = _native.levenshtein_eps(op, cmp, thr, cap=max(int(cap), 64))
            return CSRGraph(indptr, indices, wts, n, similarity=similarity)
        return self._staged(n, n, lambda r0, r1: _native.levenshtein_dense(op, op, out_bytes=2, rows=(r0, r1)), "f16", torch.uint8,
                            None, eps, comp, similarity, False)

    def _build_graph_levenshtein_long(self, mat, eps, k, similarity, comp):
        """
        `build_graph(distance=levenshtein)` for token matrices of 129..2048 positions (tokens up to 31, zeros only as
        trailing padding; else None: the generic loop with the operator): the frame on blocks of
        `pg_levenshtein_long_dense` in fp16 - a distance is at most 2048, which fp16 holds exactly.  Every pair goes
        through the full recurrence: no bag filter, no banded first pass and no fused epsilon graph beyond 128 positions.
        Returns a KNNGraph / CSRGraph with int16 weights; similarities as for Hamming, formed by the container.
        """
        if not _native.lev_long_ready():
            return None
        op = self._lev_long_operand(mat)
        if op is None:
            return None
        n, dev = op.n, op.tokens.device
        if not k and self._nothing_within(_CMP_CODE[comp], self._integer_threshold(_CMP_CODE[comp], eps)):
            return self._empty_csr(n, torch.int16, dev, similarity)
        return self._staged(n, n, lambda r0, r1: _native.levenshtein_long_dense(op, op, out_bytes=2, rows=(r0, r1)), "f16",
                            torch.int16, k, eps, comp, similarity, False)

    def _build_graph_substitution(self, idxs, eps, k, similarity, representation, comp, distance, cap=None):
        """
        `build_graph(distance=substitution(C))`: the frame on blocks of `pg_substitution_dense` in fp16.  Taken when the
        representation holds integer tokens of the table, at most 2048 positions, and width * max(C) <= 2048, so that
        every distance is an integer fp16 holds exactly; else None (the generic loop with the operator).  Returns a
        KNNGraph / CSRGraph with int16 weights; similarities as for Hamming: the same integer test on d, formed by the
        container.
        """
        try:
            mat = np.asarray(self._dataset_matrix(representation))
            if idxs is not None:
                mat = mat[np.asarray(idxs)]
            T = self._sub_tokens(mat, distance)
        except (ValueError, TypeError):
            return None
        if T is None or not self._sub_native(T.shape[1], distance):
            return None
        op = _native.sub_operand(torch.from_numpy(np.ascontiguousarray(T)), distance.symbols)
        cost = distance.device_cost()
        dense = lambda r0, r1: _native.substitution_dense(op, op, cost, out_bytes=2, rows=(r0, r1))     # noqa: E731
        return self._staged(op.n, op.n, dense, "f16", torch.int16, k, eps, comp, similarity, False)

    def _build_graph_alignment(self, idxs, eps, k, similarity, representation, comp, distance, cap=None):
        """
        `build_graph(distance=alignment(C, gap[, gap_open]))` on the routes of `_aln_staged`, when the representation
        holds integer tokens of the table; else None (the generic loop with the operator).  Returns a KNNGraph /
        CSRGraph with int16 (beyond 128 positions: int32) weights; similarities as for Hamming: the same integer test on
        d, formed by the container.
        """
        if k is not None and k < 1:
            raise ValueError("K must be at least 1.")
        try:
            mat = np.asarray(self._dataset_matrix(representation))
            if idxs is not None:
                mat = mat[np.asarray(idxs)]
            T = self._sub_tokens(mat, distance)
        except (ValueError, TypeError):
            return None
        if T is None:
            return None
        return self._aln_staged(distance, T, None, k, eps, comp, similarity)

    def _build_graph_generic(self, idxs, batch_size, eps, k, similarity, representation, distance, comp):
        """
        The distance-operator protocol for everything outside the byte-token Hamming path:
        any callable `distance(X, Y, similarity=...) -> (M,N)` (README.md:48 of the reference).
        Same batch loop and fp16 staging as the reference (:726-764), on the GPU, with a stable
        sort for the canonical tie order.
        """
        if similarity and eps:
            eps = 1 / (1 + eps)
        dev = _native.device()
        X = torch.as_tensor(np.vstack(self(representation)), dtype=torch.float16, device=dev)
        if idxs is not None:
            X = X[idxs, :]
        if distance is hamming and len(X):
            # our own operator (sequences beyond the fused engine's limits): batching does not change
            # its result, so take row blocks of up to 2^26 distances instead of the reference's 8 rows
            batch_size = max(batch_size, min(4096, (1 << 26) // len(X)))
        weights, edges = [], []
        if eps:
            for batch in self.get_every_n(X, n=batch_size):
                d = distance(X, batch, similarity=similarity)
                loc = torch.where(comp(eps, d) & (d < 1)) if similarity else torch.where(comp(d, eps) & (d > 0))
                weights.append(d[loc].cpu().numpy())
                edges.append([x.cpu().numpy() for x in loc])
            merged = {}
            for i, coo in enumerate(edges):
                merged.update(self.prod_neighbours(i, coo, batch_size, weights=weights[i]))
            empty = (np.array([], dtype=int), np.array([], dtype=int))
            return [merged.get(i, empty) for i in range(len(X))]
        for batch in self.get_every_n(X, n=batch_size):
            s = torch.sort(distance(X, batch, similarity=similarity), dim=1, descending=bool(similarity), stable=True)
            weights.append([x.cpu().numpy() for x in s[0][:, 1:k + 1]])
            edges.append([x.cpu().numpy() for x in s[1][:, 1:k + 1]])
        return list(zip(flatten(edges), flatten(weights)))

    def _restore_graphs(self, sidecar):
        """Graphs saved as flat arrays by `utils.save(..., graphs="csr")`: back onto the device, and their
        columns (the reference's tuple format, views into two host arrays per graph) into the frame."""
        if not os.path.exists(sidecar):
            return
        from .graph import load_graphs, fingerprint
        for name, g in load_graphs(sidecar, tokens_fingerprint=fingerprint(self.tokenized)).items():
            if name in self.graph or g.nrows != len(self.graph):
                continue
            tuples = g.to_tuples()
            self.graph[name] = tuples
            self.csr_graphs[name] = g
            self._csr_rows[name] = self._row_ids(tuples)

    def _device_graph_any(self, graph):
        """The device-resident form (CSRGraph or KNNGraph as built) of a column that still matches it."""
        return self.csr_graphs.get(graph) if self._device_graph(graph) is not None else None

    # ------------------------------------------------------------------ consumers of the graph column
    def _device_graph(self, graph):
        """The device-resident CSR of a graph column built by this object, if it still matches the
        column (a user may have overwritten `self.graph[name]` with something else)."""
        g = self.csr_graphs.get(graph)
        if g is None or graph not in self.graph:
            return None
        g = g.as_csr() if isinstance(g, KNNGraph) else g
        col = self.graph[graph]
        if len(col) != g.nrows or g.nrows != g.ncols:
            return None
        # identity, not shape: a user who overwrote the column (even with a graph of the same structure,
        # e.g. similarity weights instead of distances) stored other row objects
        # (every row up to 262 144 rows - an in-place replacement of ANY row's tuple is seen; 1024 evenly spaced rows beyond,
        #  where walking a million Python objects would cost more than the device analytics save)
        keep, ids = self._csr_rows.get(graph, (None, None))
        if ids is None or len(ids) != len(col):
            return None
        now = self._row_ids(col.values)[1]
        pick = slice(None) if len(ids) <= 262144 else np.linspace(0, len(ids) - 1, 1024).astype(np.int64)
        if not np.array_equal(now[pick], ids[pick]):
            return None
        return g

    @staticmethod
    def _row_ids(rows):
        """(the row objects - kept alive, so their ids stay theirs -, their ids): which tuples a graph column holds.
        Beyond 262 144 rows only 1024 evenly spaced ones are looked at."""
        n = len(rows)
        if n <= 262144:
            return list(rows), np.fromiter(map(id, rows), dtype=np.int64, count=n)
        ids = np.zeros(n, dtype=np.int64)
        pick = np.linspace(0, n - 1, 1024).astype(np.int64)
        held = [rows[i] for i in pick]
        ids[pick] = [id(o) for o in held]
        return held, ids

    def _column_csr(self, graph):
        """(indptr, indices, weights) numpy arrays of a Neighbours-style column."""
        col = self(graph)
        counts = np.fromiter((len(e[0]) for e in col), dtype=np.int64, count=len(col))
        indptr = np.concatenate([[0], np.cumsum(counts)])
        if indptr[-1] == 0:
            return indptr, np.zeros(0, dtype=int), np.zeros(0)
        return indptr, np.concatenate([e[0] for e in col]), np.concatenate([e[1] for e in col])

    def symmetrize(self, graph, mode="union", combine="min", store=None, output="csr"):
        """The undirected graph of a directed one, on the device (`CSRGraph.symmetrize`): mode="union" - (r, c) is an edge
        iff (r, c) or (c, r) was, the undirected kNN graph - or "mutual" - iff both were, the mutual-kNN graph -, the weight
        `combine` ("min" | "max") over both directions.  Graphs of scores (`local_alignment` and the like) want
        combine="max".  `graph`: a `CSRGraph` / `KNNGraph`, or the name of a stored graph; a column without a matching device
        graph is uploaded (integer weights as int32, others as final float32 values).  `store=` and `output=` as in
        `build_graph`: after `symmetrize("E", mode="mutual", store="M")`, `dirichlet("M")` and `degree("M")` run on the
        device graph."""
        if isinstance(graph, (CSRGraph, KNNGraph)):
            g = graph
        else:
            g = self._device_graph_any(graph)
            if g is None:
                indptr, indices, w = self._column_csr(graph)
                dev = _native.device()
                integer = np.issubdtype(np.asarray(w).dtype, np.integer)
                g = CSRGraph(torch.from_numpy(np.ascontiguousarray(indptr, dtype=np.int64)).to(dev),
                             torch.from_numpy(np.ascontiguousarray(indices, dtype=np.int32)).to(dev),
                             torch.from_numpy(np.ascontiguousarray(w, dtype=np.int32 if integer else np.float32)).to(dev),
                             len(self), final=not integer)
        s = g.symmetrize(mode=mode, combine=combine)
        return self._graph_result(s, None, store, None, output)

    def degree(self, graph="Neighbours", boolean_weights=False):
        g = self._device_graph(graph)
        if g is not None:
            return g.degree(boolean_weights)
        indptr, _, w = self._column_csr(graph)
        if boolean_weights:
            return np.diff(indptr).astype(np.float32)
        deg = np.zeros(len(self), dtype=np.float32)
        rows = np.repeat(np.arange(len(self)), np.diff(indptr))
        np.add.at(deg, rows, w.astype(np.float32))
        return deg

    def get_neighbour_coords(self, graph="Neighbours", boolean_weights=False):
        g = self._device_graph(graph)
        if g is not None:
            return g.coords(boolean_weights)
        indptr, J, w = self._column_csr(graph)
        I = np.repeat(np.arange(len(self), dtype=int), np.diff(indptr))
        if boolean_weights:
            return I, J, np.ones(I.shape)
        return I, J, w.astype(np.float32)

    def adjacency(self, graph="Neighbours", boolean_weights=False):
        from scipy import sparse
        I, J, V = self.get_neighbour_coords(graph=graph, boolean_weights=boolean_weights)
        return sparse.coo_matrix((V, (I, J)), shape=(len(self), len(self)))

    def laplacian(self, graph="Neighbours", boolean_weights=False, mode="outdegree"):
        L = (-1) * self.adjacency(graph, boolean_weights)
        if mode == "outdegree":
            D = self.degree(graph, boolean_weights)
        elif mode == "indegree":
            D = (-1) * np.array(L.sum(0)).reshape(-1,)
        else:
            raise ValueError("Not a valid degree mode.")
        L.setdiag(D)
        return L

    def dirichlet(self, graph="Neighbours", boolean_weights=False, scaler=_DEFAULT_SCALER, mode="outdegree"):
        if scaler is _DEFAULT_SCALER:
            from sklearn.preprocessing import MinMaxScaler as scaler
        fitness = self("Fitness").to_numpy().reshape(-1, 1)
        if scaler is not None:
            fitness = scaler().fit_transform(fitness)
        g = self._device_graph(graph) if mode in ("outdegree", "indegree") else None
        if g is not None:
            return np.array([[g.dirichlet(fitness, boolean_weights, mode=mode)]])
        L = self.laplacian(graph=graph, boolean_weights=boolean_weights, mode=mode)
        return fitness.T @ L @ fitness

    def local_variance(self, graph="Neighbours", boolean_weights=False, scaler=_DEFAULT_SCALER):
        if scaler is _DEFAULT_SCALER:
            from sklearn.preprocessing import MinMaxScaler as scaler
        f = scaler().fit_transform(self("Fitness").to_numpy().reshape(-1, 1)).reshape(-1)
        g = self._device_graph(graph)
        if g is not None:
            return g.local_variance(f)
        indptr, J, _ = self._column_csr(graph)
        out = np.full(len(self), np.nan)
        rows = np.repeat(np.arange(len(self)), np.diff(indptr))
        sums = np.zeros(len(self))
        np.add.at(sums, rows, f[rows] - f[J])
        has = np.diff(indptr) > 0
        out[has] = sums[has] / np.diff(indptr)[has]
        return out

    def graph_to_networkx(self, graph="Neighbours", labels=None, update_self=False, iterable="Sequence"):
        import networkx as nx
        names = list(self(iterable))
        label_cols = [self(l) for l in labels] if labels is not None else []
        g = nx.Graph()
        for i, name in enumerate(names):
            g.add_node(name, **{labels[j]: label_cols[j][i] for j in range(len(label_cols))})
        for i, (nbrs, _) in enumerate(self(graph)):
            g.add_edges_from((names[i], names[j]) for j in nbrs)
        if update_self:
            self.networkx_graph = g
            return None
        return g

    # ------------------------------------------------------------------ data access for ML frameworks
    def _resolve_idxs(self, idxs, distance, positions):
        """README.md:36-40 of the reference documents `distance=` / `positions=` on the data
        accessors but never wires them; here they are forwarded to `indexing`."""
        if idxs is None and (distance not in (None, False) or positions is not None):
            idxs = self.indexing(distances=None if distance in (None, False) else distance, positions=positions)
        return idxs

    def _xy(self, representation, labels, idxs):
        reps = self(representation)
        if idxs is not None:
            X = np.vstack(reps[idxs])
            y = np.vstack([self(l)[idxs] for l in labels]).T
        else:
            X = np.vstack(reps)
            y = np.vstack([self(l) for l in labels]).T
        return X, y

    def sklearn_data(self, data=None, idxs=None, representation="Tokenized", labels=["Fitness"],
                     split=[0.8, 0, 0.2], scaler=False, shuffle=True, random_state=0, distance=None, positions=None):
        import sklearn.utils as skutils
        if isinstance(split, int):
            split = [split, 0, 1 - split]
        assert sum(split) <= 1, "The sum of the split terms must be between 0 and 1"
        idxs = self._resolve_idxs(idxs, distance, positions)
        tokenized, labels = self._xy(representation, labels, idxs)
        if shuffle:
            tokenized, labels = skutils.shuffle(tokenized, labels, random_state=random_state)
        if scaler:
            labels = scaler.fit_transform(labels.reshape(-1, 1)).reshape(-1)
        labels = labels.ravel()
        a, b = int(len(tokenized) * split[0]), int(len(tokenized) * sum(split[:2]))
        parts = [tokenized[:a], labels[:a], tokenized[a:b], labels[a:b], tokenized[b:], labels[b:]]
        return tuple(p.astype("float") for p in parts)

    def gen_dataloaders(self, labels, keys, params, split_points):
        a, b = split_points
        out = {}
        for name, part in (("train", keys[:a]), ("val", keys[a:b]), ("test", keys[b:])):
            if len(part):
                out[name] = torch.utils.data.DataLoader(Dataset(part, labels), **params)
        return out

    def pytorch_dataloaders(self, split=[0.8, 0, 0.2], idxs=None, representation="Tokenized", labels=["Fitness"],
                            distance=False, positions=None,
                            params={"batch_size": 500, "shuffle": True, "num_workers": 8},
                            unsupervised=False, real_label=0):
        idxs = self._resolve_idxs(idxs, distance, positions)
        tokenized, labels = self._xy(representation, labels, idxs)
        keys = [torch.Tensor(t.astype("float32")).long() for t in tokenized]
        if unsupervised:
            data_labels = {key: real_label for key in keys}
        else:
            data_labels = {key: lab for key, lab in zip(keys, labels)}
        cuts = [int(len(tokenized) * split[0]), int(len(tokenized) * sum(split[:2]))]
        return self.gen_dataloaders(labels=data_labels, keys=list(data_labels.keys()), params=params, split_points=cuts)

    def fit(self, model, model_args, save_model=False, **kwargs):
        x_train, y_train, _, _, x_test, y_test = self("sklearn", **kwargs)
        model = model(**model_args)
        if model.__class__.__name__ == "NeuralNetRegressor":
            y_train, y_test = y_train.reshape(-1, 1), y_test.reshape(-1, 1)
        print(f"Training model {model}")
        model.fit(x_train, y_train)
        train_score = model.score(x_train, y_train)
        print(f"Model score on training data: {train_score}")
        test_score = model.score(x_test, y_test)
        print(f"Score of {model} on testing data is {test_score}")
        if save_model:
            self.learners[f"{model}"] = model
        return train_score, test_score
