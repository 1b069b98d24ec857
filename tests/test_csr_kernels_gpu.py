"""
The three CSR support kernels alone, on the GPU: `pg_csr_row_stats`, `pg_exclusive_scan`, `pg_compact_flags`.

Every graph of every distance passes through them - `indptr` is the scan of the row counts, the rows beyond the slot
capacity come from the flag compaction, and `degree`, `laplacian`, `dirichlet`, `local_variance` are `pg_csr_row_stats` -
yet they were only ever run inside `Prograph` on two Hamming graphs.  Here each is called on its own:

- `pg_csr_row_stats` against the independent model of tests/csr_model.py (`math.fsum` per row and per column): bit for
  bit where every partial sum is exact in float64 (then the order of the wave's tree reduction and of the atomics
  cannot show), within a derived bound on general floats; with no weights, uint8 and float32 weights, negative
  weights, `row0 != 0`, `nrows != ncols`, row counts that fill and do not fill a workgroup of four rows, row lengths
  around the 64 entries a wave takes a turn, columns named by many lanes and many rows, and entries with a negative
  column, which are no edges;
- the scan against NumPy's int64 cumulative sum at every length at which a lane, a wave, a tile of 2048 or a chunk of
  256 tile totals ends, with counts of 2^32 - 1 at those seams so that the running total passes 2^32 and 2^33;
- the compaction against `np.nonzero` at the same lengths.

Through the raw entries the operands and outputs lie in the middle of one larger allocation filled with a mark, each
between guards: whatever is written outside an output, or into an input, is seen.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import csr_model as M
from prograph_amd import _native

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

MARK = 0xA5
TILE = 2048                                   # elements per workgroup of the scan; pg_scan_single takes 256 tile totals a turn
LENGTHS = (1, 7, 8, 9, 255, 256, 2047, 2048, 2049, 4096, 256 * TILE - 1, 256 * TILE, 256 * TILE + 1, 257 * TILE + 5)


class Arena:
    """Arrays carved out of the middle of one device allocation of MARK bytes: 4096 bytes in front and behind, 256
    between any two.  `check()` reads everything back: the bytes outside the carved arrays still hold the mark, the
    inputs what they held; the outputs are returned."""
    EDGE, GAP = 4096, 256

    def __init__(self):
        self.items, self.size = {}, self.EDGE

    def add(self, name, array, output=False):
        array = np.ascontiguousarray(array)
        self.items[name] = (self.size, array, output)
        self.size += -(-array.nbytes // self.GAP) * self.GAP + self.GAP
        return self

    def marked(self, name, shape, dtype):
        """An output that starts as MARK bytes."""
        return self.add(name, np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, MARK, np.uint8).view(dtype).reshape(shape), True)

    def build(self):
        host = np.full(self.size + self.EDGE, MARK, dtype=np.uint8)
        for at, array, _ in self.items.values():
            host[at:at + array.nbytes] = array.reshape(-1).view(np.uint8)
        self.buf = torch.from_numpy(host).cuda()
        return self

    def ptr(self, name):
        return ctypes.c_void_p(self.buf.data_ptr() + self.items[name][0]) if name in self.items else None

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
        assert not len(bad), ("bytes outside the outputs were written", np.flatnonzero(outside)[bad[:8]], self.items_at())
        return out

    def items_at(self):
        return {name: (at, array.nbytes) for name, (at, array, _) in self.items.items()}


# ---------------------------------------------------------------- pg_csr_row_stats
ROW_CASES = [(n, r0) for n in M.NROWS for r0 in M.ROW0]
ROW_KEYS = M.KEYS[:4]


@functools.lru_cache(maxsize=None)
def _lists(nrows, row0, negative):
    indptr, indices = M.edge_lists(nrows, row0, M.SEED[nrows])
    return indptr, (M.with_negative_columns(indptr, indices) if negative else indices)


def _raw_row_stats(indptr, indices, w, f, row0, ncols=M.NCOLS):
    """All five outputs through the raw entry, everything inside an Arena; returns the outputs after its check."""
    nrows = len(indptr) - 1
    a = Arena().add("indptr", indptr).add("indices", indices if len(indices) else np.zeros(1, np.int32))
    if w is not None:
        a.add("w", w)
    a.add("f", f)
    for key in ROW_KEYS:
        a.marked(key, (nrows,), np.float64)
    a.add("col_sum", np.zeros(ncols, np.float64), output=True).build()
    w8, wf = (a.ptr("w"), None) if w is not None and w.dtype == np.uint8 else (None, a.ptr("w"))
    rc = _native.lib().pg_csr_row_stats(a.ptr("indptr"), a.ptr("indices"), w8, wf, nrows, row0, a.ptr("f"), a.ptr("deg"),
                                        a.ptr("sum_f"), a.ptr("sum_wf"), a.ptr("self_w"), a.ptr("col_sum"), _native._stream())
    assert rc == 0, _native.lib().pg_last_error()
    return a.check()


def _wrapped_row_stats(indptr, indices, w, f, row0, want, ncols=M.NCOLS):
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    got = _native.csr_row_stats(t(indptr), t(indices), t(w), f=t(f), want=want, row0=row0, ncols=ncols)
    assert set(got) == set(want)
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("negative", [False, True], ids=["edges", "negative_columns"])
@pytest.mark.parametrize("weights", ["none", "u8", "f32"])
@pytest.mark.parametrize("nrows, row0", ROW_CASES)
def test_row_stats_equal_the_model_bit_for_bit_where_sums_are_exact(nrows, row0, weights, negative):
    """Weights that are integers or multiples of 2^-10 below 8 in magnitude, f multiples of 2^-20 in [0, 1), at most 600
    entries a row and a few thousand a column: every product and partial sum is a multiple of 2^-30 below 2^18, exact in
    float64.  So the five outputs equal the model whatever the order of the tree reduction and of the atomics - all
    five together through the raw entry (guards checked), and each one asked for alone."""
    indptr, indices = _lists(nrows, row0, negative)
    w, f = M.exact_weights(weights, len(indices)), M.exact_values(M.NCOLS)
    want = M.row_stats(indptr, indices, w, f, row0, M.NCOLS)
    assert want["abs_deg"].max() < 2 ** 18 and want["abs_col_sum"].max() < 2 ** 18
    if nrows == 19:
        assert want["n_cols"][M.HOT] > 300 and (want["self_w"] != 0).sum() >= 4   # the lists are what they claim
        if negative:
            assert (indices < 0).sum() > 600 and want["n_rows"].min() == 0
    got = _raw_row_stats(indptr, indices, w, f, row0)
    for key in M.KEYS:
        assert np.array_equal(got[key], want[key]), (key, np.flatnonzero(got[key] != want[key])[:8])
    for key in M.KEYS:
        alone = _wrapped_row_stats(indptr, indices, w, f, row0, (key,))
        assert np.array_equal(alone[key], want[key]), key
    both = _wrapped_row_stats(indptr, indices, w, f, row0, M.KEYS)
    assert all(np.array_equal(both[key], want[key]) for key in M.KEYS)


@pytest.mark.parametrize("negative", [False, True], ids=["edges", "negative_columns"])
@pytest.mark.parametrize("nrows, row0", ROW_CASES)
def test_row_stats_on_general_floats_stay_within_the_bound_of_a_reordered_sum(nrows, row0, negative):
    """Random float32 weights and float64 f.  A sum of n float64 terms in any order is within (n - 1) 2^-53 sum|terms| of
    the exact sum to first order, a product adds one rounding of 2^-53 |term|, and the model's own sum is correctly
    rounded: n 2^-52 sum|terms| per row or column covers the three with a factor of two to spare."""
    indptr, indices = _lists(nrows, row0, negative)
    rng = np.random.default_rng(nrows * 100 + row0)
    w = (rng.standard_normal(len(indices)) * 10.0 ** rng.integers(-3, 4, len(indices))).astype(np.float32)
    f = rng.standard_normal(M.NCOLS) * 10.0 ** rng.integers(-3, 4, M.NCOLS)
    want = M.row_stats(indptr, indices, w, f, row0, M.NCOLS)
    got = _raw_row_stats(indptr, indices, w, f, row0)
    for key in M.KEYS:
        n = want["n_cols"] if key == "col_sum" else want["n_rows"]
        bound = n * 2.0 ** -52 * want["abs_" + key]
        err = np.abs(got[key] - want[key])
        assert np.all(err <= bound), (key, np.flatnonzero(err > bound)[:8], err.max())
    assert np.array_equal(got["deg"][want["n_rows"] == 0], np.zeros(int((want["n_rows"] == 0).sum())))


def test_row_stats_of_a_table_of_empty_slots_only():
    """Every entry a negative column (a kNN table none of whose rows found a candidate): zeros everywhere, nothing
    written in front of f or col_sum."""
    indptr = np.arange(0, 5 * 70 + 1, 70, dtype=np.int64)
    indices = np.full(350, -1, dtype=np.int32)
    got = _raw_row_stats(indptr, indices, np.full(350, 3, np.uint8), M.exact_values(M.NCOLS), 0)
    for key in M.KEYS:
        assert not got[key].any(), key


def test_row_stats_argument_errors_return_before_any_launch():
    lib = _native.lib()
    p = ctypes.c_void_p(256)                                              # never dereferenced
    call = lambda indptr=p, indices=p, nrows=4, row0=0, f=p, sum_f=None, sum_wf=None: lib.pg_csr_row_stats(
        indptr, indices, None, None, nrows, row0, f, p, sum_f, sum_wf, None, None, _native._stream())
    for bad in (dict(indptr=None), dict(indices=None), dict(nrows=0), dict(row0=-1), dict(f=None, sum_f=p), dict(f=None, sum_wf=p)):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------- pg_exclusive_scan
SEAMS = (0, 7, 8, 63, 64, 511, 512, 2047, 2048, 2049, 4095, 4096, 256 * TILE - 1, 256 * TILE, 256 * TILE + 1)


def _counts(n, pattern):
    """uint32 counts: zeros | values 0..5 | 2^32 - 1 at the last element of a lane (8 elements), a wave (512), a tile
    (2048) and a chunk of tile totals (256 tiles) and at the first of the next, at the last element, small values between."""
    rng = np.random.default_rng(n)
    if pattern == "zeros":
        return np.zeros(n, dtype=np.uint32)
    c = rng.integers(0, 6, n).astype(np.uint32)
    if pattern == "seams":
        at = np.array([s for s in SEAMS + (n - 1,) if s < n])
        c[at] = 0xFFFFFFFF
    return c


@pytest.mark.parametrize("n", LENGTHS)
def test_exclusive_scan_equals_the_int64_cumulative_sum(n):
    lib = _native.lib()
    nbytes = int(lib.pg_scan_scratch_bytes(n))
    assert nbytes == 8 * (-(-n // TILE) + 2)
    for pattern in ("zeros", "small", "seams"):
        counts = _counts(n, pattern)
        want = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        if pattern == "seams" and n >= 9:
            assert want[-1] > 2 ** 33 and want[9] > 2 ** 32                 # the total passes 2^32 inside the first wave
        a = Arena().add("counts", counts).marked("indptr", (n + 1,), np.int64).marked("scratch", (nbytes,), np.uint8).build()
        assert lib.pg_exclusive_scan(a.ptr("counts"), n, a.ptr("indptr"), a.ptr("scratch"), _native._stream()) == 0
        got = a.check()["indptr"]
        assert got.dtype == np.int64 and np.array_equal(got, want), (pattern, np.flatnonzero(got != want)[:8])


# ---------------------------------------------------------------- pg_compact_flags
def _flags(n, pattern):
    """uint8 flags from {0, 1, 2, 128, 255}: any non-zero byte is a set flag and counts once."""
    rng = np.random.default_rng(n + 1)
    set_ = rng.choice(np.array([1, 2, 128, 255], dtype=np.uint8), n)
    keep = np.zeros(n, dtype=bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "first":
        keep[0] = True
    elif pattern == "last":
        keep[n - 1] = True
    elif pattern == "tile_seam":
        keep[[i for i in (TILE - 1, TILE) if i < n]] = True
    elif pattern == "random":
        keep = rng.random(n) < 0.3
    return np.where(keep, set_, 0).astype(np.uint8)


@pytest.mark.parametrize("n", LENGTHS)
def test_compact_flags_equal_nonzero(n):
    lib = _native.lib()
    nbytes = int(lib.pg_scan_scratch_bytes(n))
    for pattern in ("none", "all", "first", "last", "tile_seam", "random"):
        flags = _flags(n, pattern)
        want = np.nonzero(flags)[0].astype(np.int64)
        assert pattern != "none" or len(want) == 0
        dev = torch.from_numpy(flags).cuda()
        got = _native.compact_flags(dev)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), pattern
        assert np.array_equal(_native.compact_flags(dev, count=len(want)).cpu().numpy(), want), pattern
        a = (Arena().add("flags", flags).marked("out", (n,), np.int64).marked("count", (1,), np.int64)
             .marked("scratch", (nbytes,), np.uint8).build())
        assert lib.pg_compact_flags(a.ptr("flags"), n, a.ptr("out"), a.ptr("count"), a.ptr("scratch"), _native._stream()) == 0
        out = a.check()
        assert int(out["count"][0]) == len(want), pattern
        assert np.array_equal(out["out"][:len(want)], want), pattern
        assert (out["out"][len(want):].view(np.uint8) == MARK).all(), pattern     # beyond the count nothing is written
