"""
Host logic of `Prograph.search(queries, eps=...)` (radius search of queries that need not be in the dataset) and of
`neighbourhood` for a string outside the dataset, with the CPU stand-in of tests/fake_native.py plus fakes of the query
entries defined here; and the argument checks of the new C entries (refused on the host before any launch: no GPU).
"""
import ctypes
import operator

import numpy as np
import pandas as pd
import pytest
import torch

import fake_native
from prograph_amd import _native, synth

OPS = {_native.CMP_LE: operator.le, _native.CMP_LT: operator.lt, _native.CMP_EQ: operator.eq,
       _native.CMP_GE: operator.ge, _native.CMP_GT: operator.gt}
COMPS = (operator.le, operator.lt, operator.eq, operator.ge, operator.gt)


def _csr(keep, w, wdtype):
    indptr = np.zeros(keep.shape[0] + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(keep.sum(1))
    r, c = np.nonzero(keep)
    return torch.from_numpy(indptr), torch.from_numpy(c.astype(np.int32)), torch.from_numpy(w[r, c]).to(wdtype)


def _fake_query_eps(qp, dp, cmp, eps, pieces=None):
    l = max(qp.l, dp.l)
    d = (fake_native._pad_to(qp.tok, l)[:, None, :] != fake_native._pad_to(dp.tok, l)[None, :, :]).sum(2)
    return _csr(OPS[cmp](d, eps), d, torch.uint8)


def _fake_f16_eps(block, cmp, eps, similarity=False, keep_zero=False):
    d = block.to(torch.float32).numpy()
    e = float(np.float16(eps))
    keep = OPS[cmp](e, d) if similarity else OPS[cmp](d, e)
    if not keep_zero:
        keep &= (d < 1) if similarity else (d > 0)
    return _csr(keep, d, torch.float16)


def _fake_pack_bytes(raw, lut, bits=_native.BITS_5, want_tokens=True, check=True):
    tok = np.asarray(lut)[np.asarray(raw)]
    return fake_native.FakePlanes(tok, bits), (torch.from_numpy(tok.astype(np.uint8)) if want_tokens else None)


@pytest.fixture
def fake(monkeypatch):
    fake_native.install(monkeypatch)
    calls = []
    monkeypatch.setattr(_native, "query_eps", lambda qp, dp, cmp, eps: (calls.append(("query_eps", qp.l, dp.l)),
                                                                         _fake_query_eps(qp, dp, cmp, eps))[1])
    monkeypatch.setattr(_native, "f16_eps", lambda *a, **kw: (calls.append(("f16_eps", kw.get("keep_zero", False))),
                                                               _fake_f16_eps(*a, **kw))[1])
    monkeypatch.setattr(_native, "pack_bytes", lambda *a, **kw: (calls.append(("pack_bytes",)), _fake_pack_bytes(*a, **kw))[1])
    return calls


def _prograph(tmp_path, tok, name="s"):
    from prograph_amd import Prograph
    f = tmp_path / f"{name}.csv"
    pd.DataFrame({"Sequence": synth.tokens_to_strings(tok),
                  "Fitness": np.random.default_rng(0).uniform(0, 1, len(tok))}).to_csv(f)
    return Prograph(file=str(f))


def _want(X, Y, eps, comp=operator.le, sim=False):
    """per query np.nonzero(comp(d, eps)) on the padded tokens, and the weights build_graph(eps=) would give."""
    l = max(X.shape[1], Y.shape[1])
    Xp, Yp = fake_native._pad_to(X, l), fake_native._pad_to(Y, l)
    d = (Yp[:, None, :] != Xp[None, :, :]).sum(2)
    out = []
    for row in d:
        j = np.nonzero(comp(row, eps))[0]
        out.append((j, (1 / (1 + row[j])).astype(np.float32) if sim else row[j].astype(np.int64)))
    return out


def _same(got, want):
    assert len(got) == len(want)
    for (gi, gw), (wi, ww) in zip(got, want):
        assert gi.dtype == np.int64 and np.array_equal(gi, wi)
        if len(wi):
            assert gw.dtype == ww.dtype and np.array_equal(gw, ww)
        else:
            assert len(gw) == 0


@pytest.fixture
def pg(fake, tmp_path, capsys):
    tok = synth.clustered_tokens(120, 12, seed=4, members=20)
    tok[77] = tok[5]                                        # a duplicated row
    tok[100] = tok[5]
    p = _prograph(tmp_path, tok)
    capsys.readouterr()
    return p


def _queries(pg):
    rng = np.random.default_rng(1)
    s9 = pg("Sequence")[9]
    mutated = ("W" if s9[0] != "W" else "Y") + s9[1:]
    return [pg("Sequence")[5], s9, mutated, "ACDXXQ", "".join(rng.choice(list("ACDEFGHIKL"), 12))]


def test_strings_tokens_and_shapes(pg, fake):
    X = pg.tokenized
    seqs = _queries(pg)
    T = pg.tokenize(seqs)
    for eps in (0, 1, 2, 4, 12, 1.5):
        want = _want(X, T, eps)
        _same(pg.search(seqs, eps=eps), want)
        _same(pg.search(T, eps=eps), want)
        _same(pg.search(torch.from_numpy(T), eps=eps), want)
    assert ("pack_bytes",) in fake and any(c[0] == "query_eps" for c in fake)
    _same(pg.search(seqs[0], eps=2), _want(X, T[:1], 2))                # one string = a list of one
    _same(pg.search(T[1], eps=2), _want(X, T[1:2], 2))                  # 1-D tokens = one query
    _same(pg.search(seqs, eps=3, similarity=True), _want(X, T, 3, sim=True))
    assert pg.search(seqs, eps=3, similarity=True)[0][1].dtype == np.float32


def test_eps_zero_finds_the_duplicates(pg):
    got = pg.search(_queries(pg), eps=0)
    assert list(got[0][0]) == [5, 77, 100] and list(got[0][1]) == [0, 0, 0]      # d = 0 is kept, ascending rows
    assert list(got[1][0]) == [9]
    for i in (2, 3):
        assert len(got[i][0]) == 0 and len(got[i][1]) == 0
    assert got[2][0] is got[3][0]                                       # rows without a hit share the empty pair


def test_comparators_and_float_eps(pg):
    X = pg.tokenized
    T = pg.tokenize(_queries(pg))
    for comp in COMPS:
        for eps in (0, 2, 2.5, 11, 12, 13, -1):
            _same(pg.search(T, eps=eps, comp=comp), _want(X, T, eps, comp))
        _same(pg.search(T, eps=2, comp=comp, similarity=True), _want(X, T, 2, comp, sim=True))


def test_shorter_and_longer_queries(pg, fake):
    X = pg.tokenized
    short = ["ACD", "K"]
    long_ = [pg("Sequence")[3] + "ACDEF", "A" * 30, pg("Sequence")[3]]
    for q in (short, long_):
        T = pg.tokenize(q)
        for eps in (3, 9, 20):
            _same(pg.search(q, eps=eps), _want(X, T, eps))
            _same(pg.search(T, eps=eps), _want(X, T, eps))
    # a longer query packs the dataset at the query's width for that call: its extra positions count against zeros
    assert any(c[0] == "query_eps" and c[1] == c[2] == 30 for c in fake)
    assert list(pg.search(long_[0], eps=5)[0][0]) == list(_want(X, pg.tokenize(long_[:1]), 5)[0][0])


def test_k_and_eps_are_exclusive_and_k_errors_unchanged(pg):
    both = "Epsilon or K must be provided, but both cannot be as they are different methods of graph construction."
    with pytest.raises(ValueError, match="Epsilon or K"):
        pg.search("ACD", 3, eps=2)
    with pytest.raises(ValueError, match="Epsilon or K"):
        pg.search("ACD", k=3, eps=0)
    with pytest.raises(ValueError, match="Epsilon or K"):
        pg.search("ACD")
    with pytest.raises(ValueError) as e:
        pg.search("ACD", 0)
    assert str(e.value) == both
    with pytest.raises(TypeError) as e:
        pg.search("ACD", 2.0)
    assert str(e.value) == "K must be provided as an integer."
    with pytest.raises(ValueError) as e:
        pg.search("ACD", -2)
    assert str(e.value) == "K must be at least 1."
    with pytest.raises(TypeError):
        pg.search("ACD", eps="2")
    with pytest.raises(ValueError):
        pg.search("ACD", eps=float("nan"))
    for empty in ([], np.zeros((0, 12), dtype=np.int64)):
        with pytest.raises(ValueError):
            pg.search(empty, eps=2)


def test_csr_output(pg):
    from prograph_amd.graph import CSRGraph
    T = pg.tokenize(_queries(pg))
    for eps, sim in ((2, False), (12, False), (3, True)):
        G = pg.search(T, eps=eps, output="csr", similarity=sim)
        assert isinstance(G, CSRGraph) and G.nrows == len(T) and G.ncols == len(pg)
        assert G.indptr.dtype == torch.int64 and G.indices.dtype == torch.int32 and G.weights.dtype == torch.uint8
        tup = pg.search(T, eps=eps, similarity=sim)
        for (gi, gw), (ti, tw) in zip(G.to_tuples(), tup):
            assert np.array_equal(gi, ti) and np.array_equal(gw, tw) and gw.dtype == tw.dtype


def test_long_sequences_take_the_staged_path(fake, tmp_path, capsys):
    tok = synth.clustered_tokens(60, 300, seed=8, members=12)
    tok[41] = tok[2]
    p = _prograph(tmp_path, tok, "long")
    del fake[:]                                             # (the constructor's eps = 1 graph excludes d = 0)
    T = tok[[2, 7]].copy()
    T[1, :3] = (T[1, :3] % 20) + 1
    for comp in COMPS:
        for eps in (0, 3, 2.5):
            got = p.search(T, eps=eps, comp=comp)
            _same(got, _want(tok, T, eps, comp))
    assert ("f16_eps", True) in fake and ("f16_eps", False) not in fake
    G = p.search(T, eps=3, output="csr")
    assert G.weights.dtype == torch.int16 and {2, 41} <= set(G.to_tuples()[0][0])


def test_generic_loop(pg):
    X = pg.tokenized.astype(np.float32)
    T = pg.tokenize(["ACDEFGHIKL", "MNPQ", pg("Sequence")[11]])

    def l1(A, B, similarity=False):
        A, B = A.to(torch.float32), B.to(torch.float32)
        B = torch.nn.functional.pad(B, (0, A.shape[1] - B.shape[1]))
        d = (B[:, None, :] - A[None, :, :]).abs().sum(2)
        return 1 / (1 + d) if similarity else d

    Tp = fake_native._pad_to(T, X.shape[1]).astype(np.float32)
    d = np.abs(Tp[:, None, :] - X[None]).sum(2)
    for eps in (0, 30, 60.5):
        got = pg.search(T, eps=eps, distance=l1)
        for (gi, gw), row in zip(got, d):
            j = np.nonzero(row <= eps)[0]
            assert np.array_equal(gi, j) and np.array_equal(gw, row[j])
        s = (1 / (1 + d)).astype(np.float32)
        got = pg.search(T, eps=eps, distance=l1, similarity=True)
        for (gi, gw), row in zip(got, s):
            j = np.nonzero(1 / (1 + eps) <= row)[0]
            assert np.array_equal(gi, j) and np.array_equal(gw, row[j])
    assert list(pg.search(T, eps=0, distance=l1)[2][0]) == [11]          # d = 0 is not excluded
    G = pg.search(T, eps=30, distance=l1, output="csr")
    assert G.nrows == 3 and G.ncols == len(pg) and G.final

    # a comparator outside the five orderings: the generic loop with the project's own Hamming operator
    from prograph_amd.distance import hamming

    def band(a, b):
        return (a >= b - 1) & (a <= b + 1) if isinstance(a, torch.Tensor) else NotImplemented

    Q = pg.tokenize([pg("Sequence")[5], pg("Sequence")[30]])
    got = pg.search(Q, eps=1, comp=band, distance=hamming)
    dd = (Q[:, None, :] != pg.tokenized[None]).sum(2)
    for (gi, gw), row in zip(got, dd):
        j = np.nonzero((row >= 0) & (row <= 2))[0]
        assert np.array_equal(gi, j) and np.array_equal(np.asarray(gw).astype(np.int64), row[j])
    assert 5 in got[0][0] and 77 in got[0][0]


def test_neighbourhood_of_a_string_outside_the_dataset(pg):
    seqs = pg("Sequence")
    s9 = seqs[9]
    mutated = ("W" if s9[0] != "W" else "Y") + s9[1:]
    assert mutated not in pg.seq_idxs
    d = (pg.tokenize([mutated]) != pg.tokenized).sum(1)
    for eps in (0, 1, 3):
        rows = pg.neighbourhood(mutated, eps)
        assert list(rows.index) == list(pg.graph.index[d <= eps])
    assert 9 in set(np.nonzero(d <= 1)[0])
    assert len(pg.neighbourhood("ACD", 0)) == 0
    # a member of the dataset: the path and the result of before
    d5 = (pg.tokenized[5] != pg.tokenized).sum(1)
    for eps in (0, 2):
        rows = pg.neighbourhood(seqs[5], eps)
        assert list(rows.index) == list(pg.graph.index[d5 <= eps])
        assert list(pg.neighbourhood(5, eps).index) == list(rows.index)


def test_keep_zero_reaches_the_binding():
    assert _native.CMP_KEEP_ZERO == 0x10 and all(c & _native.CMP_KEEP_ZERO == 0 for c in OPS)
    import inspect
    for fn in (_native.f16_eps, _native.minkowski_eps, _native.cosine_eps):
        assert inspect.signature(fn).parameters["keep_zero"].default is False


# ---- the C entries: declared, bound, exported, and refused on the host before any launch
def test_query_eps_entries_validate_arguments():
    L = _native.lib()
    for name in ("pg_query_eps_segments", "pg_query_eps_count", "pg_query_eps_fill"):
        assert name in _native.SYMBOLS and hasattr(L, name)
    p = ctypes.c_void_p(256)          # never dereferenced: every call below is refused on the host
    BAD, LONG, MANY = -1, -2, -3

    def count(qp=p, nq=10, qnpad=256, dbp=p, ndb=300, dbnpad=512, l=64, bits=5, cmp=0, eps=2.0, nseg=4, out=p):
        return L.pg_query_eps_count(qp, nq, qnpad, dbp, ndb, dbnpad, l, bits, cmp, eps, nseg, out, None)

    def fill(qp=p, nq=10, qnpad=256, dbp=p, ndb=300, dbnpad=512, l=64, bits=5, cmp=0, eps=2.0, nseg=4, ptr=p, idx=p, w=p):
        return L.pg_query_eps_fill(qp, nq, qnpad, dbp, ndb, dbnpad, l, bits, cmp, eps, nseg, ptr, idx, w, None)

    assert count(qp=None) == BAD and b"pg_query_eps_count" in L.pg_last_error()
    assert fill(qp=None) == BAD and b"pg_query_eps_fill" in L.pg_last_error()
    assert count(dbp=None) == BAD and count(out=None) == BAD
    assert fill(dbp=None) == BAD and fill(ptr=None) == BAD and fill(idx=None) == BAD and fill(w=None) == BAD
    for call in (count, fill):
        assert call(cmp=5) == BAD and call(cmp=-1) == BAD
        assert call(cmp=_native.CMP_KEEP_ZERO) == BAD                   # d = 0 is always kept here: no flag to give
        assert call(eps=float("nan")) == BAD
        assert call(bits=6) == BAD and call(bits=0) == BAD
        assert call(nq=0) == BAD and call(ndb=0) == BAD and call(nq=-4) == BAD
        assert call(dbnpad=300) == BAD and call(qnpad=5) == BAD and call(dbnpad=256) == BAD
        assert call(nseg=0) == BAD and call(nseg=6) == BAD and call(nseg=-4) == BAD
        assert call(nseg=16) == BAD                                     # 300 columns: three tiles, at most three pieces
        assert call(l=300) == LONG and call(l=160, bits=8) == LONG
        assert call(ndb=1 << 31, dbnpad=1 << 31, nseg=4) == MANY
    # the plan: a function of (nq, ndb) only, 4 segments (waves) per piece, at least one tile of 128 columns per wave
    assert L.pg_query_eps_segments(0, 300) == 0 and L.pg_query_eps_segments(5, 0) == 0
    assert L.pg_query_eps_segments(1, 100) == 4 and L.pg_query_eps_segments(1, 1) == 4
    assert L.pg_query_eps_segments(1, 200000) == 4 * 391                  # 1563 tiles: one per wave
    assert L.pg_query_eps_segments(10000, 200000) == 8                    # 1250 query groups: two pieces reach 2048
    assert L.pg_query_eps_segments(100000, 200000) == 4
    # the existing eps entries: a code outside the five is refused with or without the flag
    assert L.pg_f16_eps_count(p, 4, 4, 4, 5, 1.0, 0, p, None) == BAD and L.pg_f16_eps_count(p, 4, 4, 4, 0x15, 1.0, 0, p, None) == BAD
    assert L.pg_minkowski_eps_slots(p, 300, 512, p, 10, 256, 64, 0, 0x25, 1.0, 8, p, p, p, None) == BAD
    assert L.pg_eps_slots(p, 256, 0, 10, p, 512, 300, 64, 5, 0x10, 2.0, 8, p, p, p, p, None) == BAD   # Hamming graphs: no flag
