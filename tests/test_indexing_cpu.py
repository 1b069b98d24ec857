"""
The index pins that need no GPU (tests/indexing_testdata.py holds the data and the reference):

  * `flags_of`, the numpy reference that tests/test_indexing_gpu.py compares the kernel with, IS the reference
    project's indexing (oracle.prograph_oracle.indexing, pinned to prograph/prograph.py:298-325 by golden vectors):
    every position query under both `Bool` values on the mutant libraries, the distance sets on the ladders;
  * the queries are not trivially empty or full - the share is asserted per shape and printed;
  * the host logic of `Prograph.indexing` / `positions` / `distances` / `calc_neighbours` / `neighbourhood` around the
    kernel, with tests/fake_native.py in its place;
  * `_native.position_bitmask`, the word and bit of every position.
"""
import numpy as np
import pandas as pd
import pytest

import indexing_testdata as D
from oracle import prograph_oracle as O

N = 600
# (L, A, ref_len): every width of the kernel pins, and its short reference from 33 positions on
LIBRARIES = [(L, D.letters_of(bits), None) for L, bits in D.SHAPES] + \
            [(L, D.letters_of(bits), D.short_ref(L)) for L, bits in D.SHAPES if D.short_ref(L)]


def _lib_id(v):
    return f"L{v[0]}_A{v[1]}" + (f"_ref{v[2]}" if v[2] else "")


def _oracle_hits(T, ref_len, **kw):
    try:
        return O.indexing(T, 0, ref_len, **kw)
    except AssertionError:                                   # the reference asserts a non-empty answer (:338)
        return np.zeros(0, dtype=np.int64)


@pytest.mark.parametrize("shape", LIBRARIES, ids=_lib_id)
def test_reference_is_the_oracle_on_positions(shape):
    """flags_of == oracle.indexing for every query of position_queries and both Bool values, and at least three
    quarters of the counted queries (every single position and the first 40 pairs) hit some rows but not all."""
    L, A, short = shape
    ref_len = L if short is None else short
    T = D.library(N, L, A, seed=1000 + L, ref_len=short)
    assert T.shape == (N, L) and T.min() == 0 and T.max() <= A
    qs, counted = D.position_queries(D.edges(ref_len), ref_len, L)
    solid = total = 0
    for i, q in enumerate(qs):
        for mode, Bool in ((1, "or"), (2, "and")):
            want = _oracle_hits(T, ref_len, positions=q, Bool=Bool)
            pm, nm = D.masks_of(q, L, ref_len)
            got = np.nonzero(D.flags_of(T, 0, pos_mode=mode, pos_mask=pm, not_mask=nm)[2])[0]
            assert np.array_equal(got, want), (q, Bool)
            if i < counted:
                total += 1
                solid += 0 < len(want) < N
    print(f"non-trivial position queries at L={L} A={A} ref_len={ref_len}: {solid}/{total} = {solid / total:.2f}")
    assert 4 * solid >= 3 * total, (solid, total)


@pytest.mark.parametrize("shape", [(L, D.letters_of(bits)) for L, bits in D.SHAPES], ids=lambda v: f"L{v[0]}_A{v[1]}")
def test_reference_is_the_oracle_on_distances(shape):
    L, A = shape
    T = D.ladder(L, A, seed=2000 + L)
    n = len(T)
    assert np.array_equal(T[0], T[n // 2]) and np.array_equal(T[0], T[n - 1])
    d, hist, _ = D.flags_of(T, 0)
    wanted = sorted({x for x in D.LADDER_DISTANCES if x <= L} | {L})
    assert sorted(np.unique(d)) == wanted and hist.sum() == n and hist[0] == 6
    assert all(hist[x] == 3 for x in wanted[1:])
    for want in [[x] for x in wanted] + [D.want_per_word(d), wanted]:
        got = np.nonzero(D.flags_of(T, 0, want=want)[2])[0]
        assert np.array_equal(got, O.indexing(T, 0, L, distances=want)), want
    # a distance and a position together, from another reference row
    ref = 4 if n > 4 else 0
    for q in ([0], [L - 1]):
        pm, nm = D.masks_of(q, L, L)
        dref = D.flags_of(T, ref)[0]
        for x in np.unique(dref)[:4]:
            got = np.nonzero(D.flags_of(T, ref, want=[int(x)], pos_mode=1, pos_mask=pm, not_mask=nm)[2])[0]
            try:
                want = O.indexing(T, ref, L, distances=[int(x)], positions=q)
            except AssertionError:
                want = np.zeros(0, dtype=np.int64)
            assert np.array_equal(got, want), (q, x)


def test_generators_put_the_mutations_where_they_say():
    assert D.edges(1) == [0] and D.edges(3) == [0, 1, 2] and D.edges(32) == [0, 1, 30, 31]
    assert D.edges(33) == [0, 1, 31, 32] and D.edges(65) == [0, 1, 31, 32, 63, 64]
    assert D.edges(255) == [0, 1] + [x for w in range(32, 255, 32) for x in (w - 1, w)] + [253, 254]
    T = D.library(N, 97, 200, seed=5, ref_len=72)
    mut = T != T[0]
    assert not T[0, 72:].any() and T[0, :72].all() and T.max() > 31
    assert set(np.nonzero(mut[:, :72].any(0))[0]) <= set(D.edges(72)) and mut[:, :72].sum(1).max() == 3
    long = np.nonzero(mut[:, 72:].any(1))[0]
    assert np.array_equal(long, np.arange(3, N, 3)) and T[long][:, 72:].all()
    assert all((T[i, :72][mut[i, :72]] == 0).all() for i in range(7, N, 7)) and (T[7::7, :72] == 0).any()
    assert np.array_equal(D.row_lengths(T, 72), np.where((np.arange(N) % 3 == 0) & (np.arange(N) > 0), 97, 72))
    for L, bits in D.SHAPES:
        rows = 0
        for P, where in D.plane_blocks(L, bits):
            assert P.min() >= 1 and P.max() < (1 << bits)
            for r, j, p in where:
                diff = np.nonzero(P[r] != P[0])[0]
                assert list(diff) == [j] and (int(P[r, j]) ^ int(P[0, j])) == 1 << p
            rows += len(where)
        assert rows == bits * len(D.edges(L))


SURFACE = [("lib", 3, D.LETTERS_20, None), ("lib", 33, D.LETTERS_20, None), ("lib", 65, D.LETTERS_20, 48),
           ("lib", 255, D.LETTERS_20, None), ("lib", 255, D.LETTERS_20, 191), ("lib", 97, D.LETTERS_40, 72),
           ("lib", 128, D.LETTERS_40, None), ("ladder", 65, D.LETTERS_20, None), ("ladder", 255, D.LETTERS_20, None),
           ("ladder", 128, D.LETTERS_40, None)]


@pytest.mark.parametrize("case", SURFACE, ids=lambda c: f"{c[0]}_L{c[1]}_A{len(c[2])}" + (f"_ref{c[3]}" if c[3] else ""))
def test_surface_host_logic(case, monkeypatch, tmp_path, capsys):
    """Prograph on the libraries and ladders, the kernel answered by tests/fake_native.py: what is under test is the
    host side - masks from positions, negative positions, the reference row's own length, the distance assertion,
    the comparators' distance sets, the complement."""
    import fake_native
    fake_native.install(monkeypatch)
    from prograph_amd import Prograph
    kind, L, letters, short = case
    T = D.library(400, L, len(letters), seed=3000 + L, ref_len=short) if kind == "lib" else D.ladder(L, len(letters), seed=3000 + L)
    lens = D.row_lengths(T, short)
    f = tmp_path / "index.csv"
    pd.DataFrame({"Sequence": D.strings(T, letters, lens), "Fitness": np.linspace(0, 1, len(T))}).to_csv(f)
    pg = Prograph(file=str(f), amino_acids=letters)
    out = capsys.readouterr().out
    d0 = (T != T[0]).sum(1)
    assert f"Max Distance        : {d0.max()}" in out and f"Number of Distances : {len(np.unique(d0))}" in out
    if len(letters) > 31:
        assert T.max() > 31
    assert pg._planes_or_none() is not None
    solid = D.surface_checks(pg, T, lens, O)
    assert solid > 20


def test_position_bitmask_words_and_bits():
    from prograph_amd import _native
    for p, (w, b) in {0: (0, 0), 31: (0, 31), 32: (1, 0), 63: (1, 31), 64: (2, 0), 254: (7, 30)}.items():
        m = _native.position_bitmask([p], 8)
        want = np.zeros(8, dtype=np.uint32)
        want[w] = np.uint32(1) << np.uint32(b)
        assert m.dtype == np.uint32 and np.array_equal(m, want), p
    every = _native.position_bitmask([0, 31, 32, 63, 64, 254], 8)
    assert list(every) == [0x80000001, 0x80000001, 1, 0, 0, 0, 0, 0x40000000]
    assert np.array_equal(_native.position_bitmask([5, 5, 37, 5, 37], 2), _native.position_bitmask([37, 5], 2))
    assert not _native.position_bitmask([], 3).any() and len(_native.position_bitmask([], 3)) == 3
    for g in (1, 2, 4, 8):
        assert _native.position_bitmask([32 * g - 1], g)[g - 1] == 0x80000000
        for bad in (-1, 32 * g):
            with pytest.raises(IndexError):
                _native.position_bitmask([bad], g)
