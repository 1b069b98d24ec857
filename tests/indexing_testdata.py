"""
Data and reference for the pins of the fused index kernel (`pg_index_kernel<5>` / `<8>` behind `pg_index_flags`,
`_native.index_flags` and `Prograph.indexing` / `positions` / `distances` / `calc_neighbours` / `neighbourhood`).

The kernel reads up to eight 32-position groups, ORs 5 or 8 bit planes per group, tests one mask word per group,
looks the distance up in a 256-bit set of eight words and feeds a 256-bin histogram.  The generators below put
mutations where that can go wrong: the first and last positions, both sides of every 32-position word seam, every
bit plane on its own, every word of the distance set, an unknown letter (token 0), and a reference row shorter than
the matrix.

`flags_of` is the reference: plain numpy on the int64 token matrix.  Nothing here imports the package under test;
`surface_checks` is handed the `Prograph` object it drives.
"""
import itertools
import operator

import numpy as np

LETTERS_20 = "ACDEFGHIKLMNPQRSTVWY"
LETTERS_40 = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmn"      # tokens 32..40 need the 8-plane records
UNKNOWN = "#"                                                 # in neither alphabet: tokenises to 0

# (L, bits) of the kernel pins: one group / many, both sides of every limit, both instantiations
SHAPES = [(1, 5), (3, 5), (31, 5), (32, 5), (33, 5), (64, 5), (65, 5), (96, 5), (128, 5), (129, 5), (224, 5), (255, 5),
          (1, 8), (32, 8), (33, 8), (97, 8), (128, 8)]
LADDER_DISTANCES = (0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 127, 128, 159, 160, 191, 192, 223, 224, 254, 255)


def letters_of(bits):
    """Tokens 1..A of the data of a `bits`-plane shape: 200 at 8 planes, so that planes 5..7 carry information."""
    return 20 if bits == 5 else 200


def short_ref(L):
    """The length of the short reference of a shape, about 3L/4 (None below 33 positions)."""
    return (3 * L) // 4 if L >= 33 else None


def edges(l):
    """{0, 1, l-2, l-1} and {w-1, w} for every multiple w of 32 below l, ascending, inside 0..l-1."""
    s = {0, 1, l - 2, l - 1}
    for w in range(32, l, 32):
        s |= {w - 1, w}
    return sorted(p for p in s if 0 <= p < l)


def _other(rng, tok, A):
    """A letter of 1..A that is not `tok`."""
    return 1 + (int(tok) - 1 + int(rng.integers(1, A))) % A


def library(n, L, A, seed, ref_len=None):
    """(n, L) int64 mutant library around row 0 (see the module docstring and the issue text in the test files):
    row 0 is the base cut to `ref_len` and zero padded; every other row mutates 0..3 positions of `edges(ref_len)`,
    every seventh to token 0; with a short reference every third row keeps letters past `ref_len`."""
    rng = np.random.default_rng(seed)
    ref_len = L if ref_len is None else int(ref_len)
    full = rng.integers(1, A + 1, L)
    base = full.copy()
    base[ref_len:] = 0
    T = np.tile(base, (n, 1)).astype(np.int64)
    pool = edges(ref_len)
    for i in range(1, n):
        k = min(int(rng.integers(0, 4)), len(pool))
        for p in rng.choice(pool, size=k, replace=False):
            T[i, p] = 0 if i % 7 == 0 else _other(rng, base[p], A)
        if ref_len < L and i % 3 == 0:
            T[i, ref_len:] = rng.integers(1, A + 1, L - ref_len)
    return T


def ladder(L, A, seed):
    """(n, L) int64: for every d of LADDER_DISTANCES up to L, and d = L, three rows at exactly distance d from the base
    (the first d positions, the last d, a random set of d); the base itself at rows 0, n // 2 and n - 1."""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, A + 1, L).astype(np.int64)
    rows = []
    for d in sorted({x for x in LADDER_DISTANCES if x <= L} | {L}):
        for pos in (np.arange(d), np.arange(L - d, L), rng.choice(L, size=d, replace=False)):
            r = base.copy()
            for p in pos:
                r[p] = _other(rng, base[p], A)
            rows.append(r)
    n = len(rows) + 3
    T = np.empty((n, L), dtype=np.int64)
    bases = (0, n // 2, n - 1)
    it = iter(rows)
    for i in range(n):
        T[i] = base if i in bases else next(it)
    return T


def plane_rows(L, bits, planes=None):
    """One bit plane at a time.  Row 0 is the constant token t0; for every plane p of `planes` and every position j
    of `edges(L)` one row equals it except T[j] = t0 ^ (1 << p): distance exactly 1, mutated at exactly j, in plane
    p only.  t0 = 2 for plane 0 and 1 for the others, so no token becomes a padding 0 by accident - which is why the
    planes come in the two blocks of `plane_blocks`.  Returns (T, [(row, j, p), ...])."""
    planes = list(range(bits)) if planes is None else list(planes)
    t0 = 2 if planes == [0] else 1
    assert 0 not in planes or planes == [0]
    rows, where = [np.full(L, t0, dtype=np.int64)], []
    for p in planes:
        for j in edges(L):
            r = rows[0].copy()
            r[j] = t0 ^ (1 << p)
            where.append((len(rows), j, p))
            rows.append(r)
    return np.stack(rows), where


def plane_blocks(L, bits):
    """The two `plane_rows` matrices that cover every plane below `bits`: plane 0 around t0 = 2, the rest around 1."""
    return [plane_rows(L, bits, [0]), plane_rows(L, bits, range(1, bits))]


def position_queries(pool, ref_len=None, L=None):
    """Every single position of the pool, the first 40 pairs, then the extras: a duplicate, [-1], and - with a short
    reference - the last position of the reference with the first one past it.  Returns (queries, n_counted): the
    extras are the queries from n_counted on."""
    qs = [[p] for p in pool] + [list(c) for c in itertools.islice(itertools.combinations(pool, 2), 40)]
    counted = len(qs)
    qs += [[pool[0], pool[0]], [-1]]
    if ref_len is not None and L is not None and ref_len < L:
        qs.append([ref_len - 1, ref_len])
    return qs, counted


def masks_of(positions, L, ref_len):
    """The two position lists `Prograph.indexing` hands the kernel (reference :316): selected, must-not-differ."""
    return [p % L for p in positions], [p for p in range(ref_len) if p not in positions]


def flags_of(T, ref, want=None, pos_mode=0, pos_mask=(), not_mask=()):
    """(d, bincount(d, 256), ok) of the fused pass, in plain numpy on the int64 token matrix."""
    T = np.asarray(T, dtype=np.int64)
    mut = T != T[ref]
    d = mut.sum(1)
    ok = np.ones(len(T), dtype=bool)
    if want is not None:
        ok &= np.isin(d, np.asarray(list(want), dtype=np.int64))
    if pos_mode:
        sel = mut[:, list(pos_mask)]
        ok &= sel.any(1) if pos_mode == 1 else sel.all(1)
        ok &= ~mut[:, list(not_mask)].any(1)
    return d, np.bincount(d, minlength=256), ok


def want_per_word(d):
    """One distance of `d` in each of the eight 32-distance words that `d` reaches: the largest of each word."""
    present = np.unique(d)
    return [int(present[present >> 5 == w].max()) for w in range(8) if np.any(present >> 5 == w)]


def row_lengths(T, ref_len=None):
    """String length of every row: the matrix width, or `ref_len` for a row that is padded past a short reference."""
    L = T.shape[1]
    if ref_len is None or ref_len >= L:
        return np.full(len(T), L)
    return np.where((T[:, ref_len:] != 0).any(1), L, ref_len)


def strings(T, letters, lens):
    """The rows as strings over `letters` (token t -> letters[t - 1]); token 0 inside a row's length is an unknown letter."""
    lut = np.array([UNKNOWN] + list(letters))
    return ["".join(lut[r[:n]]) for r, n in zip(np.asarray(T), lens)]


CMPS = (operator.le, operator.lt, operator.eq, operator.ge, operator.gt)


def surface_checks(pg, T, lens, O, few=12):
    """Drive the index surface of the `Prograph` object `pg`, built on the strings of `T`, against the oracle module
    `O` (the restatement of the reference's :254-343, :526-544, :571-588) and plain numpy: every position query of
    row 0 under both `Bool` values, `few` of them for a middle and the last row, distances in every word of the
    distance set, both together, the complement, the shorthands, the five comparators at an integer and a
    half-integer eps, the neighbourhood, and the assertions for a distance that is absent or beyond 255.
    Returns the number of compared answers that were neither empty nor everything."""
    import pytest
    T = np.asarray(T, dtype=np.int64)
    n, L = T.shape
    assert np.array_equal(pg.tokenized, T)
    solid = 0

    def same(kw, ref):
        nonlocal solid
        okw = {k: v for k, v in kw.items() if k != "reference_seq"}
        try:
            want = O.indexing(T, ref, int(lens[ref]), **okw)
        except AssertionError:
            with pytest.raises(AssertionError):
                pg.indexing(**kw)
            return
        got = pg.indexing(**kw)
        if isinstance(want, tuple):
            assert isinstance(got, tuple) and len(got) == 2, kw
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), kw
            want = want[0]
        else:
            assert got.dtype == np.int64 and np.array_equal(got, want), (kw, ref)
        solid += 0 < len(want) < n

    for ref in (0, n // 2, n - 1):
        ref_len = int(lens[ref])
        d = (T != T[ref]).sum(1)
        present = [int(x) for x in np.unique(d)]
        qs, _ = position_queries(edges(ref_len), ref_len, L)
        for q in (qs if ref == 0 else qs[:few // 2] + qs[-few // 2:]):
            for mode in ("or", "and"):
                same(dict(reference_seq=ref, positions=q, Bool=mode), ref)
        words = want_per_word(d)
        same(dict(reference_seq=ref, distances=words), ref)
        for x in present[:3] + words:
            same(dict(reference_seq=ref, distances=x), ref)
        for q in qs[:few]:
            for mode in ("or", "and"):
                same(dict(reference_seq=ref, positions=q, distances=present[:4], Bool=mode), ref)
                same(dict(reference_seq=ref, positions=q, distances=present[1:3], Bool=mode, complement=True), ref)
        same(dict(reference_seq=ref, distances=present[-2:], complement=True), ref)
        absent = next(x for x in range(256) if x not in present) if len(present) < 256 else None
        for bad in (absent, 256, 300):
            if bad is not None and bad not in present:
                with pytest.raises(AssertionError):
                    pg.indexing(reference_seq=ref, distances=[present[0], bad])
        for eps in (2, 1.5, float(present[-1]) - 0.5, present[-1]):
            for comp in CMPS:
                got = pg.calc_neighbours(ref, eps=eps, comp=comp)
                assert np.array_equal(got, np.nonzero(comp(d, eps))[0]), (ref, eps, comp)
                assert np.array_equal(got, O.calc_neighbours(T, ref, eps=eps, comp=comp)), (ref, eps, comp)
        for eps in (0, 1, 2.5, present[-1]):
            assert list(pg.neighbourhood(ref, eps).index) == list(np.nonzero(d <= eps)[0]), (ref, eps)

    # the shorthands answer for the seed, row 0 (or a later copy of it: the same tokens, the same answers)
    pool = edges(int(lens[0]))
    d0 = (T != T[0]).sum(1)
    for q in ([pool[0]], pool[-2:]):
        try:
            want = O.indexing(T, 0, int(lens[0]), positions=q)
        except AssertionError:
            with pytest.raises(AssertionError):
                pg.positions(q)
        else:
            assert np.array_equal(pg.positions(q), want)
    words = want_per_word(d0)
    assert np.array_equal(pg.distances(words), O.indexing(T, 0, int(lens[0]), distances=words))
    assert np.array_equal(pg.distances(words[-1]), np.nonzero(d0 == words[-1])[0])
    return solid
