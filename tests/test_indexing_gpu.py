"""
The fused index kernel on the GPU, `pg_index_kernel<5>` / `<8>` behind `pg_index_flags`, against the plain numpy
reference `flags_of` of tests/indexing_testdata.py (which tests/test_indexing_cpu.py ties to the reference project's
indexing): bit for bit, at every group count from one to eight, both plane counts, every word of the position masks
and of the 256-bit distance set, distances up to 255, reference rows other than row 0 and shorter than the matrix,
row counts around the workgroup of 256, many workgroups on the histogram, every output selection, the argument checks,
and `Prograph`'s index surface on both sides of the two width limits (255 | 256 positions, 128 | 129 with tokens
above 31), where the kernel hands over to torch ops.
"""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch

import indexing_testdata as D
from oracle import prograph_oracle as O
from prograph_amd import _native

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

N = 600
ONLY = dict(want_dist_out=False, want_hist=False)


def _pack(T, bits):
    return _native.pack(torch.from_numpy(np.ascontiguousarray(T)), bits=bits)


def _flags(p, ref, **kw):
    d, h, f = _native.index_flags(p, ref, **ONLY, **kw)
    assert d is None and h is None and f.dtype == torch.uint8 and f.shape == (p.n,)
    return f.cpu().numpy()


def _check_matrix(T, bits, ref, ref_len, queries=True):
    """Everything `index_flags` returns for reference row `ref` of `T` against `flags_of`.  Returns the planes."""
    n, L = T.shape
    p = _pack(T, bits)
    assert (p.n, p.l, p.bits, p.g) == (n, L, bits, (L + 31) // 32)
    d, hist, _ = D.flags_of(T, ref)
    dist, h, fl = _native.index_flags(p, ref)
    assert dist.dtype == torch.uint8 and dist.shape == (n,) and np.array_equal(dist.cpu().numpy(), d)
    assert h.dtype == torch.int64 and h.shape == (256,) and np.array_equal(h.cpu().numpy(), hist) and int(h.sum()) == n
    assert fl.dtype == torch.uint8 and np.array_equal(fl.cpu().numpy(), np.ones(n, dtype=np.uint8))       # want=None: every row
    # one output at a time: what is not asked for is None, what is asked for is the same
    only = _native.index_flags(p, ref, want_hist=False, want_flags=False)
    assert only[1] is None and only[2] is None and np.array_equal(only[0].cpu().numpy(), d)
    only = _native.index_flags(p, ref, want_dist_out=False, want_flags=False)
    assert only[0] is None and only[2] is None and np.array_equal(only[1].cpu().numpy(), hist)
    # the distance set: a member in every word the data reaches, everything present, nothing, values outside 0..255
    words = D.want_per_word(d)
    for want in [words, [int(x) for x in np.unique(d)], [words[-1]], [], [300, -1], [300, -1, words[0], 256 + words[-1]]]:
        got = _flags(p, ref, want=want)
        assert np.array_equal(got, D.flags_of(T, ref, want=want)[2]), (want, np.nonzero(got)[0][:8])
    assert not _flags(p, ref, want=[]).any() and not _flags(p, ref, want=[300, -1]).any()
    if not queries:
        return p
    # the position masks, alone and with a distance set
    qs, _ = D.position_queries(D.edges(ref_len), ref_len, L)
    both = sorted(set(words) | {1, 2})
    for q in qs:
        pm, nm = D.masks_of(q, L, ref_len)
        for mode in (1, 2):
            for want in (None, both):
                got = _flags(p, ref, want=want, pos_mode=mode, pos_mask=pm, not_mask=nm)
                ok = D.flags_of(T, ref, want=want, pos_mode=mode, pos_mask=pm, not_mask=nm)[2]
                assert np.array_equal(got, ok), (q, mode, want, np.nonzero(got != ok)[0][:8])
    return p


@pytest.mark.parametrize("L,bits", D.SHAPES)
def test_kernel_against_reference(L, bits):
    A = D.letters_of(bits)
    T = D.library(N, L, A, seed=4000 + L)
    assert bits == 5 or T.max() > 127
    _check_matrix(T, bits, 0, L)
    _check_matrix(T, bits, 595, L, queries=L in (33, 255, 128))            # an unknown-letter row (595 = 7 * 85) as the reference
    short = D.short_ref(L)
    if short:
        _check_matrix(D.library(N, L, A, seed=4100 + L, ref_len=short), bits, 0, short)
    R = D.ladder(L, A, seed=4200 + L)
    _check_matrix(R, bits, 0, L)
    _check_matrix(R, bits, len(R) // 2 + 1, L, queries=False)            # a far row as the reference: other distances


@pytest.mark.parametrize("L,bits", D.SHAPES)
def test_every_plane_at_every_edge(L, bits):
    """A row that differs from the reference in ONE bit plane at ONE position is at distance 1 and is flagged by the
    query for that position alone, under either mode: a dropped plane, or a plane read from the wrong word, fails."""
    hit = {(j, mode): 0 for j in D.edges(L) for mode in (1, 2)}
    for P, where in D.plane_blocks(L, bits):
        p = _check_matrix(P, bits, 0, L, queries=False)
        dist, _, _ = _native.index_flags(p, 0, want_hist=False, want_flags=False)
        dist = dist.cpu().numpy()
        assert dist[0] == 0 and np.array_equal(dist[1:], np.ones(len(P) - 1, dtype=np.uint8))
        for j in D.edges(L):
            pm, nm = D.masks_of([j], L, L)
            mine = [r for r, jj, _ in where if jj == j]
            for mode in (1, 2):
                got = np.nonzero(_flags(p, 0, pos_mode=mode, pos_mask=pm, not_mask=nm))[0]
                assert list(got) == mine, (j, mode)
                assert np.array_equal(got, np.nonzero(D.flags_of(P, 0, pos_mode=mode, pos_mask=pm, not_mask=nm)[2])[0])
                hit[j, mode] += len(got)
    assert all(v == bits for v in hit.values()), hit


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1000])
def test_row_counts_and_reference_rows(n):
    L = 65
    T = D.library(n, L, 20, seed=4300 + n)
    R = D.ladder(L, 20, seed=4400 + n)
    R = R[np.arange(n) % len(R)]                                            # the ladder, repeated or cut to n rows
    for ref in sorted({r for r in (0, 255, 256, n - 1) if r < n}):
        _check_matrix(T, 5, ref, L, queries=ref in (0, n - 1))
        _check_matrix(R, 5, ref, L, queries=False)


def test_many_workgroups_on_the_histogram():
    """66 000 rows, 258 workgroups: every one of them adds its LDS bins to the same 256 global counters."""
    L, blocks = 65, 110
    T = np.concatenate([D.library(N, L, 20, seed=4500 + b if b % 10 else 4500) for b in range(blocks)])
    R = D.ladder(L, 20, seed=4500)                                          # the same seed, the same base row as every tenth block
    T[N * 50:N * 51] = R[np.arange(N) % len(R)]
    assert T.shape == (blocks * N, L)
    ref = N * 50 + 300
    p = _pack(T, 5)
    d, hist, _ = D.flags_of(T, ref)
    dist, h, _ = _native.index_flags(p, ref, want_flags=False)
    assert np.array_equal(dist.cpu().numpy(), d)
    assert np.array_equal(h.cpu().numpy(), hist) and int(h.sum()) == len(T) and np.count_nonzero(hist) >= 16
    pm, nm = D.masks_of([32, 63], L, L)
    for mode in (1, 2):
        got = _flags(p, ref, want=[1, 2, 3, 33, 64], pos_mode=mode, pos_mask=pm, not_mask=nm)
        ok = D.flags_of(T, ref, want=[1, 2, 3, 33, 64], pos_mode=mode, pos_mask=pm, not_mask=nm)[2]
        assert np.array_equal(got, ok) and 0 < ok.sum() < len(T)


def _ptr(t, offset=0):
    return ctypes.c_void_p(0) if t is None else ctypes.c_void_p(t.data_ptr() + offset)


def test_direct_call_writes_its_outputs_and_nothing_else():
    L, n, tail = 65, 257, 64
    T = D.library(n, L, 20, seed=4600)
    p = _pack(T, 5)
    dev = p.buf.device
    dist = torch.full((n + tail,), 0xA5, dtype=torch.uint8, device=dev)
    flags = torch.full((n + tail,), 0x5A, dtype=torch.uint8, device=dev)
    hist = torch.zeros(256 + 8, dtype=torch.int64, device=dev)
    hist[256:] = -7
    want = np.zeros(8, dtype=np.uint32)
    want[0] = 0b0110                                                        # distances 1 and 2
    pm, nm = D.masks_of([31, 32], L, L)
    dw, dp, dn = (torch.from_numpy(a.view(np.int32)).to(dev)
                  for a in (want, _native.position_bitmask(pm, p.g), _native.position_bitmask(nm, p.g)))
    rc = _native.lib().pg_index_flags(_ptr(p.buf), n, p.npad, L, 5, 3, _ptr(dw), 1, _ptr(dp), _ptr(dn), _ptr(dist), _ptr(hist),
                                      _ptr(flags), _native._stream())
    assert rc == 0, _native.lib().pg_last_error()
    torch.cuda.synchronize()
    d, h, ok = D.flags_of(T, 3, want=[1, 2], pos_mode=1, pos_mask=pm, not_mask=nm)
    assert np.array_equal(dist[:n].cpu().numpy(), d) and bool((dist[n:] == 0xA5).all())
    assert np.array_equal(flags[:n].cpu().numpy(), ok) and bool((flags[n:] == 0x5A).all()) and ok.any()
    assert np.array_equal(hist[:256].cpu().numpy(), h) and bool((hist[256:] == -7).all())


def test_argument_errors_return_before_a_launch():
    """Every bad argument is refused with a message, and no output byte changes.  The plane buffer is larger than any
    of these calls could read if it were launched after all, with a row in front of row 0."""
    L, n = 255, 300
    T = D.library(n, L, 20, seed=4700)
    npad = _native.npad(n)
    chunk = 16 * npad                                                       # bytes of one chunk array
    p = _pack(T, 5)
    dev = p.buf.device
    room = torch.zeros(chunk * 19, dtype=torch.uint8, device=dev)
    room[chunk:chunk + p.buf.numel()] = p.buf
    dist = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
    flags = torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)
    hist = torch.full((256,), -7, dtype=torch.int64, device=dev)
    masks = torch.zeros(8, dtype=torch.int32, device=dev)
    lib = _native.lib()

    def call(n_=n, npad_=npad, l=L, bits=5, ref=0, mode=0, pm=None, nm=None):
        return lib.pg_index_flags(_ptr(room, chunk), n_, npad_, l, bits, ref, None, mode, _ptr(pm), _ptr(nm), _ptr(dist),
                                  _ptr(hist), _ptr(flags), _native._stream())

    cases = [("ref = -1", dict(ref=-1), "bad argument"), ("pos_mode = 3", dict(mode=3, pm=masks, nm=masks), "position mode"),
             ("ref = n", dict(ref=n), "bad argument"), ("bits = 6", dict(bits=6), "bits must be 5 or 8"),
             ("npad < n", dict(npad_=256), "bad argument"), ("pos_mode 1, no masks", dict(mode=1), "position mode"),
             ("l = 256 with 5 bits", dict(l=256), "native limit"), ("pos_mode 2, one mask", dict(mode=2, pm=masks), "position mode"),
             ("l = 129 with 8 bits", dict(l=129, bits=8), "native limit")]
    for name, kw, message in cases:
        rc = call(**kw)
        assert rc != 0, name
        assert message in lib.pg_last_error().decode(), (name, lib.pg_last_error())
    torch.cuda.synchronize()
    assert bool((dist == 0xA5).all()) and bool((flags == 0x5A).all()) and bool((hist == -7).all())
    assert call() == 0                                                     # the same operands, good arguments: it runs
    torch.cuda.synchronize()
    assert np.array_equal(dist.cpu().numpy(), D.flags_of(T, 0)[0])
    with pytest.raises(RuntimeError, match="bad argument"):
        _native.index_flags(p, n)
    with pytest.raises(IndexError):
        _native.index_flags(p, 0, pos_mode=1, pos_mask=[256], not_mask=[])


# (kind, width, letters, the kernel runs): both sides of 255 | 256 and, with tokens above 31, of 128 | 129
SURFACE = [("lib", 255, D.LETTERS_20, True), ("lib", 256, D.LETTERS_20, False), ("lib", 128, D.LETTERS_40, True),
           ("lib", 129, D.LETTERS_40, False), ("ladder", 255, D.LETTERS_20, True), ("ladder", 256, D.LETTERS_20, False),
           ("ladder", 128, D.LETTERS_40, True), ("ladder", 129, D.LETTERS_40, False)]


@pytest.mark.parametrize("case", SURFACE, ids=lambda c: f"{c[0]}_L{c[1]}_A{len(c[2])}")
def test_surface_on_both_sides_of_the_limits(case, tmp_path, capsys):
    from prograph_amd import Prograph
    kind, L, letters, fused = case
    short = None if kind == "ladder" else (3 * L) // 4
    T = D.library(400, L, len(letters), seed=4800, ref_len=short) if kind == "lib" else D.ladder(L, len(letters), seed=4800)
    assert len(letters) < 32 or T.max() > 31
    lens = D.row_lengths(T, short)
    f = tmp_path / "index.csv"
    pd.DataFrame({"Sequence": D.strings(T, letters, lens), "Fitness": np.linspace(0, 1, len(T))}).to_csv(f)
    pg = Prograph(file=str(f), amino_acids=letters)
    out = capsys.readouterr().out
    d0 = (T != T[0]).sum(1)
    assert f"Max Distance        : {d0.max()}" in out and f"Number of Distances : {len(np.unique(d0))}" in out
    assert (pg._planes_or_none() is not None) == fused
    assert D.surface_checks(pg, T, lens, O) > 20
