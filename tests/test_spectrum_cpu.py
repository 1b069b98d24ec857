"""
The k-mer spectrum distance without a GPU: the kernel's window routine compiled for the host under the
sanitizers (tests/capi_spectrum), the argument checks of the operator and of the C ABI, and the operator's torch
expression on CPU tensors against the `collections.Counter` definition of tests/spectrum_testdata.py.  The kernel and the
routes of `build_graph` / `search`: tests/test_spectrum_gpu.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
from spectrum_testdata import bucket_of, d2_of, euclid_of, profile, profiles
from prograph_amd.distance import cosine, euclidean, spectrum


def test_the_window_routine_on_the_host():
    """tests/capi_spectrum/spectrum_check.cpp: pg_spectrum.h compiled for the host with -fsanitize=address,undefined against
    a naive counter - every sequence over {0, 1, 2} and {0, 1, 2, 3} of lengths 0..7 for k = 1..4, exact and dims = 64;
    random rows at lengths {0, k-1, k, k+1, 63, 64, 65, 2048} with 2, 20, 31 and 255 symbols and k up to 6; the hash
    against the formula in 64-bit arithmetic."""
    capi = os.path.join(REPO, "tests", "capi_spectrum")
    subprocess.check_call(["make", "-s", "-C", capi])
    out = subprocess.run([os.path.join(capi, "_build", "spectrum_check")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "spectrum routines OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_operator_argument_errors():
    for bad in (dict(k=0), dict(k=7), dict(symbols=1), dict(symbols=256), dict(k=6, symbols=36, dims=64), dict(k=4, symbols=216, dims=64),
                dict(k=3, symbols=33), dict(k=4, symbols=20), dict(dims=32), dict(dims=65536), dict(dims=96), dict(dims=-64),
                dict(metric="minkowski"), dict(metric=None)):
        with pytest.raises(ValueError):
            spectrum(**bad)
    assert spectrum().D == 8000 and spectrum(k=3, symbols=32).D == 32768 and spectrum(k=6, symbols=20, dims=1024).D == 1024
    assert spectrum(k=4, symbols=215, dims=64).D == 64 and spectrum(k=1, symbols=2).D == 2 and spectrum(dims=0).D == 8000
    op = spectrum(k=2, symbols=4, metric="euclidean")
    assert (op.k, op.symbols, op.dims, op.metric, op.D) == (2, 4, 0, "euclidean", 16) and op.plain is euclidean
    assert spectrum().plain is cosine


def test_c_abi_argument_errors_without_gpu():
    from prograph_amd import _native
    lib = _native.lib()
    assert lib.pg_spectrum_dims(3, 20, 0) == 8000 and lib.pg_spectrum_dims(3, 32, 0) == 32768
    assert lib.pg_spectrum_dims(3, 33, 0) == -1 and lib.pg_spectrum_dims(6, 20, 1024) == 1024
    for k, symbols, dims in ((0, 20, 0), (7, 2, 0), (2, 1, 0), (2, 256, 0), (6, 36, 64), (4, 216, 64), (2, 20, 32), (2, 20, 65536),
                             (2, 20, 96), (2, 20, -64), (4, 20, 0)):
        assert lib.pg_spectrum_dims(k, symbols, dims) == -1, (k, symbols, dims)
    p = ctypes.c_void_p(256)                                              # never dereferenced: every check is on the host

    def call(tokens=p, n=4, l=20, ld=20, rows=None, k=3, symbols=20, dims=0, out=p, ldo=8000, flags=p):
        return lib.pg_spectrum_profile(tokens, n, l, ld, rows, k, symbols, dims, out, ldo, flags, None)

    for bad in (dict(tokens=None), dict(out=None), dict(flags=None), dict(n=0), dict(n=-1), dict(l=0), dict(ld=19), dict(ldo=7999),
                dict(k=0), dict(k=7), dict(symbols=1), dict(symbols=256), dict(symbols=33), dict(dims=32), dict(dims=96),
                dict(dims=65536), dict(k=6, symbols=36, dims=64), dict(dims=64, ldo=63)):
        assert call(**bad) == -1, bad
    assert call(l=2049, ld=2049) == -2 and b"2048" in lib.pg_last_error()
    assert call(l=2049, ld=2048) == -1                                    # the argument checks come first


K_CASES = [(1, 3, 0), (2, 4, 0), (3, 20, 0), (3, 20, 64), (5, 20, 1024), (6, 31, 32768)]


@pytest.mark.parametrize("k,symbols,dims", K_CASES)
def test_embed_on_cpu_tensors_is_the_definition(k, symbols, dims):
    op = spectrum(k=k, symbols=symbols, dims=dims or None)
    rng = np.random.default_rng(k * 100 + symbols)
    width = 70
    T = np.zeros((9, width), dtype=np.int64)
    for r, l in enumerate((0, k - 1, k, k + 1, 63, 64, 65, 70, 70)):
        T[r, :l] = rng.integers(1, symbols + 1, l)
    T[7, rng.integers(0, width, 12)] = 0                                  # interior zeros
    T[8, :] = symbols                                                     # one repeated letter: the highest code
    want = profiles(T, k, symbols, dims)
    assert want[0].sum() == 0 and want[1].sum() == 0 and want[2].sum() == 1 and want[8].max() == width - k + 1
    assert 0 < want[7].sum() < width - k + 1
    for tokens in (torch.from_numpy(T), T, torch.from_numpy(T).to(torch.uint8), torch.from_numpy(T).to(torch.float16)):
        got = op.embed(tokens)
        assert got.dtype == torch.float16 and got.shape == (9, op.D) and got.device.type == "cpu"
        assert np.array_equal(got.numpy().astype(np.int64), want)
    # one row; rows of length 0, k - 1 and k on their own
    assert np.array_equal(op.embed(T[5]).numpy().astype(np.int64), want[5:6])
    for l in (0, k - 1, k):
        row = rng.integers(1, symbols + 1, l)
        got = op.embed(torch.from_numpy(row))
        assert got.shape == (1, op.D) and np.array_equal(got.numpy()[0].astype(np.int64), profile(row, k, symbols, dims))
        assert int(got.sum()) == (1 if l == k else 0)


def test_the_largest_count_is_exact():
    T = np.full((1, 2048), 2, dtype=np.int64)
    got = spectrum(k=1, symbols=3).embed(T).numpy()
    assert got.tolist() == [[0.0, 2048.0, 0.0]]
    got = spectrum(k=6, symbols=3, dims=64).embed(T).numpy()[0]
    assert got.max() == 2043.0 and np.count_nonzero(got) == 1


def test_hashed_buckets_follow_the_formula():
    for k, symbols, dims in ((3, 20, 64), (5, 20, 1024), (6, 31, 32768), (2, 255, 4096)):
        op = spectrum(k=k, symbols=symbols, dims=dims)
        rng = np.random.default_rng(dims)
        for row in list(rng.integers(1, symbols + 1, (20, k))) + [np.full(k, 1), np.full(k, symbols)]:
            code = 0
            for t in row:
                code = code * symbols + int(t) - 1
            bucket = (((code + 1) * 2654435761) % (1 << 32)) >> (32 - (dims.bit_length() - 1))
            assert bucket == bucket_of(code, dims)
            got = op.embed(row).numpy()[0]
            assert got[bucket] == 1 and got.sum() == 1, (k, symbols, dims, row)


def test_embed_refuses_what_is_outside_the_contract():
    op = spectrum(k=2, symbols=4)
    with pytest.raises(ValueError):
        op.embed(np.array([[1, 2, 5, 1]]))                                # a token above `symbols`
    with pytest.raises(ValueError):
        op.embed(np.array([[1, -1, 2]]))
    with pytest.raises(ValueError):
        op.embed(np.array([[1, 300, 2]]))
    with pytest.raises(ValueError):
        op.embed(np.array([[1.5, 2.0]]))
    with pytest.raises(ValueError):
        op.embed(np.ones((2, 2049), dtype=np.int64))
    assert op.embed(np.ones((2, 2048), dtype=np.int64)).shape == (2, 16)
    with pytest.raises(ValueError):
        op(np.ones((2, 2049), dtype=np.int64), np.ones((1, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        op(np.ones((0, 4), dtype=np.int64), np.ones((1, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        op.embed(np.ones((2, 3, 4), dtype=np.int64))


def _tokens(n, width, symbols, seed, lo=0):
    rng = np.random.default_rng(seed)
    T = np.zeros((n, width), dtype=np.int64)
    for r in range(n):
        l = int(rng.integers(lo, width + 1))
        T[r, :l] = rng.integers(1, symbols + 1, l)
    return T


@pytest.mark.parametrize("k,symbols,dims", [(2, 4, 0), (3, 20, 0), (3, 20, 256)])
def test_euclidean_is_the_rounded_root_of_the_exact_integer(k, symbols, dims):
    """`metric="euclidean"` on CPU tensors: float32(sqrt(d2)) bit for bit, d2 from int64 counts; operands of different
    widths, and similarity = 1 / (1 + d)."""
    op = spectrum(k=k, symbols=symbols, dims=dims or None, metric="euclidean")
    X, Y = _tokens(40, 50, symbols, seed=1), _tokens(13, 31, symbols, seed=2)
    Y[3, :31] = X[7, :31]
    X[7, 31:] = 0                                                         # the same sequence at two widths: d = 0
    d2 = d2_of(profiles(X, k, symbols, dims), profiles(Y, k, symbols, dims))
    want = euclid_of(d2)
    got = op(torch.from_numpy(X), torch.from_numpy(Y))
    assert got.dtype == torch.float32 and got.shape == (13, 40)
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    assert got[3, 7] == 0 and d2[3, 7] == 0
    s = op(torch.from_numpy(X), torch.from_numpy(Y), similarity=True)
    assert np.array_equal(s.numpy().view(np.int32), (np.float32(1) / (np.float32(1) + want)).view(np.int32))
    assert np.array_equal(op(X, Y).numpy(), got.numpy())                  # arrays as well as tensors


def test_cosine_is_the_plain_metric_of_the_profiles_and_its_similarity():
    op = spectrum(k=2, symbols=4)
    X, Y = _tokens(30, 24, 4, seed=3, lo=2), _tokens(9, 40, 4, seed=4, lo=2)
    px = torch.from_numpy(profiles(X, 2, 4)).to(torch.float16)
    py = torch.from_numpy(profiles(Y, 2, 4)).to(torch.float16)
    d = op(torch.from_numpy(X), torch.from_numpy(Y))
    assert torch.equal(d, cosine(px, py)) and d.dtype == torch.float32 and d.shape == (9, 30)
    s = op(torch.from_numpy(X), torch.from_numpy(Y), similarity=True)
    assert torch.equal(s, 1 / (1 + d))
    # against the definition in float64: the sums are exact, the epilogue is a few float32 roundings
    a, b = profiles(X, 2, 4).astype(np.float64), profiles(Y, 2, 4).astype(np.float64)
    ref = 1 - (b @ a.T) / np.sqrt((a * a).sum(1))[None, :] / np.sqrt((b * b).sum(1))[:, None]
    assert np.abs(d.numpy() - ref).max() < 1e-6


def test_zero_profiles():
    """A row shorter than k, or with an unknown in every window: the zero profile.  Cosine gives it d = 1 to everything,
    itself and other zero profiles included; under Euclidean it is an ordinary point at sqrt(ny) from y, 0 from its like."""
    k = 3
    X = np.array([[1, 2, 3, 4, 1, 2], [1, 2, 0, 0, 0, 0], [1, 2, 0, 3, 4, 0], [0, 0, 0, 0, 0, 0], [4, 4, 4, 4, 0, 0]])
    P = profiles(X, k, 4)
    assert P[1].sum() == 0 and P[2].sum() == 0 and P[3].sum() == 0 and P[0].sum() == 4 and P[4].sum() == 2
    T = torch.from_numpy(X)
    d = spectrum(k=k, symbols=4)(T, T).numpy()
    for z in (1, 2, 3):
        assert np.all(d[z] == 1) and np.all(d[:, z] == 1)
    assert d[0, 0] == 0 and d[4, 4] == 0 and 0 < d[0, 4] <= 1
    assert np.all(spectrum(k=k, symbols=4)(T, T, similarity=True).numpy()[1] == 0.5)
    e = spectrum(k=k, symbols=4, metric="euclidean")(T, T).numpy()
    assert np.all(e[1:4, 1:4] == 0) and e[1, 0] == 2.0 and e[3, 4] == 2.0 and e[0, 3] == 2.0
    assert np.array_equal(e.view(np.int32), euclid_of(d2_of(P, P)).view(np.int32))
