"""
GPU checks of the VALUES of the Minkowski kernels (pg_pack_f16, pg_minkowski_dense and, through mk_accumulate /
mk_finish, the fused pg_minkowski_knn / pg_minkowski_eps_*) against the interval model of tests/minkowski_model.py:
every value is one of its pair's two allowed fp16 values, which for a decided pair - most of them, and all of the
`lattice` and `tiny` ones - is bit equality.  The model assumes nothing about the kernel's accumulation order, so
no tolerance here is measured.  The dimensions cover one partial chunk (1, 2, 7), whole chunks (8, 16, 128), a
partial chunk after whole ones (9, 15, 17, 127), both sides of the staged switch of the fused kernels (128 | 129),
a partial chunk after a whole LDS segment (129, 135), a partial last segment (136, 255, 257, 1000, 2049) and
whole segments (1280); the scales cover fp16-subnormal squares (`tiny`), sums on the 65504 | inf boundary and an
overflowing difference (`edge`).  tests/test_minkowski_model_cpu.py pins the model and the data themselves.
"""
import ctypes

import numpy as np
import pytest
import torch

import minkowski_model as mm

pytestmark = pytest.mark.gpu

M, N = 33, 300                 # 16 + 16 + 1 query rows, 256 + 44 columns
DIMS = (1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 255, 257, 1000, 1280, 2049)
CMPS = ("CMP_LE", "CMP_LT", "CMP_EQ", "CMP_GE", "CMP_GT")
NP_CMP = {"CMP_LE": np.less_equal, "CMP_LT": np.less, "CMP_EQ": np.equal, "CMP_GE": np.greater_equal, "CMP_GT": np.greater}


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


def _dev(nat, a):
    return torch.from_numpy(np.array(a)).to(nat.device())


def _packed(nat, x, y):
    return nat.pack_f16(_dev(nat, x)), nat.pack_f16(_dev(nat, y))


def _check_block(got, model, what):
    """got: (m, n) fp16 device tensor; model: (a, b, decided) of the same pairs."""
    a, b, decided = model
    assert got.dtype == torch.float16 and tuple(got.shape) == a.shape, what
    g = got.cpu().numpy()
    ok = mm.inside(g, a, b)
    bad = np.argwhere(~ok)
    assert ok.all(), (what, len(bad), [(int(i), int(j), float(g[i, j]), float(a[i, j]), float(b[i, j])) for i, j in bad[:5]])
    assert np.array_equal(mm.bits(g)[decided], mm.bits(a)[decided]), what


@pytest.mark.parametrize("kind", mm.KINDS)
@pytest.mark.parametrize("d", DIMS)
def test_dense_against_the_model(nat, d, kind):
    x, y, models, _ = mm.case(kind, N, M, d)
    xp, yp = _packed(nat, x, y)
    dup = np.arange(mm.DUPLICATES)
    over = np.isinf(models[False][0]) & np.isinf(models[False][1])
    assert over.any() == (kind == "edge")
    if kind in ("lattice", "tiny"):
        assert models[False][2].all() and models[True][2].all()
    elif d <= 1280:
        assert min(models[False][2].mean(), models[True][2].mean()) >= 0.85
    for sim in (False, True):
        got = nat.minkowski_dense(xp, yp, similarity=sim)
        _check_block(got, models[sim], (kind, d, sim))
        g = got.cpu().numpy()
        assert (mm.bits(g[dup, dup]) == (0x3C00 if sim else 0)).all(), (kind, d, sim)        # duplicates: 0, or 1
        assert (mm.bits(g[over]) == (0 if sim else 0x7C00)).all(), (kind, d, sim)            # overflow: inf, or 0


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
@pytest.mark.parametrize("m", [1, 15, 16, 17, 33])
def test_shapes_against_the_model(nat, m, n):
    x, y, models, _ = mm.case("lattice", n, m, 13)
    xp, yp = _packed(nat, x, y)
    for sim in (False, True):
        assert models[sim][2].all()
        _check_block(nat.minkowski_dense(xp, yp, similarity=sim), models[sim], (m, n, sim))


def test_swapped_operands(nat):
    """(y - x)^2 = (x - y)^2 in fp16: the block of the swapped operands is the transposed model."""
    x, y, models, _ = mm.case("lattice", 513, 33, 13)
    xp, yp = _packed(nat, x, y)
    for sim in (False, True):
        _check_block(nat.minkowski_dense(yp, xp, similarity=sim), tuple(np.ascontiguousarray(t.T) for t in models[sim]),
                     ("swapped", sim))


@pytest.mark.parametrize("sim", [False, True])
@pytest.mark.parametrize("kind", ["normal", "tiny"])
def test_operator_on_the_device_against_the_cpu(nat, kind, sim):
    from prograph_amd.distance import minkowski
    x, y, models, _ = mm.case(kind, N, M, 129)
    a, b, decided = models[sim]
    cpu = minkowski(torch.from_numpy(x.copy()), torch.from_numpy(y.copy()), similarity=sim)
    got = minkowski(_dev(nat, x), _dev(nat, y), similarity=sim)
    assert got.is_cuda and got.dtype == cpu.dtype == torch.float16 and got.shape == cpu.shape
    _check_block(got, models[sim], (kind, sim))
    assert mm.inside(cpu.numpy(), a, b).all()
    assert np.array_equal(mm.bits(got.cpu().numpy())[decided], mm.bits(cpu.numpy())[decided])
    assert decided.mean() >= 0.98


def _model_order(v, sim):
    """The (value, column) order of every row: ascending distances, descending similarities, ties by column."""
    key = mm.bits(v)                                     # non-negative fp16: the bits order like the values
    return np.argsort(0xFFFF - key if sim else key, axis=1, kind="stable")


@pytest.mark.parametrize("sim", [False, True])
@pytest.mark.parametrize("d", [9, 129, 1000])
def test_graphs_against_the_model_order(nat, d, sim):
    """Lattice data: every value is decided and the rows tie heavily, so the fused kNN lists and eps CSRs must equal
    a plain numpy selection over the MODEL's values - indices, and weights by bits."""
    x, y, models, _ = mm.case("lattice", N, M, d)
    v, _, decided = models[sim]
    assert decided.all()
    xp, yp = _packed(nat, x, y)
    order = _model_order(v, sim)
    ranked = np.take_along_axis(v, order, axis=1)
    assert (ranked[:, 1:] == ranked[:, :-1]).sum(1).min() >= 50              # every row ties, many times
    for k in (1, 16, 63, 100):
        for first in (0, 1):
            idx, w = nat.minkowski_knn(xp, yp, k, first=first, similarity=sim)
            assert idx.dtype == torch.int32 and w.dtype == torch.float16 and tuple(idx.shape) == tuple(w.shape) == (M, k)
            assert np.array_equal(idx.cpu().numpy(), order[:, first:first + k]), (d, sim, k, first)
            assert np.array_equal(mm.bits(w.cpu().numpy()), mm.bits(ranked[:, first:first + k])), (d, sim, k, first)
            if k > 1:                                                        # some row ties across the end of its list
                assert (ranked[:, first + k - 1] == ranked[:, first + k]).any(), (d, sim, k, first)
    eps = np.sort(v.reshape(-1))[v.size // 2]                      # a value many pairs take
    assert 0 < float(eps) < np.inf and (v == eps).sum() >= M
    v32 = v.astype(np.float32)
    for c in CMPS:
        hit = (NP_CMP[c](np.float32(eps), v32) & (v32 < 1)) if sim else (NP_CMP[c](v32, np.float32(eps)) & (v32 > 0))
        assert hit.any() and not hit.all()
        ip, ix, w = nat.minkowski_eps(xp, yp, getattr(nat, c), float(eps), similarity=sim)
        assert ip.dtype == torch.int64 and ix.dtype == torch.int32 and w.dtype == torch.float16
        assert np.array_equal(ip.cpu().numpy(), np.concatenate([[0], np.cumsum(hit.sum(1))])), (d, sim, c)
        assert np.array_equal(ix.cpu().numpy(), np.nonzero(hit)[1]), (d, sim, c)
        assert np.array_equal(mm.bits(w.cpu().numpy()), mm.bits(v[hit])), (d, sim, c)


def _bits(t):
    return t.cpu().numpy().view(np.int16)


@pytest.mark.parametrize("kind", ["tiny", "edge"])
@pytest.mark.parametrize("d", [1, 7, 127, 129, 136, 1000])
def test_fused_equals_staged(nat, d, kind):
    """The claim of test_minkowski_fused_gpu.py at the new dimensions and scales: rows of inf ties and of zeros."""
    x, y, models, _ = mm.case(kind, N, M, d)
    xp, yp = _packed(nat, x, y)
    for sim in (False, True):
        block = nat.minkowski_dense(xp, yp, similarity=sim)
        _check_block(block, models[sim], (kind, d, sim))
        for k in (1, 16, 63, 100):
            for first in (0, 1):
                fi, fw = nat.minkowski_knn(xp, yp, k, first=first, similarity=sim)
                si, sw = nat.f16_knn(block, k, first=first, descending=sim)
                assert torch.equal(fi, si), (kind, d, sim, k, first)
                assert np.array_equal(_bits(fw), _bits(sw)), (kind, d, sim, k, first)
        vals = block.float().cpu().numpy().reshape(-1)
        thresholds = [float(np.median(vals[np.isfinite(vals) & (vals > 0)]))]
        if kind == "edge" and not sim:
            thresholds.append(float(np.inf))
        for eps in thresholds:
            for c in CMPS:
                got = nat.minkowski_eps(xp, yp, getattr(nat, c), eps, similarity=sim)
                want = nat.f16_eps(block, getattr(nat, c), eps, similarity=sim)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (kind, d, sim, c, eps)
                assert np.array_equal(_bits(got[2]), _bits(want[2])), (kind, d, sim, c, eps)


@pytest.mark.parametrize("d", [7, 13, 136])
def test_pack_with_a_row_list_and_a_leading_dimension(nat, d):
    """pg_pack_f16 through ctypes: rows gathered by a list (a permutation with a repeat) from a source whose rows
    lie ld > d elements apart.  The buffer - pre-filled with ones - equals nat.pack_f16 of the gathered contiguous
    rows and a numpy layout of it byte for byte: chunk q of vector s at (q * npad + s) * 16, zeros in the rows
    n .. npad and behind element d of the last chunk."""
    rng = np.random.default_rng(d)
    r, ld = 290, d + 5
    src = rng.standard_normal((r, ld)).astype(np.float16)
    src[src == 0] = np.float16(1)                                   # no zero in the source: a zero is a fill
    rows = np.concatenate([rng.permutation(r), [3, 3, r - 1]]).astype(np.int64)
    n, npad, nq = len(rows), nat.npad(len(rows)), (d + 7) // 8
    assert n % 256 and npad == 512 and int(nat.lib().pg_f16_nchunks(d)) == nq
    dsrc, drows = _dev(nat, src), _dev(nat, rows)
    buf = torch.full((nq * npad * 16,), 0xFF, dtype=torch.uint8, device=nat.device())
    rc = nat.lib().pg_pack_f16(ctypes.c_void_p(dsrc.data_ptr()), n, d, ld, ctypes.c_void_p(drows.data_ptr()),
                               ctypes.c_void_p(buf.data_ptr()), npad, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    want = np.zeros((nq, npad, 8), np.float16)
    padded = np.zeros((n, nq * 8), np.float16)
    padded[:, :d] = src[rows, :d]
    want[:, :n, :] = padded.reshape(n, nq, 8).transpose(1, 0, 2)
    got = buf.cpu().numpy()
    assert np.array_equal(got, want.view(np.uint8).reshape(-1))
    ref = nat.pack_f16(_dev(nat, src[rows, :d]))
    assert (ref.n, ref.d, ref.npad) == (n, d, npad) and np.array_equal(got, ref.buf.cpu().numpy())
