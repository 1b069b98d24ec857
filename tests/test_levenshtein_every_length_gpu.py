"""
The Levenshtein kernel beyond 128 positions (pg_lev_long.hip) at every text and pattern length, on the sets of
tests/lev_every_testdata.py: every length 0..257 against every length 0..257 at each of the five instantiated block
counts, a long lane in every wave (nbw = NB beside short lanes), every chunk count 3..16 with every segment count and
tail of the last chunk, the output frame, the pack kernel's lengths, layout and validity word, and the operator's choice
by that word.  Every comparison is an every-entry equality of integers with the C oracle's plain Wagner-Fischer
(pinned, with what the sets cover, in tests/test_levenshtein_every_length_cpu.py).
"""
import ctypes
import sys

import numpy as np
import pytest
import torch

import lev_every_testdata as EV
import lev_testdata as LT
from oracle import c_oracle as C
from oracle import prograph_oracle as O
from prograph_amd.distance import levenshtein

pytestmark = [pytest.mark.gpu, pytest.mark.one_engine]

ROWS = 16                                          # PG_LEVD_ROWS: text rows per workgroup


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


_operands = {}


def operand(nat, name, width):
    """(operand, lengths, rows) of the rows of set E / T / P / EP that fit `width`, packed at that width; once per module."""
    if (name, width) not in _operands:
        T = {"E": EV.set_e, "T": EV.set_t, "P": EV.set_p, "EP": EV.set_ep}[name]()
        tok, rows = EV.at_width(T, width)
        op = nat.lev_long_operand(torch.from_numpy(tok))
        assert op.valid() and (op.n, op.l) == (len(rows), width)
        _operands[(name, width)] = op, LT.lengths(tok), rows
    return _operands[(name, width)]


def same(got, want, text_lens, pattern_lens, what=""):
    """Every entry equal as integers; the message names the first differing (text length, pattern length, got, want)."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    got = got.astype(np.int64)
    bad = np.argwhere(got != want)
    if len(bad):
        r, c = bad[0]
        pytest.fail(f"{what}: {len(bad)} of {want.size} entries differ, the first at text length {int(text_lens[r])}, pattern "
                    f"length {int(pattern_lens[c])}: got {int(got[r, c])}, want {int(want[r, c])}")


def dense(nat, xo, yo, out_bytes, rows=None):
    got = nat.levenshtein_long_dense(xo, yo, out_bytes=out_bytes, rows=rows)
    assert got.dtype == (torch.float16 if out_bytes == 2 else torch.int64) and got.is_cuda
    return got


# ---------------------------------------------------------------- 1. every length x every length x every instance
@pytest.mark.parametrize("width", [128, 256, 257, 1024, 2048])
def test_every_text_length_against_every_pattern_length(nat, width):
    """The patterns: the rows of E that fit, at width 128 (NB = 1), 256 (2), 257 (4), 1024 (8), 2048 (16) - in the wide
    operands the blocks above a wave's longest pattern are skipped.  The texts: E at width 257, and E at width 2048
    against the widest patterns.  Both output types, and two row ranges that begin and end inside a group of 16 rows."""
    assert EV.instance(width) == {128: 1, 256: 2, 257: 4, 1024: 8, 2048: 16}[width]
    xo, lx, cols = operand(nat, "E", width)
    D = EV.d_ee()
    for yw in (257, 2048) if width == 2048 else (257,):
        yo, ly, rows = operand(nat, "E", yw)
        assert len(rows) == 258
        want = D[np.ix_(rows, cols)]
        for out_bytes in (8, 2):
            same(dense(nat, xo, yo, out_bytes), want, ly, lx, f"width {width}, texts at {yw}, {out_bytes} bytes")
        for (r0, r1), out_bytes in (((5, 38), 2), ((83, 251), 8)):
            assert r0 % ROWS and r1 % ROWS
            same(dense(nat, xo, yo, out_bytes, rows=(r0, r1)), want[r0:r1], ly[r0:r1], lx, f"width {width}, rows {r0}..{r1}")


# ---------------------------------------------------------------- 2. a long lane in every wave
@pytest.mark.parametrize("nb", [4, 8, 16])
def test_long_lane_in_every_wave(nat, nb):
    """E with rows of P among them, one pattern of exactly NB blocks in every wave of 64 columns: nbw = NB, and the short
    lanes of the wave run through blocks of padding rows beside it."""
    cols = EV.long_lane_columns(nb)
    lens = np.array(EV.lens_ep())[cols]
    for w in range(0, len(cols), 64):
        assert max(EV.blocks(l) for l in lens[w:w + 64]) == nb and lens[w:w + 64].min() < 64
    tok = np.ascontiguousarray(EV.set_ep()[cols][:, :128 * nb])
    assert np.array_equal(LT.lengths(tok), lens)
    xo = nat.lev_long_operand(torch.from_numpy(tok))
    assert xo.valid() and EV.instance(xo.l) == nb
    yo, ly, _ = operand(nat, "E", 257)
    want = EV.d_e_ep()[:, cols]
    same(dense(nat, xo, yo, 8), want, ly, lens, f"NB {nb}")
    same(dense(nat, xo, yo, 2, rows=(3, 250)), want[3:250], ly[3:250], lens, f"NB {nb}, fp16")


# ---------------------------------------------------------------- 3. every chunk count and tail
def test_every_chunk_count_and_tail_against_wide_patterns(nat):
    """Texts T (3..16 chunks, 1..4 segments in the last, every tail 1..32) against E followed by P at width 2048."""
    xo, lx, cols = operand(nat, "EP", 2048)
    yo, ly, rows = operand(nat, "T", 2048)
    assert len(cols) == 288 and len(rows) == 58
    D = EV.d_t_ep()
    same(dense(nat, xo, yo, 8), D, ly, lx, "T x EP")
    same(dense(nat, xo, yo, 2, rows=(7, 55)), D[7:55], ly[7:55], lx, "T x EP, fp16")


@pytest.mark.parametrize("width", [257, 128])
def test_every_chunk_count_and_tail_at_small_instances(nat, width):
    """The same texts against E alone at width 257 (NB = 4) and 128 (NB = 1): up to 16 chunks of text over few blocks."""
    xo, lx, cols = operand(nat, "E", width)
    yo, ly, _ = operand(nat, "T", 2048)
    want = EV.d_t_ep()[:, cols]
    same(dense(nat, xo, yo, 8), want, ly, lx, f"T x E at {width}")
    same(dense(nat, xo, yo, 2), want, ly, lx, f"T x E at {width}, fp16")


def test_long_rows_as_patterns_of_every_short_text(nat):
    """The transposed call: T as patterns (every block count 3..16, the last row anywhere), E as texts."""
    xo, lx, _ = operand(nat, "T", 2048)
    yo, ly, _ = operand(nat, "E", 257)
    want = np.ascontiguousarray(EV.d_t_ep()[:, :258].T)
    same(dense(nat, xo, yo, 8), want, ly, lx, "E x T")
    same(dense(nat, xo, yo, 2, rows=(1, 255)), want[1:255], ly[1:255], lx, "E x T, fp16")


# ---------------------------------------------------------------- 4. the output frame
@pytest.mark.parametrize("out_bytes", [8, 2])
def test_output_frame(nat, out_bytes):
    """The C entry with ldo = n + 3 into a sentinel-filled buffer of one row more than is written: the written entries are
    the reference, every other element is still the sentinel."""
    xo, lx, _ = operand(nat, "E", 257)
    yo, ly, _ = operand(nat, "E", 257)
    r0, r1 = 3, 254                                                  # the rows are taken from inside the operand, too
    n, m, ldo = xo.n, r1 - r0, xo.n + 3
    assert n % 256 and m % ROWS
    out = torch.full((m + 1, ldo), -7, dtype=torch.float16 if out_bytes == 2 else torch.int64, device=nat.device())
    rc = nat.lib().pg_levenshtein_long_dense(ctypes.c_void_p(xo.buf.data_ptr()), n, xo.npad, ctypes.c_void_p(xo.lens.data_ptr()),
                                             xo.l, ctypes.c_void_p(yo.buf.data_ptr() + 16 * r0), m, yo.npad,
                                             ctypes.c_void_p(yo.lens.data_ptr() + 4 * r0), yo.l, ctypes.c_void_p(out.data_ptr()),
                                             out_bytes, ldo, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    got = out.cpu().numpy().astype(np.int64)
    same(got[:m, :n], EV.d_ee()[r0:r1], ly[r0:r1], lx, "the frame's inside")
    assert (got[:m, n:] == -7).all() and (got[m] == -7).all()


# ---------------------------------------------------------------- 5. the pack kernel
def test_pack_lengths(nat):
    for name, own in (("E", 257), ("T", 2048), ("P", 2048), ("EP", 2048)):
        for width in {own, 2048}:
            op, lens, rows = operand(nat, name, width)
            got = op.lens.cpu().numpy()
            assert got.dtype == np.int32 and np.array_equal(got, lens), (name, width)
    assert np.array_equal(operand(nat, "E", 257)[1], EV.lens_e()) and np.array_equal(operand(nat, "P", 2048)[1], EV.lens_p())
    assert np.array_equal(operand(nat, "T", 2048)[1], EV.lens_t())


def packed_layout(tok, npad):
    """The documented layout in numpy: uint4 number (b * 5 + q) * npad + s holds bit q of the tokens 128 b .. 128 b + 127 of
    row s, token 128 b + i at bit i of the 128 (little endian); rows n .. npad and positions past the width are zero."""
    n, l = tok.shape
    nb = -(-l // 128)
    padded = np.zeros((npad, nb * 128), dtype=np.uint8)
    padded[:n, :l] = tok
    bits = (padded[None, :, :] >> np.arange(5, dtype=np.uint8)[:, None, None]) & 1          # (q, s, position)
    bits = bits.reshape(5, npad, nb, 128).transpose(2, 0, 1, 3)                              # (b, q, s, 128)
    return np.packbits(bits, axis=-1, bitorder="little").reshape(-1)                         # 16 bytes per (b, q, s)


def test_packed_layout_byte_for_byte(nat):
    tok = np.array(EV.set_e())                                       # a writable copy for torch.from_numpy
    n, l, npad = len(tok), tok.shape[1], nat.npad(len(tok))
    assert (n, l, npad) == (258, 257, 512)
    dtok = torch.from_numpy(tok).to(nat.device())
    buf = torch.full((3 * 5 * npad * 16,), 0xFF, dtype=torch.uint8, device=nat.device())
    lens = torch.full((n,), -1, dtype=torch.int32, device=nat.device())
    flags = torch.full((1,), -1, dtype=torch.int32, device=nat.device())
    rc = nat.lib().pg_lev_long_pack(ctypes.c_void_p(dtok.data_ptr()), n, l, l, ctypes.c_void_p(buf.data_ptr()), npad,
                                    ctypes.c_void_p(lens.data_ptr()), ctypes.c_void_p(flags.data_ptr()),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    want = packed_layout(tok, npad)
    got = buf.cpu().numpy()
    assert want.shape == got.shape
    bad = np.nonzero(got != want)[0]
    assert not len(bad), f"{len(bad)} bytes differ, the first at {bad[0]}: uint4 {bad[0] // 16} = (block * 5 + plane) * {npad} + row"
    assert int(flags.item()) == 0 and np.array_equal(lens.cpu().numpy(), EV.lens_e())
    assert np.array_equal(operand(nat, "E", 257)[0].buf.cpu().numpy(), want)                 # the wrapper's buffer is that one


DEFECT_AT = (0, 31, 32, 127, 128, 129, 255, 256, 1023, 1024, 2046)
DEFECTS = [("zero", p, 0) for p in DEFECT_AT] + [(f"token {t}", p, t) for t in (32, 255) for p in DEFECT_AT + (2047,)]


def test_validity_word(nat):
    """Full rows are valid at widths 129, 257 and 2048.  One defective row among 70 valid ones - one interior zero, or one
    token above 31, at one position - makes the operand invalid, wherever the row stands."""
    rng = np.random.default_rng(77)
    full = rng.integers(1, 32, (71, 2048)).astype(np.uint8)
    for width in (129, 257, 2048):
        assert nat.lev_long_operand(torch.from_numpy(np.ascontiguousarray(full[:, :width]))).valid(), width
    dev = torch.from_numpy(full).to(nat.device())
    missed = []
    for width in (257, 2048):
        for what, pos, token in DEFECTS:
            if pos >= width - (token == 0):                          # a zero needs a token behind it to be interior
                continue
            for row in (0, 64, 70):
                T = dev[:, :width].clone()
                T[row, pos] = token
                op = nat.lev_long_operand(T)
                if op.valid():
                    missed.append((width, what, pos, row))
    assert not missed, f"taken for valid (width, defect, position, row): {missed}"


# ---------------------------------------------------------------- 6. the operator decides by that word
def test_operator_decides_by_the_validity_word(nat, monkeypatch):
    mod = sys.modules["prograph_amd.distance.levenshtein"]
    rng = np.random.default_rng(78)
    lens = (300, 131, 250, 0, 299, 140, 1, 300)
    X = np.zeros((len(lens), 300), dtype=np.uint8)
    for r, l in zip(X, lens):
        r[:l] = rng.integers(1, 32, l)
    X[5, :140] = X[4, :140]                                          # related rows: small distances among the large
    X[7, :300] = X[0, :300]
    X[7, 129:132] = (1 + X[7, 129:132].astype(np.int64) % 31)
    Z = X.copy()
    Z[4, 130] = 0                                                    # the one interior zero
    assert Z.max() <= 31 and np.array_equal(LT.lengths(Z), lens) and (Z[4, :299] == 0).sum() == 1
    ys = [0, 4, 5]

    def run(T):
        dT = torch.from_numpy(T).cuda()
        d = levenshtein(dT, dT[ys])
        assert d.is_cuda and d.dtype == torch.int64
        return d.cpu().numpy()

    want_valid = C.lev_matrix(X, X[ys])
    want_zero = np.array([[O.levenshtein_full(Z[y].tolist(), lens[y], Z[x].tolist(), lens[x]) for x in range(len(lens))] for y in ys])
    assert want_zero[1, 4] == 0 and (want_zero != want_valid).any()   # the zero is a symbol: other distances
    same(run(X), want_valid, np.array(lens)[ys], lens, "valid operands")
    same(run(Z), want_zero, np.array(lens)[ys], lens, "one interior zero at position 130")
    monkeypatch.setattr(mod, "_torch_levenshtein", None)             # the kernel or nothing
    same(run(X), want_valid, np.array(lens)[ys], lens, "valid operands, no torch expression")
    with pytest.raises(TypeError):                                   # the invalid call does not return the kernel's numbers
        run(Z)
