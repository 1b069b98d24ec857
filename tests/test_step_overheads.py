"""
The fixed per-call work around the kNN sweep: the pack kernel against a host mirror of the plane
buffer, the gate words the probe's decision launch leaves - and the counter block it zeroes - against a host
re-computation, and the kNN passes whose issue-priority steps sit at the edges of a sweep against the oracle's order.
Bit-exact: integer work throughout.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from prograph_amd import _native
    _native.lib()
    _native.device()
    return _native


# ---------------------------------------------------------------------------------------------------------------------
# pack: host mirror of the plane buffer (include/prograph_hip.h "Token storage"; signature and fold sections: pg_api.hip)
# ---------------------------------------------------------------------------------------------------------------------
def _nib8(x):
    """8 bits -> 8 nibbles, bit i in bit 0 of nibble i (pg_common.h: pg_nib8)"""
    x = x.astype(np.uint64) & np.uint64(0xFF)
    out = np.zeros_like(x)
    for i in range(8):
        out |= ((x >> np.uint64(i)) & np.uint64(1)) << np.uint64(4 * i)
    return out


def mirror_planes(tok, bits):
    """The bytes pg_pack_planes writes for the (n, l) token matrix `tok` (values taken modulo 2^bits, as the kernel does
    for tokens it flags)."""
    tok = np.asarray(tok).astype(np.int64)
    n, l = tok.shape
    ng = (l + 31) // 32
    nq = (ng * bits + 3) // 4
    npad = ((max(n, 1) + 255) // 256) * 256
    t = np.zeros((npad, ng * 32), dtype=np.int64)
    t[:n, :l] = tok
    j = np.arange(32, dtype=np.uint64)
    words = np.zeros((npad, bits * ng), dtype=np.uint64)           # plane-major record order: word p * ng + g
    for p in range(bits):
        for g in range(ng):
            b = ((t[:, g * 32:(g + 1) * 32] >> p) & 1).astype(np.uint64)
            words[:, p * ng + g] = (b << j).sum(axis=1)
    chunks = np.zeros((nq, npad, 4), dtype=np.uint32)
    for w in range(bits * ng):
        chunks[w >> 2, :, w & 3] = words[:, w].astype(np.uint32)
    even = np.zeros(npad, dtype=np.uint64)
    odd = np.zeros(npad, dtype=np.uint64)
    for g in range(ng):
        if g & 1:
            odd ^= words[:, g]
        else:
            even ^= words[:, g]
    s64 = even | (odd << np.uint64(32))
    sig = (s64 & np.uint64((1 << 54) - 1)) ^ (s64 >> np.uint64(54))
    lo = sig & np.uint64(0xFFFFFFFF)
    hi = sig >> np.uint64(32)
    hi[:n] |= np.uint64(0xFFC00000)                                 # the ten bias slots of real sequences
    sigsec = np.zeros((npad // 32, 64, 4), dtype=np.uint32)
    s = np.arange(npad)
    for i in range(4):
        sigsec[s >> 5, s & 31, i] = (_nib8(lo >> np.uint64(8 * i)) << np.uint64(1)).astype(np.uint32)
        sigsec[s >> 5, 32 + (s & 31), i] = (_nib8(hi >> np.uint64(8 * i)) << np.uint64(1)).astype(np.uint32)
    fold = np.zeros((2, npad, 4), dtype=np.uint32)
    for p in range(bits):
        f = np.zeros(npad, dtype=np.uint64)
        for g in range(ng):
            f ^= words[:, p * ng + g]
        fold[p >> 2, :, p & 3] = f.astype(np.uint32)
    return np.concatenate([chunks.reshape(-1), sigsec.reshape(-1), fold.reshape(-1)]).view(np.uint8)


def _pack_raw(nat, src, n, l, ld, bits, rows=None):
    """pg_pack_planes on the device tensor `src` (any row stride `ld`, in elements); returns (buffer bytes, flag word)."""
    dev = src.device
    buf = torch.full((nat.planes_bytes(n, l, bits),), 0xA5, dtype=torch.uint8, device=dev)
    flags = torch.full((1,), 7, dtype=torch.int32, device=dev)
    ridx = None if rows is None else torch.as_tensor(np.asarray(rows), dtype=torch.int64).to(dev)
    rc = nat.lib().pg_pack_planes(nat._ptr(src), src.element_size(), n, l, ld, nat._ptr(ridx), bits, nat._ptr(buf), nat.npad(n),
                                  nat._ptr(flags), nat._stream())
    assert rc == 0, nat.lib().pg_last_error()
    return buf.cpu().numpy(), int(flags.item())


_DT = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}


def test_pack_equals_host_mirror(nat):
    """Every section of the plane buffer, byte for byte: sequence counts around the workgroup (64) and padding (256)
    sizes, widths around a group of 32 tokens, both plane counts, every element size."""
    rng = np.random.RandomState(11)
    for n in (1, 31, 255, 256, 257, 1000):
        for l in (1, 31, 32, 33, 64):
            for bits in (5, 8):
                tok = rng.randint(0, 1 << bits, size=(n, l))
                want = mirror_planes(tok, bits)
                for es in (1, 2, 4, 8):
                    src = torch.from_numpy(tok.astype(_DT[es])).cuda()
                    got, flag = _pack_raw(nat, src, n, l, l, bits)
                    assert flag == 0, (n, l, bits, es)
                    assert np.array_equal(got, want), (n, l, bits, es)


def test_pack_row_list_odd_stride_and_bytes(nat):
    """A row list, row strides above the width - odd ones, where no row after the first is aligned - and pg_pack_bytes with
    its token output."""
    rng = np.random.RandomState(12)
    for n_src, l, bits in [(700, 64, 5), (300, 33, 8), (257, 96, 5)]:
        tok = rng.randint(0, 1 << bits, size=(n_src, l))
        rows = rng.randint(0, n_src, size=n_src + 37)
        for es in (1, 2, 4, 8):
            src = torch.from_numpy(tok.astype(_DT[es])).cuda()
            got, flag = _pack_raw(nat, src, len(rows), l, l, bits, rows=rows)
            assert flag == 0 and np.array_equal(got, mirror_planes(tok[rows], bits)), (n_src, l, bits, es)
            for ld in ((l + 3) | 1, (l + 17) | 1, l + 16):           # odd strides (position by position); rows 16 bytes apart
                wide = rng.randint(0, 1 << bits, size=(n_src, ld)).astype(_DT[es])
                wide[:, :l] = tok
                got, flag = _pack_raw(nat, torch.from_numpy(wide).cuda(), n_src, l, ld, bits)
                assert flag == 0 and np.array_equal(got, mirror_planes(tok, bits)), (n_src, l, bits, es, ld)
                got, flag = _pack_raw(nat, torch.from_numpy(wide).cuda(), len(rows), l, ld, bits, rows=rows)
                assert flag == 0 and np.array_equal(got, mirror_planes(tok[rows], bits)), (n_src, l, bits, es, ld)
    # pg_pack_bytes: token = table[byte], written row-major as well
    table = rng.randint(0, 32, size=256).astype(np.uint8)
    for n, width, bits in [(1, 1, 5), (257, 33, 5), (1000, 64, 5), (300, 31, 8)]:
        raw = rng.randint(0, 256, size=(n, width)).astype(np.uint8)
        planes, tokens = nat.pack_bytes(raw, table, bits=bits)
        assert np.array_equal(tokens.cpu().numpy(), table[raw])
        assert np.array_equal(planes.buf.cpu().numpy(), mirror_planes(table[raw], bits)), (n, width, bits)


def test_pack_flags_a_token_outside_the_alphabet(nat):
    """One bad token anywhere sets the validity word - in the 16-byte-load path, in the tail group, in the scalar path, for
    negative values - and the buffer still holds the tokens' low bits."""
    rng = np.random.RandomState(13)
    for es, bad in [(1, 32), (2, 32), (2, -1), (4, 1 << 20), (8, -5), (8, 1 << 40), (2, 256)]:
        for l, ld in [(64, 64), (40, 40), (64, 67)]:
            tok = rng.randint(0, 32, size=(300, l)).astype(np.int64)
            for pos in [(0, 0), (299, l - 1), (130, 33)]:
                t = tok.copy()
                t[pos] = bad
                wide = np.zeros((300, ld), dtype=_DT[es])
                wide[:, :l] = t.astype(_DT[es])
                got, flag = _pack_raw(nat, torch.from_numpy(wide).cuda(), 300, l, ld, 5)
                assert flag != 0, (es, bad, l, ld, pos)
                assert np.array_equal(got, mirror_planes(t & 31, 5)), (es, bad, l, ld, pos)
    # 8 planes: 255 is a token, 256 is not
    t = rng.randint(0, 256, size=(70, 64)).astype(np.int16)
    assert _pack_raw(nat, torch.from_numpy(t).cuda(), 70, 64, 64, 8)[1] == 0
    t[69, 63] = 256
    assert _pack_raw(nat, torch.from_numpy(t).cuda(), 70, 64, 64, 8)[1] != 0
    with pytest.raises(ValueError):
        nat.pack(torch.from_numpy(np.array([[1, 2, 40]], dtype=np.int64)), bits=5)


# ---------------------------------------------------------------------------------------------------------------------
# gate: the probe's decision, and the counter block it zeroes, against a host re-computation from the tokens
# ---------------------------------------------------------------------------------------------------------------------
PROBE_N = 65536          # PG_PROBE_MIN_N: the smallest launch that is probed
PROBE_ROWS, PROBE_WAVES, PROBE_STRIDE = 64, 128, 8
WS_GATES, WS_COUNTS = 576, 640


def host_probe(tok, near, lo, span, need):
    """Per sample row the columns nearer than `near` and inside [lo, lo + span] among the tiles the probe looks at, and the
    two gate words decided from them (pg_api.hip: "Data probe + decision")."""
    n = len(tok)
    near_s = np.zeros(PROBE_ROWS, dtype=np.int64)
    eps_s = np.zeros(PROBE_ROWS, dtype=np.int64)
    ntile = (n + 63) // 64
    for s in range(PROBE_ROWS):
        row = (n * (2 * s + 1)) // (2 * PROBE_ROWS)
        tiles = np.arange(s % PROBE_STRIDE, ntile, PROBE_STRIDE)
        cols = (tiles[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)
        cols = cols[cols < n]
        d = (tok[cols] != tok[row]).sum(axis=1)
        near_s[s] = int((d < near).sum())
        eps_s[s] = int(((d >= lo) & (d <= lo + span)).sum())
    clustered = int((near_s * PROBE_STRIDE >= need).sum())
    pairs = PROBE_ROWS * n
    one = 2 * int(near_s.sum()) * PROBE_STRIDE > pairs
    g0 = (2 if one else 0) if 2 * clustered >= PROBE_ROWS else 1
    g1 = 1 if int(eps_s.sum()) * PROBE_STRIDE * 25 > pairs else 0
    return near_s, eps_s, (g0, g1)


@pytest.fixture(scope="module")
def probe_inputs(nat):
    """name -> (planes, what the host says about a kNN launch with k = 12, about an eps <= 2 launch)"""
    from prograph_amd import synth
    data = {
        # (655 clusters: with a power of two a row's cluster mates all fall into one of the probe's eight tile classes)
        "clustered": synth.clustered_tokens(PROBE_N, 64, seed=21, members=100),
        "unclustered": np.random.RandomState(8).randint(1, 21, size=(PROBE_N, 64)).astype(np.uint8),
        "one_cluster": synth.clustered_tokens(PROBE_N, 64, seed=5, members=PROBE_N),
    }
    out = {}
    for name, tok in data.items():
        planes = nat.pack(torch.from_numpy(tok), bits=5)
        knn = host_probe(tok, near=10, lo=1, span=0, need=1 + 12)      # the MFMA engine's cap at L > 32; eps interval [1, 1]
        eps = host_probe(tok, near=0, lo=1, span=1, need=1)            # no cap; d in [1, 2]
        out[name] = (planes, knn, eps)
    return out


@pytest.fixture
def spy_workspace(nat, monkeypatch):
    """Every workspace of a call comes poisoned and is kept: nothing in it may be taken for zero."""
    for v in ("PG_ENGINE", "PG_ENGINE_MIN_ROWS", "PG_PROBE", "PG_PROBE_S", "PG_PROBE_W", "PG_KNN_GUESS", "PG_GATE_FORCE", "PG_MM_R"):
        monkeypatch.delenv(v, raising=False)
    seen = []

    def poisoned(nrows, dev):
        ws = torch.full((int(nat.lib().pg_workspace_bytes(int(nrows))),), 0xEE, dtype=torch.uint8, device=dev)
        seen.append(ws)
        return ws
    monkeypatch.setattr(nat, "workspace", poisoned)
    return seen


def _gate_words(ws):
    torch.cuda.synchronize()
    head = ws[:WS_COUNTS + 8 * PROBE_ROWS * PROBE_WAVES].cpu().numpy()
    counts = head[WS_COUNTS:].view(np.uint32).reshape(PROBE_ROWS, PROBE_WAVES, 2).astype(np.int64).sum(axis=1)
    gates = head[WS_GATES:WS_GATES + 8].view(np.uint32)
    reserved = head[64:WS_GATES]                                       # the reserved part of the counter block: zeroed with it
    return counts, (int(gates[0]), int(gates[1])), reserved


@pytest.mark.parametrize("name", ["clustered", "unclustered", "one_cluster"])
def test_gate_equals_host_decision(nat, probe_inputs, spy_workspace, name):
    planes, (k_near, k_eps, k_gates), (e_near, e_eps, e_gates) = probe_inputs[name]
    assert {"clustered": k_gates[0] == 0, "unclustered": k_gates[0] == 1, "one_cluster": k_gates[0] == 2}[name]   # the inputs are what they are called
    for _ in range(2):                                                # the second call: fresh workspace, same stream
        del spy_workspace[:]
        nat.knn_graph(planes, planes, 12)
        counts, gates, reserved = _gate_words(spy_workspace[0])
        assert np.array_equal(counts[:, 0], k_near) and np.array_equal(counts[:, 1], k_eps)
        assert gates == k_gates
        assert not reserved.any()
    if name == "one_cluster":
        return                                                        # (its eps <= 2 graph is all pairs: nothing more to learn)
    for _ in range(2):
        del spy_workspace[:]
        nat.eps_graph(planes, planes, nat.CMP_LE, 2)
        counts, gates, reserved = _gate_words(spy_workspace[0])
        assert np.array_equal(counts[:, 0], e_near) and np.array_equal(counts[:, 1], e_eps)
        assert gates == e_gates
        assert not reserved.any()


@pytest.mark.parametrize("force", ["0", "1", "2", "3", "4"])
def test_forced_gate_words(nat, probe_inputs, spy_workspace, monkeypatch, force):
    planes = probe_inputs["clustered"][0]
    monkeypatch.setenv("PG_GATE_FORCE", force)
    f = int(force)
    for _ in range(2):
        del spy_workspace[:]
        nat.knn_graph(planes, planes, 12)
        _, gates, reserved = _gate_words(spy_workspace[0])
        assert gates == ((f & 1) + (2 if f & 4 else 0), (f >> 1) & 1)
        assert not reserved.any()


def test_short_probe_grids(nat, probe_inputs, spy_workspace, monkeypatch):
    """PG_PROBE_S / PG_PROBE_W shrink the probe's grid - down to one wave, and to a last workgroup with idle waves - and
    the decision still comes out."""
    planes = probe_inputs["clustered"][0]
    for s, w in [("1", "1"), ("3", "2"), ("5", "3"), ("64", "1")]:
        monkeypatch.setenv("PG_PROBE_S", s)
        monkeypatch.setenv("PG_PROBE_W", w)
        monkeypatch.setenv("PG_GATE_FORCE", "1")
        del spy_workspace[:]
        nat.knn_graph(planes, planes, 12)
        _, gates, reserved = _gate_words(spy_workspace[0])
        assert gates == (1, 0) and not reserved.any(), (s, w)
        monkeypatch.setenv("PG_GATE_FORCE", "2")
        del spy_workspace[:]
        nat.knn_graph(planes, planes, 12)
        _, gates, reserved = _gate_words(spy_workspace[0])
        assert gates == (0, 1) and not reserved.any(), (s, w)


# ---------------------------------------------------------------------------------------------------------------------
# kNN: 64-row passes (the instance with the progress-driven issue priority) at the edges of a sweep
# ---------------------------------------------------------------------------------------------------------------------
def host_knn(tok, r0, nr, k):
    """Ranks 1..k of the canonical (distance, column) order of rows [r0, r0 + nr) against all rows."""
    d = np.concatenate([(tok[a:min(a + 128, r0 + nr), None, :] != tok[None, :, :]).sum(axis=2) for a in range(r0, r0 + nr, 128)]).astype(np.int64)
    key = np.sort(d * (1 << 24) + np.arange(len(tok))[None, :], axis=1)[:, 1:k + 1]
    return (key & ((1 << 24) - 1)).astype(np.int32), (key >> 24).astype(np.uint8)


@pytest.fixture(scope="module")
def knn_cases():
    from prograph_amd import synth
    big = synth.clustered_tokens(3077, 64, seed=31, members=64)       # 25 super-tiles of 128 columns
    small = synth.clustered_tokens(1500, 64, seed=32, members=64)     # 12 super-tiles: fewer than the 16 priority steps
    return {
        "rows_from_column_0": (big, 0, 69),                           # one pass of 64 rows and five more
        "rows_end_in_the_last_super_tile": (big, 3077 - 69, 69),
        "fewer_than_16_super_tiles": (small, 0, 1500),                # 23 passes and 28 rows
    }


@pytest.mark.parametrize("case", ["rows_from_column_0", "rows_end_in_the_last_super_tile", "fewer_than_16_super_tiles"])
def test_knn_64_row_passes_at_sweep_edges(nat, knn_cases, monkeypatch, case):
    tok, r0, nr = knn_cases[case]
    monkeypatch.setenv("PG_ENGINE", "mfma")
    monkeypatch.setenv("PG_MM_R", "2")
    planes = nat.pack(torch.from_numpy(tok), bits=5)
    want_idx, want_d = host_knn(tok, r0, nr, 16)
    idx, dist = nat.knn_graph(planes, planes, 16, row0=r0, nrows=nr)
    assert np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(dist.cpu().numpy(), want_d)
    if case == "fewer_than_16_super_tiles":                          # the numpy order above is the oracle's
        from oracle import prograph_oracle as O
        rk = O.neighbours_to_knn(O.build_graph(tok.astype(np.int64), k=16))
        assert np.array_equal(want_idx, rk[0]) and np.array_equal(want_d, rk[1])
