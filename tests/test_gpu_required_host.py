"""Host calls that rebuild only the shards a caller asks for:
rs_reconstruct_some, rs_reconstruct_some_batch, rs_codec_decode_data and its batch form.

Every wanted shard is compared byte for byte with the oracle's codeword (oracle.cref); every
other buffer -- the unwanted missing shards and the sentinel bytes behind each shard -- must be
what it was, and an unwanted shard's `lens` entry stays 0. Unwanted missing shards always get a
real (sentinel-filled) buffer here; that their pointers reach no table is shown on the CPU
(tests/native/required_host_test.cpp, required_routes.cpp).

The batch runs through the three transports in one process: pageable buffers whose staging is
under CALLFS_RS_SMALL_MAX_BYTES (in place), pageable buffers above it (staged) and
rs_host_alloc buffers (direct)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

RS_OK, RS_E_TOO_FEW, RS_E_SHARD_SIZE, RS_E_NO_DATA, RS_E_CORRUPT, RS_E_INSUFFICIENT = 0, -3, -4, -5, -6, -7
SENT = 32
K, M, N_ = 10, 4, 14
SIZES_SMALL = [1 + 37 * b for b in range(64)]        # 64 sizes, ~1 MiB of staging in all
SIZES_LARGE = [1000 + 997 * b for b in range(64)]    # ~29 MiB: every class above the small limit


@pytest.fixture(scope="module")
def ctx1(native_lib):
    """A context of one device: its lane's table cache makes counters repeatable."""
    c = native_lib.Context(1)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _codewords(k, m, sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for S in sizes:
        data = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
        full = data + [np.ascontiguousarray(p) for p in cref.encode(data, k, m)]
        for a in full:
            a.setflags(write=False)
        out.append(full)
    return out


def _ptrs(arrs):
    return (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])


def _counters(Nat, ctx):
    c = Nat.HostCounters()
    assert Nat.lib.rs_host_counters_read(ctx.handle, ctypes.byref(c)) == 0
    return {n: int(getattr(c, n)) for n, _ in c._fields_}


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def _cases(n, k, batch, seed):
    """Seeded (missing, wanted) index sets per stripe: 0..m lost, a seeded subset wanted, flags
    on present shards thrown in. Stripes 0..3: w = 0 with c > 0; w = m; r = 0; all wanted."""
    m = n - k
    rng = np.random.default_rng(seed)
    lost, want = [], []
    for _ in range(batch):
        l = sorted(int(i) for i in rng.choice(n, size=int(rng.integers(0, m + 1)), replace=False))
        w = [i for i in l if rng.integers(0, 2)] + [int(rng.integers(0, n))]
        lost.append(l)
        want.append(sorted(set(w)))
    lost[0], want[0] = [1], [0, n - 1]
    lost[1], want[1] = list(range(1, m + 1)), list(range(n))
    lost[2], want[2] = list(range(k - 1, k - 1 + m)), []
    lost[3], want[3] = [0, n - 1], [0, n - 1]
    return lost, want


class _Batch:
    """Buffers of a batch: present shards hold the codeword, missing ones 0x5A, every buffer
    SENT bytes of 0xA5 behind it. alloc(nbytes) gives a writable uint8 array."""

    def __init__(self, k, m, sizes, lost, seed, alloc=None):
        self.k, self.m, self.n, self.sizes, self.lost = k, m, k + m, sizes, lost
        self.cw = _codewords(k, m, tuple(sizes), seed)
        alloc = alloc or (lambda nb: np.empty(nb, np.uint8))
        B, n = len(sizes), self.n
        self.bufs, self.lens = [], (ctypes.c_size_t * (B * n))()
        for b, S in enumerate(sizes):
            for i in range(n):
                a = alloc(S + SENT)
                a[S:] = 0xA5
                a[:S] = 0x5A if i in lost[b] else self.cw[b][i]
                self.lens[b * n + i] = 0 if i in lost[b] else S
                self.bufs.append(a)

    def snapshot(self):
        self.before = [a.copy() for a in self.bufs]

    def check(self, want, status, ran=(RS_OK, RS_E_CORRUPT)):
        """Wanted missing shards of the stripes that ran hold the codeword and their lens S;
        every other buffer and lens entry is unchanged."""
        n = self.n
        for b, S in enumerate(self.sizes):
            for i in range(n):
                a = self.bufs[b * n + i]
                if i in self.lost[b] and i in want[b] and status[b] in ran:
                    assert np.array_equal(a[:S], self.cw[b][i]), (b, i, S)
                    assert (a[S:] == 0xA5).all(), (b, i)
                    assert self.lens[b * n + i] == S, (b, i)
                else:
                    assert np.array_equal(a, self.before[b * n + i]), (b, i, S)
                    assert self.lens[b * n + i] == (0 if i in self.lost[b] else S), (b, i)


def _required(n, want):
    return (ctypes.c_uint8 * (len(want) * n))(*[1 if i in w else 0 for w in want for i in range(n)])


def test_reconstruct_some_alone(native_lib, ctx1):
    L = native_lib.lib
    S = 100_003
    lost, want = [[0, 3, 12]], [[3, 5]]
    bt = _Batch(K, M, [S], lost, seed=1)
    bt.snapshot()
    assert L.rs_reconstruct_some(ctx1.handle, K, M, _ptrs(bt.bufs), bt.lens, _required(N_, want)) == RS_OK
    bt.check(want, [RS_OK])
    assert bt.lens[3] == S and bt.lens[0] == 0 and bt.lens[12] == 0
    # nothing wanted: RS_OK and no device work
    bt = _Batch(K, M, [S], lost, seed=1)
    bt.snapshot()
    c0 = _counters(native_lib, ctx1)
    assert L.rs_reconstruct_some(ctx1.handle, K, M, _ptrs(bt.bufs), bt.lens, _required(N_, [[1, 13]])) == RS_OK
    assert _delta(c0, _counters(native_lib, ctx1)) == {k: 0 for k in c0}
    bt.check([[]], [RS_OK])
    # NULL: rs_reconstruct
    bt = _Batch(K, M, [S], lost, seed=1)
    bt.snapshot()
    assert L.rs_reconstruct_some(ctx1.handle, K, M, _ptrs(bt.bufs), bt.lens, None) == RS_OK
    bt.check([lost[0]], [RS_OK])
    # too few shards, whatever is wanted
    bt = _Batch(K, M, [64], [[0, 1, 2, 3, 4]], seed=2)
    assert L.rs_reconstruct_some(ctx1.handle, K, M, _ptrs(bt.bufs), bt.lens, _required(N_, [[0]])) == RS_E_TOO_FEW


@pytest.mark.parametrize("verify", [0, 1])
@pytest.mark.parametrize("transport", ["inplace", "staged", "direct"])
def test_some_batch(native_lib, ctx1, transport, verify):
    """A 64-stripe RS(10,4) batch of 64 sizes with seeded masks and wanted sets."""
    L = native_lib.lib
    sizes = SIZES_SMALL if transport == "inplace" else SIZES_LARGE
    B = len(sizes)
    lost, want = _cases(N_, K, B, seed=40 + verify)
    lost[10] = [0, 1, 2, 3, 4]          # too few shards
    lost[20], want[20] = [2, 11], [2]   # written {2}, compared {12, 13}: flipped below
    pinned = []
    alloc = None
    if transport == "direct":  # one rs_host_alloc allocation, carved into the shards' buffers
        pinned.append(native_lib.PinnedBuffer(sum((S + SENT + 63) // 64 * 64 for S in sizes) * N_, ctx1))
        at = [0]

        def alloc(nb):
            a = pinned[0].array[at[0]:at[0] + nb]
            at[0] += (nb + 63) // 64 * 64
            return a
    bt = _Batch(K, M, sizes, lost, seed=9, alloc=alloc)
    bt.bufs[20 * N_ + 13][sizes[20] - 1] ^= 0x10
    bt.snapshot()
    status = (ctypes.c_int * B)(*[77] * B)
    c0 = _counters(native_lib, ctx1)
    rc = L.rs_reconstruct_some_batch(ctx1.handle, K, M, B, _ptrs(bt.bufs), bt.lens,
                                     _required(N_, want), verify, status)
    d = _delta(c0, _counters(native_lib, ctx1))
    st = list(status)
    expect = [RS_OK] * B
    expect[10] = RS_E_TOO_FEW
    if verify:
        expect[20] = RS_E_CORRUPT
    assert st == expect
    assert rc == next(s for s in st if s)
    bt.check(want, st)
    # one ragged call, its stripes in classes by row count, one run each
    rows = set()
    for b in range(B):
        if b == 10:
            continue
        w = len([i for i in lost[b] if i in want[b]])
        c = (N_ - len(lost[b]) - K) if verify else 0
        rows.add(w + c)
    classes = len(rows - {0})
    assert classes >= 3
    assert d["calls"] == 1 and d["ragged_calls"] == 1
    if transport == "inplace":
        assert d["chunks"] == classes and d["copies"] <= classes, d  # (table uploads alone)
    elif transport == "staged":  # (at least one class is above the small limit: H2D and D2H)
        assert d["chunks"] >= classes and d["copies"] > classes, d
    else:
        assert d["chunks"] == classes, d
    for p in pinned:
        p.close()


def test_counters(native_lib, ctx1):
    L = native_lib.lib
    sizes = SIZES_SMALL[:16]
    B = len(sizes)
    # a batch of stripes without a row reaches no device
    lost = [[0, 1, 12, 13] if b % 2 else [] for b in range(B)]
    want = [[5] if b % 2 else [0] for b in range(B)]
    for verify in (0, 1):
        if verify:  # with verify, nothing to compare either: exactly k present everywhere
            lost, want = [[0, 1, 12, 13]] * B, [[5, 10]] * B
        bt = _Batch(K, M, sizes, lost, seed=3)
        bt.snapshot()
        status = (ctypes.c_int * B)(*[77] * B)
        c0 = _counters(native_lib, ctx1)
        assert L.rs_reconstruct_some_batch(ctx1.handle, K, M, B, _ptrs(bt.bufs), bt.lens,
                                           _required(N_, want), verify, status) == RS_OK
        assert _delta(c0, _counters(native_lib, ctx1)) == {k: 0 for k in c0}
        assert list(status) == [RS_OK] * B
        bt.check([[]] * B, list(status))
    # required == NULL counts exactly what rs_reconstruct_batch counts (tables cached by the
    # first call)
    lost, _ = _cases(N_, K, B, seed=5)
    deltas = []
    for which in ("warm", "full", "some"):
        bt = _Batch(K, M, sizes, lost, seed=3)
        bt.snapshot()
        status = (ctypes.c_int * B)(*[77] * B)
        c0 = _counters(native_lib, ctx1)
        if which == "some":
            rc = L.rs_reconstruct_some_batch(ctx1.handle, K, M, B, _ptrs(bt.bufs), bt.lens, None, 1, status)
        else:
            rc = L.rs_reconstruct_batch(ctx1.handle, K, M, B, _ptrs(bt.bufs), bt.lens, 1, status)
        assert rc == RS_OK and list(status) == [RS_OK] * B
        deltas.append(_delta(c0, _counters(native_lib, ctx1)))
        bt.check(lost, list(status))
    assert deltas[1] == deltas[2] and deltas[2]["calls"] == 1


def _decode(L, ctx, fn, bt, b, size):
    out = np.full(size + SENT, 0xC3, np.uint8)
    n = bt.n
    lens = (ctypes.c_size_t * n)(*bt.lens[b * n:(b + 1) * n])
    rc = fn(ctx.handle, bt.k, bt.m, _ptrs(bt.bufs[b * n:(b + 1) * n]), lens,
            ctypes.c_void_p(out.ctypes.data), size)
    return rc, out, list(lens)


def test_decode_data(native_lib, ctx1):
    """rs_codec_decode_data: rs_codec_decode's `out` byte for byte, missing parity left alone."""
    L = native_lib.lib
    sizes = [1, 17, 4097, 100_003, 700_001]
    lost = [[0, 13], [3, 10, 11], [12], [0, 1, 2, 3], [5, 11]]
    for b, S in enumerate(sizes):
        size = K * S - (S // 2 if S > 1 else 0)
        full = _Batch(K, M, sizes, lost, seed=6)
        rc0, out0, _ = _decode(L, ctx1, L.rs_codec_decode, full, b, size)
        data = _Batch(K, M, sizes, lost, seed=6)
        data.snapshot()
        rc1, out1, lens1 = _decode(L, ctx1, L.rs_codec_decode_data, data, b, size)
        assert rc0 == rc1 == RS_OK
        assert np.array_equal(out0, out1) and (out1[size:] == 0xC3).all()
        assert np.array_equal(out1[:size], np.concatenate(data.cw[b][:K])[:size])
        for i in range(N_):
            a = data.bufs[b * N_ + i]
            if i in lost[b] and i < K:
                assert np.array_equal(a[:S], data.cw[b][i]) and lens1[i] == S
            else:
                assert np.array_equal(a, data.before[b * N_ + i]), (b, i)
                assert lens1[i] == (0 if i in lost[b] else S)
    # all data present, exactly k shards: the bytes, and no device call
    bt = _Batch(K, M, [5000], [[10, 11, 12, 13]], seed=7)
    c0 = _counters(native_lib, ctx1)
    rc, out, lens = _decode(L, ctx1, L.rs_codec_decode_data, bt, 0, 49_999)
    assert rc == RS_OK and _delta(c0, _counters(native_lib, ctx1))["calls"] == 0
    assert np.array_equal(out[:49_999], np.concatenate(bt.cw[0][:K])[:49_999])
    assert (out[49_999:] == 0xC3).all() and lens[10:] == [0, 0, 0, 0]
    # a flipped compared shard
    bt = _Batch(K, M, [5000], [[0, 11]], seed=7)
    bt.bufs[13][77] ^= 1
    rc, out, lens = _decode(L, ctx1, L.rs_codec_decode_data, bt, 0, 50_000)
    assert rc == RS_E_CORRUPT and lens[0] == 5000 and lens[11] == 0


def test_decode_data_error_precedence(native_lib, ctx1):
    """The cases of test_decode_error_precedence (tests/test_gpu_parity.py), for both forms."""
    L = native_lib.lib
    k, m, n = 4, 2, 6
    for fn in (L.rs_codec_decode_data, L.rs_codec_decode):
        bt = _Batch(k, m, [25], [[]], seed=8)
        assert _decode(L, ctx1, fn, bt, 0, 101)[0] == RS_E_INSUFFICIENT
        bt = _Batch(k, m, [25], [list(range(n))], seed=8)
        assert _decode(L, ctx1, fn, bt, 0, 10)[0] == RS_E_NO_DATA
        bt = _Batch(k, m, [25], [[]], seed=8)
        bt.lens[1] = 24
        assert _decode(L, ctx1, fn, bt, 0, 100)[0] == RS_E_SHARD_SIZE
        bt = _Batch(k, m, [25], [[0, 1, 5]], seed=8)
        assert _decode(L, ctx1, fn, bt, 0, 100)[0] == RS_E_TOO_FEW
        # insufficient after a rebuild: the wanted shards are filled first
        bt = _Batch(k, m, [25], [[1, 4]], seed=8)
        rc, _, lens = _decode(L, ctx1, fn, bt, 0, 101)
        assert rc == RS_E_INSUFFICIENT and lens[1] == 25
        assert lens[4] == (0 if fn is L.rs_codec_decode_data else 25)


@pytest.mark.parametrize("sizes", [SIZES_SMALL[:24], SIZES_LARGE[:24]], ids=["inplace", "staged"])
def test_decode_data_batch(native_lib, ctx1, sizes):
    """rs_codec_decode_data_batch against rs_codec_decode_batch on the same objects."""
    L = native_lib.lib
    B = len(sizes)
    lost, _ = _cases(N_, K, B, seed=77)
    lost[4] = [10, 11, 12, 13]      # all data present, exactly k shards: a plain copy
    lost[5] = []                    # nothing missing: compared rows alone
    lost[6] = [0, 1, 2, 3, 4]       # too few
    lost[7] = [1, 12]               # compared shard 13 flipped below
    osz = [K * S - S // 3 for S in sizes]
    osz[8] = K * sizes[8] + 1       # insufficient
    outs = {}
    for name, fn in (("full", L.rs_codec_decode_batch), ("data", L.rs_codec_decode_data_batch)):
        bt = _Batch(K, M, sizes, lost, seed=10)
        bt.bufs[7 * N_ + 13][sizes[7] // 2] ^= 4
        bt.snapshot()
        out = [np.full(max(o, 1) + SENT, 0xC3, np.uint8) for o in osz]
        status = (ctypes.c_int * B)(*[77] * B)
        rc = fn(ctx1.handle, K, M, B, _ptrs(bt.bufs), bt.lens, _ptrs(out),
                (ctypes.c_int64 * B)(*osz), status)
        st = list(status)
        expect = [RS_OK] * B
        expect[6], expect[7], expect[8] = RS_E_TOO_FEW, RS_E_CORRUPT, RS_E_INSUFFICIENT
        assert st == expect and rc == RS_E_TOO_FEW, name
        outs[name] = out
        want = [list(range(K)) if name == "data" else list(range(N_))] * B
        bt.check(want, st, ran=(RS_OK, RS_E_CORRUPT, RS_E_INSUFFICIENT))
        for b in range(B):
            if st[b] == RS_OK:
                assert np.array_equal(out[b][:osz[b]], np.concatenate(bt.cw[b][:K])[:osz[b]]), (name, b)
                assert (out[b][osz[b]:] == 0xC3).all(), (name, b)
    for b in range(B):
        if b not in (6, 7, 8):
            assert np.array_equal(outs["full"][b], outs["data"][b]), b
