"""Update / EncodeIdx on host memory: rs_update, rs_encode_idx,
rs_update_batch, rs_codec_overwrite and their Python mirrors. Expected bytes come from the
oracles alone: after an update the parity is cref.encode of the new data, after EncodeIdx the
starting parity XOR cref.apply(P[:, changed], shards), after an overwrite every shard is
oracle.rs_oracle.codec_encode of the overwritten object. Every case asserts before the call
that old != new in every changed shard and that the expected parity differs from the starting
parity, so a call that does nothing cannot pass; data shards, new shards and the bytes behind
every buffer must stay what they were."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref, rs_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS_OK, RS_E_NO_DATA, RS_E_ARG = 0, -5, -10
SENT = 32


@pytest.fixture(scope="module")
def ctx1(native_lib):
    """A context of one device: its lane's table cache makes counters repeatable."""
    c = native_lib.Context(1)
    yield c
    c.close()


def _counters(Nat, ctx):
    c = Nat.HostCounters()
    assert Nat.lib.rs_host_counters_read(ctx.handle, ctypes.byref(c)) == 0
    return {n: int(getattr(c, n)) for n, _ in c._fields_}


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


@functools.lru_cache(maxsize=None)
def _stripe(k, m, S, changed, seed):
    """(old [k][S], new [k][S], parity of old [m][S], parity of new [m][S]), read-only."""
    rng = np.random.default_rng(seed)
    old = rng.integers(0, 256, (k, S), dtype=np.uint8)
    new = old.copy()
    for i in changed:
        new[i] = rng.integers(0, 256, S, dtype=np.uint8)
        new[i][0] = old[i][0] ^ 0x80
        assert not np.array_equal(new[i], old[i])
    p0 = np.stack(cref.encode(list(old), k, m))
    p1 = np.stack(cref.encode(list(new), k, m)) if changed else p0
    if changed:  # every entry of P is non-zero (MDS): one changed shard changes every row
        assert not np.array_equal(p0, p1)
        assert len(changed) > 1 or all(not np.array_equal(p0[j], p1[j]) for j in range(m))
    for a in (old, new, p0, p1):
        a.setflags(write=False)
    return old, new, p0, p1


def _buf(src, alloc=None):
    """A writable copy of `src` with SENT bytes of 0xA5 behind it."""
    a = (alloc or (lambda nb: np.empty(nb, np.uint8)))(len(src) + SENT)
    a[:len(src)] = src
    a[len(src):] = 0xA5
    return a


def _vp(arrs):
    return (ctypes.c_void_p * max(len(arrs), 1))(*[0 if a is None else a.ctypes.data for a in arrs])


def _intact(bufs, srcs):
    for a, s in zip(bufs, srcs):
        if a is not None:
            assert np.array_equal(a[:len(s)], s) and (a[len(s):] == 0xA5).all()


@pytest.mark.parametrize("S", [1, 17, 4096, 2 ** 20 + 1])
@pytest.mark.parametrize("k,m", [(3, 2), (10, 4), (16, 4), (10, 20)])
def test_update_and_progressive_encode_idx(native_lib, ctx1, k, m, S):
    L = native_lib.lib
    changed = (0, k - 1)
    old, new, p0, p1 = _stripe(k, m, S, changed, 1000 * k + m)
    ob = [_buf(old[i]) if i in changed else None for i in range(k)]
    nb = [_buf(new[i]) if i in changed else None for i in range(k)]
    pb = [_buf(p0[j]) for j in range(m)]
    assert L.rs_update(ctx1.handle, k, m, S, _vp(ob), _vp(nb), _vp(pb)) == RS_OK
    _intact(pb, p1)
    _intact(ob, [old[i] for i in range(k)])
    _intact(nb, [new[i] for i in range(k)])
    # EncodeIdx: the k shards of the new data in a shuffled order over zeroed parity
    order = [int(i) for i in np.random.default_rng(S + k).permutation(k)]
    pz = [_buf(np.zeros(S, np.uint8)) for _ in range(m)]
    shards = [_buf(new[i]) for i in range(k)]
    assert p1.any()
    for i in order:
        assert L.rs_encode_idx(ctx1.handle, k, m, S, ctypes.c_void_p(shards[i].ctypes.data), i, _vp(pz)) == RS_OK
    _intact(pz, p1)
    _intact(shards, list(new))


SETS = [(0,), (9,), (3, 7), (), (0, 1, 2)]


def _batch(k, m, sizes, seed, alloc=None):
    st = [_stripe(k, m, S, tuple(i for i in SETS[b % len(SETS)] if i < k), seed + b)
          for b, S in enumerate(sizes)]
    sets = [tuple(i for i in SETS[b % len(SETS)] if i < k) for b in range(len(sizes))]
    ob = [_buf(st[b][0][i], alloc) if i in sets[b] else None for b in range(len(sizes)) for i in range(k)]
    nb = [_buf(st[b][1][i], alloc) if i in sets[b] else None for b in range(len(sizes)) for i in range(k)]
    pb = [_buf(st[b][2][j], alloc) for b in range(len(sizes)) for j in range(m)]
    return st, sets, ob, nb, pb


def _check_batch(k, m, st, sets, ob, nb, pb, status, skip=()):
    for b in range(len(st)):
        old, new, p0, p1 = st[b]
        ran = b not in skip
        assert status[b] == (RS_OK if ran else status[b])
        _intact(pb[b * m:(b + 1) * m], p1 if ran else p0)
        _intact(ob[b * k:(b + 1) * k], list(old))
        _intact(nb[b * k:(b + 1) * k], list(new))


@pytest.mark.parametrize("k,m,sizes", [(10, 4, tuple(1 + 634 * b for b in range(64))),
                                       (10, 20, tuple(1 + 150 * b for b in range(64)))])
def test_update_batch_is_one_round_trip(native_lib, ctx1, k, m, sizes):
    """64 stripes of sizes 1..40,000 (RS(10,20): two launch groups) with mixed changed sets: one
    call, one chunk, one launch per group of 16 rows, a status per stripe."""
    L = native_lib.lib
    assert max(sizes) <= 40_000 and len(set(sizes)) == 64
    st, sets, ob, nb, pb = _batch(k, m, sizes, seed=7)
    B = len(sizes)
    szs = (ctypes.c_size_t * B)(*sizes)
    # stripe 5 (changed {0}) has no old bytes: RS_E_ARG, and its parity stays; stripe 6 ({9}) has size 0
    ob[5 * k + 0] = None
    szs[6] = 0
    status = (ctypes.c_int * B)(*([99] * B))
    c0 = _counters(native_lib, ctx1)
    rc = L.rs_update_batch(ctx1.handle, k, m, B, szs, _vp(ob), _vp(nb), _vp(pb), status)
    d = _delta(c0, _counters(native_lib, ctx1))
    assert rc == RS_E_ARG  # the first nonzero status in stripe order
    assert status[5] == RS_E_ARG and status[6] == RS_E_NO_DATA
    assert [status[b] for b in range(B) if b not in (5, 6)] == [RS_OK] * (B - 2)
    assert d["calls"] == 1 and d["chunks"] == 1 and d["launches"] == (m + 15) // 16, d
    assert d["ragged_calls"] == 1
    ob[5 * k + 0] = _buf(st[5][0][0])
    _check_batch(k, m, st, sets, ob, nb, pb, list(status), skip=(5, 6))


def test_update_batch_encode_idx_mode(native_lib, ctx1):
    L = native_lib.lib
    k, m = 10, 4
    sizes = [1 + 634 * b for b in range(0, 64, 3)]
    st, sets, ob, nb, pb = _batch(k, m, sizes, seed=9)
    B = len(sizes)
    E = cref.encode_matrix(k, m)
    rng = np.random.default_rng(4)
    start = [rng.integers(0, 256, S, dtype=np.uint8) for S in sizes for _ in range(m)]
    pb = [_buf(s) for s in start]
    status = (ctypes.c_int * B)()
    assert L.rs_update_batch(ctx1.handle, k, m, B, (ctypes.c_size_t * B)(*sizes), None, _vp(nb), _vp(pb),
                             status) == RS_OK
    for b in range(B):
        want = start[b * m:(b + 1) * m]
        if sets[b]:
            add = cref.apply(E[k:, list(sets[b])], [st[b][1][i] for i in sets[b]])
            want = [w ^ a for w, a in zip(want, add)]
            assert any(not np.array_equal(w, s) for w, s in zip(want, start[b * m:(b + 1) * m]))
        _intact(pb[b * m:(b + 1) * m], want)
    _intact(nb, [st[b][1][i] for b in range(B) for i in range(k)])


def test_pinned_buffers_take_the_staged_route(native_lib, ctx1):
    """Every buffer in rs_host_alloc memory, above the zero-copy threshold: still chunks."""
    L = native_lib.lib
    k, m = 10, 4
    sizes = [100_000, 17, 65_536 + 5]
    pinned = native_lib.PinnedBuffer(sum(sizes) * (2 * k + m) + 64 * 3 * (2 * k + m) * 2, ctx1)
    at = [0]

    def alloc(nb):
        a = pinned.array[at[0]:at[0] + nb]
        at[0] += (nb + 63) // 64 * 64
        return a

    st, sets, ob, nb, pb = _batch(k, m, sizes, seed=21, alloc=alloc)
    B = len(sizes)
    status = (ctypes.c_int * B)()
    c0 = _counters(native_lib, ctx1)
    assert L.rs_update_batch(ctx1.handle, k, m, B, (ctypes.c_size_t * B)(*sizes), _vp(ob), _vp(nb), _vp(pb),
                             status) == RS_OK
    d = _delta(c0, _counters(native_lib, ctx1))
    assert d["calls"] == 1 and d["chunks"] >= 1 and d["copies"] >= 2 * d["chunks"], d
    _check_batch(k, m, st, sets, ob, nb, pb, list(status))
    del st, ob, nb, pb
    pinned.close()


def test_no_change_moves_no_counter(native_lib, ctx1):
    L = native_lib.lib
    k, m, S = 10, 4, 4096
    old, new, p0, p1 = _stripe(k, m, S, (), 3)
    pb = [_buf(p0[j]) for j in range(m)]
    ob = [_buf(old[i]) for i in range(k)]
    none = [None] * k
    c0 = _counters(native_lib, ctx1)
    assert L.rs_update(ctx1.handle, k, m, S, _vp(ob), _vp(none), _vp(pb)) == RS_OK
    status = (ctypes.c_int * 2)(9, 9)
    assert L.rs_update_batch(ctx1.handle, k, m, 2, (ctypes.c_size_t * 2)(S, 0), _vp(ob + ob), _vp(none + none),
                             _vp(pb + pb), status) == RS_OK
    assert list(status) == [RS_OK, RS_OK]
    assert L.rs_update_batch(ctx1.handle, k, m, 0, None, None, None, None, None) == RS_OK
    assert _delta(c0, _counters(native_lib, ctx1)) == {n: 0 for n in c0}
    _intact(pb, p0)


_CUTS_CHILD = r"""
import ctypes, sys
import numpy as np
from oracle import cref
from callfs_amd import _native as N

k, m, S = 4, 2, 300_000
rng = np.random.default_rng(8)
old = rng.integers(0, 256, (k, S), dtype=np.uint8)
new = old.copy()
changed = (1, 3)
for i in changed:
    new[i] ^= rng.integers(1, 256, S, dtype=np.uint8)
p0 = np.stack(cref.encode(list(old), k, m))
p1 = np.stack(cref.encode(list(new), k, m))
assert all(not np.array_equal(p0[j], p1[j]) for j in range(m))
par = p0.copy()
ctx = N.Context(1)
vp = lambda rows: (ctypes.c_void_p * len(rows))(*[0 if r is None else r.ctypes.data for r in rows])
c0, c1 = N.HostCounters(), N.HostCounters()
N.lib.rs_host_counters_read(ctx.handle, ctypes.byref(c0))
rc = N.lib.rs_update(ctx.handle, k, m, S, vp([old[i] if i in changed else None for i in range(k)]),
                     vp([new[i] if i in changed else None for i in range(k)]), vp(list(par)))
N.lib.rs_host_counters_read(ctx.handle, ctypes.byref(c1))
chunks = c1.chunks - c0.chunks
ok = rc == 0 and np.array_equal(par, p1) and chunks >= 3 and c1.launches - c0.launches == chunks
print("column cuts child:", "ok" if ok else "rc=%d chunks=%d equal=%s" % (rc, chunks, np.array_equal(par, p1)))
ctx.close()
sys.exit(0 if ok else 1)
"""


def test_column_cuts(native_lib):
    """CALLFS_RS_CHUNK_BYTES is read once per process: in a fresh child a 300,000-byte stripe of
    six staged rows is cut into at least three column chunks."""
    env = dict(os.environ)
    env["CALLFS_RS_CHUNK_BYTES"] = str(512 << 10)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _CUTS_CHILD], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "column cuts child: ok" in r.stdout


def _ranges(k, S):
    """(offset, len): inside one shard, across one boundary, whole middle shards, the first byte,
    the last byte, the whole object, and a range that ends in an earlier column than it starts."""
    total = k * S
    out = [(S + 2, min(5, S - 2)), (S - 3, 7), (S - 1, 2 * S + 2), (0, 1), (total - 1, 1), (0, total),
           (2 * S - 2, 5), (S, S), (3, total - 5)]
    return [(o, n) for o, n in out if n > 0 and o + n <= total]


@pytest.mark.parametrize("S", [17, 4097])
@pytest.mark.parametrize("k,m", [(4, 2), (10, 4)])
def test_codec_overwrite(native_lib, ctx1, k, m, S):
    from callfs_amd.erasure import Codec, ErasureProfile
    L = native_lib.lib
    rng = np.random.default_rng(S * k)
    obj = rng.integers(0, 256, k * S, dtype=np.uint8)
    codec = Codec(ctx1)
    for q, (off, n) in enumerate(_ranges(k, S)):
        shards = [_buf(np.asarray(s)) for s in rs_oracle.codec_encode(obj.tobytes(), k, m)]
        data = obj[off:off + n] ^ rng.integers(1, 256, n, dtype=np.uint8)  # differs in every byte
        new_obj = obj.copy()
        new_obj[off:off + n] = data
        want = [np.asarray(s) for s in rs_oracle.codec_encode(new_obj.tobytes(), k, m)]
        assert any(not np.array_equal(want[k + j], shards[k + j][:S]) for j in range(m))
        dbuf = _buf(data)
        if q % 2:
            views = [memoryview(s)[:S] for s in shards]
            codec.overwrite(views, ErasureProfile(k, m), off, memoryview(dbuf)[:n])
        else:
            assert L.rs_codec_overwrite(ctx1.handle, k, m, S, _vp(shards), off,
                                        ctypes.c_void_p(dbuf.ctypes.data), n) == RS_OK
        _intact(shards, want)
        _intact([dbuf], [data])
    # untouched data shards may be NULL
    shards = [_buf(np.asarray(s)) for s in rs_oracle.codec_encode(obj.tobytes(), k, m)]
    data = obj[S:S + 3] ^ 0xFF
    new_obj = obj.copy()
    new_obj[S:S + 3] = data
    want = [np.asarray(s) for s in rs_oracle.codec_encode(new_obj.tobytes(), k, m)]
    part = [s if i == 1 or i >= k else None for i, s in enumerate(shards)]
    assert L.rs_codec_overwrite(ctx1.handle, k, m, S, _vp(part), S, ctypes.c_void_p(data.ctypes.data), 3) == RS_OK
    _intact(shards, want)


def test_errors(native_lib, ctx1):
    from callfs_amd import erasure as E
    L = native_lib.lib
    k, m, S = 4, 2, 64
    old, new, p0, p1 = _stripe(k, m, S, (1,), 5)
    pb = [_buf(p0[j]) for j in range(m)]
    ob, nb = [None, _buf(old[1]), None, None], [None, _buf(new[1]), None, None]
    h = ctx1.handle
    assert L.rs_update(h, k, m, 0, _vp(ob), _vp(nb), _vp(pb)) == RS_E_NO_DATA
    assert L.rs_update(h, k, m, S, _vp([None] * k), _vp(nb), _vp(pb)) == RS_E_ARG      # ErrInvalidInput
    assert L.rs_update(h, k, m, S, _vp(ob), _vp(nb), _vp([pb[0], None])) == RS_E_ARG
    assert L.rs_encode_idx(h, k, m, S, ctypes.c_void_p(nb[1].ctypes.data), k, _vp(pb)) == RS_E_ARG
    assert L.rs_encode_idx(h, k, m, 0, ctypes.c_void_p(nb[1].ctypes.data), 1, _vp(pb)) == RS_E_NO_DATA
    assert L.rs_encode_idx(h, k, m, S, ctypes.c_void_p(nb[1].ctypes.data), 1, _vp([None, pb[1]])) == RS_E_ARG
    _intact(pb, p0)
    # the Python mirror
    shards = [None, bytearray(old[1]), None, None] + [bytearray(p0[j]) for j in range(m)]
    with pytest.raises(E.ErrInvalidInput):
        E.update([None] * k + shards[k:], [None, bytes(new[1]), None, None], k, m, ctx1)
    with pytest.raises(E.ErrInvalidShardIdx):
        E.encode_idx(bytes(new[1]), k, shards[k:], k, m, ctx1)
    with pytest.raises(E.ErrInvalidProfile):
        E.Codec(ctx1).overwrite(shards, E.ErasureProfile(0, 2), 0, b"x")
    assert [bytes(s) for s in shards[k:]] == [bytes(p) for p in p0]
    E.update(shards, [None, bytes(new[1]), None, None], k, m, ctx1)
    assert [bytes(s) for s in shards[k:]] == [bytes(p) for p in p1]
    assert bytes(shards[1]) == bytes(old[1])  # the data shards remain the same
    par = [bytearray(S) for _ in range(m)]
    for i in (2, 0, 3, 1):
        E.encode_idx(bytes(new[i]), i, par, k, m, ctx1)
    assert [bytes(s) for s in par] == [bytes(p) for p in p1]
    st = E.update_batch([[None, bytes(old[1]), None, None], [None] * k],
                        [[None, bytes(new[1]), None, None], [None] * k],
                        [[bytearray(p0[j]) for j in range(m)], [bytearray(3) for _ in range(m)]], k, m, ctx1)
    assert st == [RS_OK, RS_OK]
    with pytest.raises(native_lib.NativeError):  # a range past k*S: RS_E_ARG
        E.Codec(ctx1).overwrite([bytearray(S) for _ in range(k + m)], E.ErasureProfile(k, m), k * S, b"x")
