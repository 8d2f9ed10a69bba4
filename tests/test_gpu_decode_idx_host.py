"""DecodeIdx on host memory: rs_decode_idx, rs_decode_idx_batch and their Python
mirrors, against the oracle and against a decode-idx device plan over the same bytes. Expected
bytes come from oracle.cref alone: cref.reconstruct with present = expect after a complete feed,
the start XOR (merge) or exactly (store) cref.apply(C[:, delivered], inputs) after a partial one,
with C from cref.reconstruct of the unit vectors. Every case asserts before the call that every
delivered shard is non-zero in its first byte and that the expected bytes differ from the starting
bytes in every wanted shard, so a call that does nothing cannot pass; inputs, unwanted shards
and the bytes behind every buffer must stay what they were."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS_OK, RS_E_TOO_FEW_SHARDS, RS_E_NO_DATA, RS_E_ARG = 0, -3, -5, -10
STORE = 1
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


def _expected(k, m, b):
    """First k, last k, and two sets that mix data and parity."""
    n = k + m
    evens = (list(range(0, n, 2)) + list(range(1, n, 2)))[:k]
    return [tuple(range(k)), tuple(range(n - k, n)), tuple(sorted(evens)),
            tuple(sorted(set(range(n)) - set(range(1, 1 + m))))][b % 4]


def _wanted(k, m, e, b):
    """All that are not expected, one, two, none."""
    rest = [i for i in range(k + m) if i not in e]
    return tuple([rest, rest[-1:], rest[:1] + rest[-1:] if len(rest) > 1 else rest, []][(b // 4 + b) % 4])


@functools.lru_cache(maxsize=None)
def _coef(k, m, expect):
    """C (n, k): cref.reconstruct of the k unit vectors placed at the expected indices."""
    shards = [None] * (k + m)
    for j, v in enumerate(expect):
        shards[v] = np.zeros(k, dtype=np.uint8)
        shards[v][j] = 1
    C = np.stack(cref.reconstruct(shards, [i in expect for i in range(k + m)], k, m))
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def _stripe(k, m, S, expect, feeds, seed):
    """(data [k][S] of the expected shards in ascending index order, full [n][S] =
    cref.reconstruct from them, terms: per feed [n][S]). Redrawn until every feed's terms are
    non-zero in the first byte of every shard that is not expected."""
    rng = np.random.default_rng(seed)
    C = _coef(k, m, expect)
    rest = [i for i in range(k + m) if i not in expect]
    while True:
        data = rng.integers(0, 256, (k, S), dtype=np.uint8)
        data[:, 0] |= 1  # every delivered shard is non-zero in its first byte
        terms = [np.stack(cref.apply(C[:, list(f)], [data[j] for j in f])) for f in feeds]
        if all(t[w][0] != 0 for t in terms for w in rest):
            break
    shards = [None] * (k + m)
    for j, v in enumerate(expect):
        shards[v] = data[j]
    full = np.stack(cref.reconstruct(shards, [i in expect for i in range(k + m)], k, m))
    for a in [data, full] + terms:
        a.setflags(write=False)
    return data, full, terms


def _buf(src, alloc=None):
    """A writable copy of `src` with SENT bytes of 0xA5 behind it."""
    a = (alloc or (lambda nb: np.empty(nb, np.uint8)))(len(src) + SENT)
    a[:len(src)] = src
    a[len(src):] = 0xA5
    return a


def _vp(arrs):
    return (ctypes.c_void_p * max(len(arrs), 1))(*[None if a is None else a.ctypes.data for a in arrs])


def _u8(flags):
    return (ctypes.c_uint8 * max(len(flags), 1))(*[1 if f else 0 for f in flags])


def _intact(bufs, srcs):
    for a, s in zip(bufs, srcs):
        if a is not None:
            assert np.array_equal(a[:len(s)], s) and (a[len(s):] == 0xA5).all()


def _junk(rng, S, differ_from):
    j = rng.integers(0, 256, S, dtype=np.uint8)
    j[0] = differ_from[0] ^ 0x80
    return j


def _split(k, parts, seed):
    perm = [int(i) for i in np.random.default_rng(seed).permutation(k)]
    cuts = [round(q * k / parts) for q in range(parts + 1)]
    return tuple(f for f in (tuple(sorted(perm[cuts[q]:cuts[q + 1]])) for q in range(parts)) if f)


def _plan_feed(k, m, S, expect, wanted, feeds, data, start, store_first):
    """The same feeds through decode-idx device plans over device copies of the same bytes:
    the wanted shards' final bytes, as numpy rows."""
    import torch
    from callfs_amd.device import Plan
    n = k + m
    dev = torch.device("cuda:0")
    t = {v: torch.from_numpy(np.array(data[j])).to(dev) for j, v in enumerate(expect)}
    d = {w: torch.from_numpy(np.array(start[w])).to(dev) for w in wanted}
    for q, f in enumerate(feeds):
        deliver = {expect[j] for j in f}
        plan = Plan.decode_idx(k, m, [S], [[i in expect for i in range(n)]],
                               [t[i].data_ptr() if i in deliver else 0 for i in range(n)],
                               [d[i].data_ptr() if i in d else 0 for i in range(n)],
                               store=store_first and q == 0)
        plan.launch()
        torch.cuda.synchronize()
        plan.close()
    return {w: d[w].cpu().numpy() for w in wanted}


@pytest.mark.parametrize("S", [1, 17, 4096, 2 ** 20 + 1])
@pytest.mark.parametrize("k,m,which", [(3, 2, 2), (10, 4, 3), (16, 4, 1), (10, 20, 2)])
def test_progressive_decode(native_lib, ctx1, k, m, which, S):
    """Three calls deliver the k expected shards (data and parity mixed) in a shuffled split: from
    zeroed destinations by merging, and with the first call storing over junk. Both end in
    cref.reconstruct's bytes and in the bytes the device plans leave."""
    L = native_lib.lib
    n = k + m
    expect = _expected(k, m, which)
    wanted = tuple(i for i in range(n) if i not in expect)
    feeds = _split(k, 3, S + k)
    data, full, terms = _stripe(k, m, S, expect, feeds, 1000 * k + m)
    rng = np.random.default_rng(S)
    ex = _u8([i in expect for i in range(n)])
    for store_first in (False, True):
        start = {w: _junk(rng, S, terms[0][w]) if store_first else np.zeros(S, np.uint8) for w in wanted}
        dst = [_buf(start[i]) if i in wanted else None for i in range(n)]
        inputs = [_buf(data[expect.index(i)]) if i in expect else None for i in range(n)]
        now = {w: start[w] for w in wanted}
        for q, f in enumerate(feeds):
            store = store_first and q == 0
            deliver = {expect[j] for j in f}
            want = {w: terms[q][w] if store else now[w] ^ terms[q][w] for w in wanted}
            assert all(not np.array_equal(want[w], now[w]) for w in wanted)
            inp = [inputs[i] if i in deliver else None for i in range(n)]
            assert L.rs_decode_idx(ctx1.handle, k, m, S, _vp(dst), ex, _vp(inp), STORE if store else 0) == RS_OK
            _intact([dst[w] for w in wanted], [want[w] for w in wanted])
            now = want
        _intact([dst[w] for w in wanted], [full[w] for w in wanted])
        _intact([inputs[i] for i in expect], list(data))
        dev = _plan_feed(k, m, S, expect, wanted, feeds, data, start, store_first)
        for w in wanted:
            assert np.array_equal(dev[w], dst[w][:S]), w


def _batch(k, m, sizes, feed, seed, start="random", alloc=None):
    """Per stripe its own expected and wanted sets; `feed` (positions in V) delivered everywhere."""
    rng = np.random.default_rng(seed)
    n = k + m
    st, expect, wanted, inputs, dst, start_rows = [], [], [], [], [], []
    for b, S in enumerate(sizes):
        e = _expected(k, m, b)
        w = _wanted(k, m, e, b)
        data, full, terms = _stripe(k, m, S, e, (feed,), seed + b)
        st.append((data, full, terms[0]))
        expect.append(e)
        wanted.append(w)
        deliver = {e[j] for j in feed}
        inputs += [_buf(data[e.index(i)], alloc) if i in deliver else None for i in range(n)]
        rows = [None] * n
        for i in range(n):
            if i in w:
                rows[i] = _junk(rng, S, terms[0][i]) if start == "junk" else rng.integers(0, 256, S, dtype=np.uint8)
        start_rows.append(rows)
        dst += [_buf(rows[i], alloc) if rows[i] is not None else None for i in range(n)]
    return st, expect, wanted, inputs, dst, start_rows


def _check_batch(k, m, st, expect, wanted, inputs, dst, start_rows, feed, store, skip=()):
    n = k + m
    for b in range(len(st)):
        data, full, term = st[b]
        for w in wanted[b]:
            s0 = start_rows[b][w]
            want = s0 if b in skip else (term[w] if store else s0 ^ term[w])
            if b not in skip:
                assert not np.array_equal(want, s0)
            _intact([dst[b * n + w]], [want])
        for j in feed:
            _intact([inputs[b * n + expect[b][j]]], [data[j]])


@pytest.mark.parametrize("k,m,sizes", [(10, 4, tuple(1 + 634 * b for b in range(64))),
                                       (10, 20, tuple(1 + 150 * b for b in range(64)))])
def test_batch_is_one_round_trip_and_store_skips_the_upload(native_lib, ctx1, k, m, sizes):
    """64 stripes of sizes 1..40,000 (RS(10,20): two launch groups) with their own expected and
    wanted sets: one call, one chunk, one launch per group of 16 rows, a status per stripe. The
    `copies` counter shows that a store call does not upload the wanted shards: 2 per chunk (the
    H2D of metadata and inputs, the D2H) against a merge call's 3."""
    L = native_lib.lib
    assert max(sizes) <= 40_000 and len(set(sizes)) == 64
    n = k + m
    feed = (1, 4, 8)
    B = len(sizes)
    groups = (m + 15) // 16
    deltas = {}
    for mode, store in (("warm", False), ("merge", False), ("store", True)):
        st, expect, wanted, inputs, dst, start_rows = _batch(k, m, sizes, feed, seed=7,
                                                             start="junk" if store else "random")
        szs = (ctypes.c_size_t * B)(*sizes)
        ex = [i in expect[b] for b in range(B) for i in range(n)]
        # stripe 5 expects one shard too few; stripe 7 has size 0 (and wants shards)
        assert wanted[5] and wanted[7]
        ex[5 * n + expect[5][9]] = False
        szs[7] = 0
        status = (ctypes.c_int * B)(*([99] * B))
        c0 = _counters(native_lib, ctx1)
        rc = L.rs_decode_idx_batch(ctx1.handle, k, m, B, szs, _vp(dst), _u8(ex), _vp(inputs),
                                   STORE if store else 0, status)
        d = deltas[mode] = _delta(c0, _counters(native_lib, ctx1))
        assert rc == RS_E_TOO_FEW_SHARDS  # the first nonzero status in stripe order
        assert status[5] == RS_E_TOO_FEW_SHARDS and status[7] == RS_E_NO_DATA
        assert [status[b] for b in range(B) if b not in (5, 7)] == [RS_OK] * (B - 2)
        assert d["calls"] == 1 and d["chunks"] == 1 and d["launches"] == groups and d["ragged_calls"] == 1, d
        _check_batch(k, m, st, expect, wanted, inputs, dst, start_rows, feed, store, skip=(5, 7))
    # the tables are on the lane after the first call: what is left is the chunk's own copies
    assert deltas["merge"]["copies"] == 3 and deltas["store"]["copies"] == 2, deltas


def test_pinned_buffers_take_the_staged_route(native_lib, ctx1):
    """Every buffer in rs_host_alloc memory, above the zero-copy threshold: still chunks."""
    L = native_lib.lib
    k, m = 10, 4
    n = k + m
    sizes = [100_000, 17, 65_536 + 5]
    pinned = native_lib.PinnedBuffer(sum(sizes) * n + 64 * 3 * n * 2 + SENT * 3 * n, ctx1)
    at = [0]

    def alloc(nb):
        a = pinned.array[at[0]:at[0] + nb]
        at[0] += (nb + 63) // 64 * 64
        return a

    feed = (0, 3, 9)
    st, expect, wanted, inputs, dst, start_rows = _batch(k, m, sizes, feed, seed=21, alloc=alloc)
    B = len(sizes)
    status = (ctypes.c_int * B)()
    ex = [i in expect[b] for b in range(B) for i in range(n)]
    c0 = _counters(native_lib, ctx1)
    assert L.rs_decode_idx_batch(ctx1.handle, k, m, B, (ctypes.c_size_t * B)(*sizes), _vp(dst), _u8(ex),
                                 _vp(inputs), 0, status) == RS_OK
    d = _delta(c0, _counters(native_lib, ctx1))
    assert d["calls"] == 1 and d["chunks"] >= 1 and d["copies"] >= 3 * d["chunks"], d
    _check_batch(k, m, st, expect, wanted, inputs, dst, start_rows, feed, False)
    del st, inputs, dst
    pinned.close()


def test_nothing_to_do_moves_no_counter(native_lib, ctx1):
    L = native_lib.lib
    k, m, S = 10, 4, 4096
    n = k + m
    e = _expected(k, m, 2)
    data, full, terms = _stripe(k, m, S, e, ((0,),), 3)
    rest = [i for i in range(n) if i not in e]
    rng = np.random.default_rng(1)
    start = [rng.integers(0, 256, S, dtype=np.uint8) for _ in rest]
    dst = [_buf(start[rest.index(i)]) if i in rest else None for i in range(n)]
    inp = [_buf(data[e.index(i)]) if i in e else None for i in range(n)]
    none = [None] * n
    ex = _u8([i in e for i in range(n)])
    c0 = _counters(native_lib, ctx1)
    for flags in (0, STORE):
        assert L.rs_decode_idx(ctx1.handle, k, m, S, _vp(dst), ex, _vp(none), flags) == RS_OK  # nothing delivered
        assert L.rs_decode_idx(ctx1.handle, k, m, S, _vp(none), ex, _vp(inp), flags) == RS_OK  # nothing wanted
        status = (ctypes.c_int * 2)(9, 9)
        assert L.rs_decode_idx_batch(ctx1.handle, k, m, 2, (ctypes.c_size_t * 2)(S, 0), _vp(dst + none),
                                     _u8([i in e for i in range(n)] * 2), _vp(none + inp), flags, status) == RS_OK
        assert list(status) == [RS_OK, RS_OK]
    assert L.rs_decode_idx_batch(ctx1.handle, k, m, 0, None, None, None, None, 0, None) == RS_OK
    assert _delta(c0, _counters(native_lib, ctx1)) == {name: 0 for name in c0}
    _intact([dst[i] for i in rest], start)


_CUTS_CHILD = r"""
import ctypes, sys
import numpy as np
from oracle import cref
from callfs_amd import _native as N

k, m, S = 4, 2, 300_000
n = k + m
expect = (0, 2, 4, 5)
wanted = (1, 3)
rng = np.random.default_rng(8)
shards = [None] * n
for i in expect:
    shards[i] = rng.integers(1, 256, S, dtype=np.uint8)
full = np.stack(cref.reconstruct(shards, [i in expect for i in range(n)], k, m))
ctx = N.Context(1)
vp = lambda rows: (ctypes.c_void_p * len(rows))(*[None if r is None else r.ctypes.data for r in rows])
ex = (ctypes.c_uint8 * n)(*[1 if i in expect else 0 for i in range(n)])
ok = True
for first_store in (False, True):
    dst = {w: (full[w] ^ 0xFF) if first_store else np.zeros(S, np.uint8) for w in wanted}
    assert all(not np.array_equal(dst[w], full[w]) for w in wanted)
    c0, c1 = N.HostCounters(), N.HostCounters()
    N.lib.rs_host_counters_read(ctx.handle, ctypes.byref(c0))
    rc = 0
    for q, part in enumerate(((4, 0), (5, 2))):
        rc = rc or N.lib.rs_decode_idx(ctx.handle, k, m, S, vp([dst.get(i) for i in range(n)]), ex,
                                       vp([shards[i] if i in part else None for i in range(n)]),
                                       1 if first_store and q == 0 else 0)
    N.lib.rs_host_counters_read(ctx.handle, ctypes.byref(c1))
    chunks = c1.chunks - c0.chunks
    equal = all(np.array_equal(dst[w], full[w]) for w in wanted)
    good = rc == 0 and equal and chunks >= 6 and c1.launches - c0.launches == chunks and c1.calls - c0.calls == 2
    if not good:
        print("store" if first_store else "merge", "rc=%d chunks=%d equal=%s" % (rc, chunks, equal))
    ok = ok and good
print("column cuts child:", "ok" if ok else "failed")
ctx.close()
sys.exit(0 if ok else 1)
"""


def test_column_cuts(native_lib):
    """CALLFS_RS_CHUNK_BYTES is read once per process: in a fresh child, under a 256 KiB chunk
    budget, each call over a 300,000-byte stripe of four staged rows is cut into at least three
    column chunks, in merge mode and with a storing first call."""
    env = dict(os.environ)
    env["CALLFS_RS_CHUNK_BYTES"] = str(256 << 10)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _CUTS_CHILD], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "column cuts child: ok" in r.stdout


def test_errors_and_python_mirror(native_lib, ctx1):
    from callfs_amd import erasure as E
    L = native_lib.lib
    k, m, S = 4, 2, 64
    n = k + m
    e = (0, 1, 3, 5)
    feeds = ((2,), (0, 3), (1,))
    data, full, terms = _stripe(k, m, S, e, feeds, 5)
    rest = (2, 4)
    start = [np.full(S, 0x33, np.uint8) for _ in rest]
    dst = [_buf(start[rest.index(i)]) if i in rest else None for i in range(n)]
    inp = [_buf(data[e.index(i)]) if i == 0 else None for i in range(n)]
    h = ctx1.handle
    ex = _u8([i in e for i in range(n)])
    assert L.rs_decode_idx(h, k, m, 0, _vp(dst), ex, _vp(inp), 0) == RS_E_NO_DATA
    assert L.rs_decode_idx(h, k, m, S, _vp(dst), _u8([i in e[:3] for i in range(n)]), _vp(inp), 0) == RS_E_TOO_FEW_SHARDS
    assert L.rs_decode_idx(h, k, m, S, _vp(dst), _u8([i in e + (2,) for i in range(n)]), _vp(inp), 0) == RS_E_ARG
    assert L.rs_decode_idx(h, k, m, S, _vp(dst), ex, _vp([None, None, inp[0]] + [None] * 3), 0) == RS_E_ARG
    assert L.rs_decode_idx(h, k, m, S, _vp([dst[2]] + [None] * 5), ex, _vp(inp), 0) == RS_E_ARG
    assert L.rs_decode_idx(h, k, m, S, _vp(dst), ex, _vp(inp), 2) == RS_E_ARG
    _intact([dst[i] for i in rest], start)
    # the Python mirror: the same refusals as upstream-style errors, then a progressive decode
    flags = [i in e for i in range(n)]
    one = [bytes(data[e.index(i)]) if i == 0 else None for i in range(n)]
    out = [bytearray(S) if i in rest else None for i in range(n)]
    with pytest.raises(E.ErrTooFewShards):
        E.decode_idx(out, [i in e[:3] for i in range(n)], one, k, m, context=ctx1)
    with pytest.raises(E.ErrInvalidInput):
        E.decode_idx(out, [i in e + (2,) for i in range(n)], one, k, m, context=ctx1)
    with pytest.raises(E.ErrInvalidInput):
        E.decode_idx(out, flags, [None, None, bytes(S)] + [None] * 3, k, m, context=ctx1)
    with pytest.raises(E.ErrInvalidInput):
        E.decode_idx([bytearray(S)] + out[1:], flags, one, k, m, context=ctx1)
    with pytest.raises(E.ErrShardSize):
        E.decode_idx(out, flags, [bytes(S + 1)] + [None] * 5, k, m, context=ctx1)
    with pytest.raises(E.ErrTooFewShards):
        E.decode_idx(out[:-1], flags, one, k, m, context=ctx1)
    with pytest.raises(TypeError):
        E.decode_idx([bytes(S) if i in rest else None for i in range(n)], flags, one, k, m, context=ctx1)
    with pytest.raises(E.ErrInvalidProfile):
        E.decode_idx(out, flags, one, 0, m + k, context=ctx1)
    assert all(bytes(out[i]) == bytes(S) for i in rest)
    junk = [bytearray(b"\x77" * S) if i in rest else None for i in range(n)]
    for q, f in enumerate(feeds):
        got = [bytes(data[j]) if j in f else None for j in range(k)]
        row = [got[e.index(i)] if i in e else None for i in range(n)]
        E.decode_idx(out, flags, row, k, m, context=ctx1)
        E.decode_idx(junk, flags, row, k, m, store=q == 0, context=ctx1)
    for i in rest:
        assert full[i].any()
        assert bytes(out[i]) == bytes(full[i]) and bytes(junk[i]) == bytes(full[i])
    # the batch mirror: a status per stripe, stripes of different sizes
    d2, f2, t2 = _stripe(k, m, 17, e, ((0, 1, 2, 3),), 6)
    outs = [[bytearray(S) if i in rest else None for i in range(n)],
            [bytearray(17) if i in rest else None for i in range(n)],
            [bytearray(S) if i in rest else None for i in range(n)]]
    ins = [[bytes(data[e.index(i)]) if i in e else None for i in range(n)],
           [bytes(d2[e.index(i)]) if i in e else None for i in range(n)],
           [bytes(data[e.index(i)]) if i in e else None for i in range(n)]]
    st = E.decode_idx_batch(outs, [flags, flags, [i in e[:3] for i in range(n)]], ins, k, m, context=ctx1)
    assert st == [RS_OK, RS_OK, RS_E_TOO_FEW_SHARDS]
    for i in rest:
        assert bytes(outs[0][i]) == bytes(full[i]) and bytes(outs[1][i]) == bytes(f2[i])
        assert bytes(outs[2][i]) == bytes(S)
    with pytest.raises(ValueError):
        E.decode_idx_batch(outs, [flags], ins, k, m, context=ctx1)
