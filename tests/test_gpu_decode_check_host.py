"""DecodeCheck on host memory: rs_decode_check, rs_decode_check_batch and their
Python mirrors, against the oracle and against decode-check device plans over the same bytes.
Expected bytes come from oracle.cref alone: the implied shards are cref.reconstruct with present =
expect over the shards as they are (damage included), a syndrome is implied ^ actual, and a partial
feed's terms are cref.apply(C[:, delivered], inputs), with C from cref.reconstruct of the unit
vectors. Inputs, the bytes behind every buffer and, in a final call, the accumulators must stay
what they were."""
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
RS_OK, RS_E_TOO_FEW_SHARDS, RS_E_NO_DATA, RS_E_CORRUPT, RS_E_ARG = 0, -3, -5, -6, -10
STORE, FINAL = 1, 2
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
    """First k, last k, and a set that mixes data and parity."""
    n = k + m
    return [tuple(range(k)), tuple(range(n - k, n)), tuple(sorted(set(range(n)) - set(range(1, 1 + m))))][b % 3]


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
def _stripe(k, m, S, expect, damage, seed):
    """(actual [n][S]: a codeword with the damage (shard, offset, xor value) applied; implied
    [n][S]: cref.reconstruct from the expected shards of `actual`)."""
    rng = np.random.default_rng(seed)
    data = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
    actual = np.stack(data + cref.encode(data, k, m))
    for shard, off, val in damage:
        actual[shard, off] ^= val
    n = k + m
    implied = np.stack(cref.reconstruct([actual[i] if i in expect else None for i in range(n)],
                                        [i in expect for i in range(n)], k, m))
    actual.setflags(write=False)
    implied.setflags(write=False)
    return actual, implied


def _terms(k, m, expect, actual, rows, compared, deliver):
    """{row: what a call delivering the shards `deliver` computes for the row}."""
    C = _coef(k, m, expect)
    pos = [j for j, v in enumerate(expect) if v in deliver]
    S = actual.shape[1]
    t = cref.apply(C[list(rows)][:, pos], [actual[expect[j]] for j in pos]) if pos else [np.zeros(S, np.uint8)
                                                                                           for _ in rows]
    out = dict(zip(rows, t))
    for j in compared:
        if j in deliver:
            out[j] = out[j] ^ actual[j]
    return out


def _buf(src):
    """A writable copy of `src` with SENT bytes of 0xA5 behind it."""
    a = np.empty(len(src) + SENT, np.uint8)
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


def _split3(k, seed):
    perm = [int(i) for i in np.random.default_rng(seed).permutation(k)]
    cuts = [round(q * k / 3) for q in range(4)]
    return [sorted(perm[cuts[q]:cuts[q + 1]]) for q in range(3)]


def _plan_feed(k, m, S, expect, wanted, compared, calls, actual, start):
    """The same calls through decode-check device plans over device copies of the same bytes: the
    rows' final bytes and whether the final launch flagged the stripe."""
    import torch
    from callfs_amd.device import Plan
    n = k + m
    dev = torch.device("cuda:0")
    t = {i: torch.from_numpy(np.array(actual[i])).to(dev) for i in list(expect) + list(compared)}
    d = {r: torch.from_numpy(np.array(start[r])).to(dev) for r in list(wanted) + list(compared)}
    bad = False
    for deliver, store, final in calls:
        plan = Plan.decode_check(k, m, [S], [[i in expect for i in range(n)]],
                                 [t[i].data_ptr() if i in deliver else 0 for i in range(n)],
                                 [d[i].data_ptr() if i in wanted else 0 for i in range(n)],
                                 [d[i].data_ptr() if i in compared else 0 for i in range(n)], store=store, final=final)
        plan.launch()
        bad = plan.corrupt()
        plan.close()
    return {r: d[r].cpu().numpy() for r in d}, bad


@pytest.mark.parametrize("damage", ["clean", "compared", "expected"])
@pytest.mark.parametrize("S", [1, 17, 4096, 2 ** 20 + 1])
def test_three_calls_per_stripe(native_lib, ctx1, S, damage):
    """RS(10,4), an expected set that mixes data and parity, two wanted and two compared shards.
    Three calls deliver the expected shards in a shuffled split, the second one compared shard
    with it, the third (final) the other: merging from zeroed rows, and with the first call
    storing over junk. After every non-final call the rows hold the oracle's partial sums; the
    final call leaves the accumulators alone, completes the wanted shards and returns RS_E_CORRUPT
    exactly when a compared shard differs from what the expected shards imply; the device plans
    leave the same bytes and the same flag."""
    L = native_lib.lib
    k, m, n = 10, 4, 14
    expect = _expected(k, m, 2)
    rest = [i for i in range(n) if i not in expect]
    wanted, compared = tuple(rest[:2]), tuple(rest[2:])
    dmg = {"clean": (), "compared": ((compared[1], S - 1, 0x04),), "expected": ((expect[4], S // 2, 0x21),)}[damage]
    actual, implied = _stripe(k, m, S, expect, dmg, 1000 + S)
    differs = any(not np.array_equal(actual[j], implied[j]) for j in compared)
    assert differs == (damage != "clean")
    feeds = _split3(k, S + k)
    delivers = [{expect[j] for j in feeds[0]}, {expect[j] for j in feeds[1]} | {compared[0]},
                {expect[j] for j in feeds[2]} | {compared[1]}]
    rows = sorted(wanted + compared)
    ex = _u8([i in expect for i in range(n)])
    rng = np.random.default_rng(S)
    for store_first in (False, True):
        start = {r: rng.integers(0, 256, S, dtype=np.uint8) if store_first else np.zeros(S, np.uint8) for r in rows}
        buf = {r: _buf(start[r]) for r in rows}
        inputs = {i: _buf(actual[i]) for i in list(expect) + list(compared)}
        dst = [buf[i] if i in wanted else None for i in range(n)]
        chk = [buf[i] if i in compared else None for i in range(n)]
        now = dict(start)
        calls = [(delivers[q], store_first and q == 0, q == 2) for q in range(3)]
        for deliver, store, final in calls:
            t = _terms(k, m, expect, actual, rows, compared, deliver)
            want = {r: t[r] if store else now[r] ^ t[r] for r in rows}
            inp = [inputs[i] if i in deliver else None for i in range(n)]
            rc = L.rs_decode_check(ctx1.handle, k, m, S, _vp(dst), _vp(chk), ex, _vp(inp),
                                   (STORE if store else 0) | (FINAL if final else 0))
            if final:
                assert [bool(want[j].any()) for j in compared] == [not np.array_equal(actual[j], implied[j])
                                                                   for j in compared]
                assert rc == (RS_E_CORRUPT if differs else RS_OK)
                want = {r: want[r] if r in wanted else now[r] for r in rows}
            else:
                assert rc == RS_OK
            _intact([buf[r] for r in rows], [want[r] for r in rows])
            now = want
        _intact([buf[w] for w in wanted], [implied[w] for w in wanted])
        _intact([inputs[i] for i in inputs], [actual[i] for i in inputs])
        dev, flagged = _plan_feed(k, m, S, expect, wanted, compared, calls, actual, start)
        assert flagged == differs
        for r in rows:
            assert np.array_equal(dev[r], buf[r][:S]), r


def _batch(k, m, sizes, seed, damaged=()):
    """Per stripe its own expected set, wanted set (two, one, none of the rest) and compared set
    (two, one of the rest); stripes in `damaged` carry one flipped byte in a compared shard."""
    n = k + m
    out = []
    for b, S in enumerate(sizes):
        e = _expected(k, m, b)
        rest = [i for i in range(n) if i not in e]
        compared = tuple(rest[len(rest) - (2 - b % 2):])
        wanted = tuple([i for i in rest if i not in compared][:(2, 1, 0)[b % 3]])
        dmg = ((compared[0], S // 3, 1 + b % 200),) if b in damaged else ()
        actual, implied = _stripe(k, m, S, e, dmg, seed + b)
        out.append((e, wanted, compared, actual, implied))
    return out


@pytest.mark.parametrize("bits", [0, STORE, FINAL, FINAL | STORE], ids=["merge", "store", "final-merge", "final-store"])
def test_batch_is_one_round_trip(native_lib, ctx1, bits):
    """64 stripes of sizes 1..40,000 with their own expected, wanted and compared sets, everything
    delivered in one call: one launch per chunk (the 16 staged rows of 1.3 MB each pass the chunk
    budget once), a status per stripe -- RS_E_CORRUPT under FINAL for the damaged stripes alone.
    `copies` is what DESIGN.md §5.15 states for every kind of chunk: 2 for a store chunk, 3 for a
    merge chunk, final or not."""
    L = native_lib.lib
    k, m, n = 10, 4, 14
    sizes = tuple(1 + 634 * b for b in range(64))
    B = len(sizes)
    damaged = (3, 20, 41, 63)
    store, final = bool(bits & STORE), bool(bits & FINAL)
    st = _batch(k, m, sizes, 7, damaged)
    deltas = []
    for attempt in ("warm", "measured"):  # the tables are on the lane after the first call
        rng = np.random.default_rng(5)
        inputs, dst, chk, ex, start = [], [], [], [], []
        for b, (e, wanted, compared, actual, implied) in enumerate(st):
            S = sizes[b]
            rows = {r: rng.integers(0, 256, S, dtype=np.uint8) for r in wanted + compared}
            if final and not store:  # a final merge tests accumulator ^ terms: the accumulators start at zero
                rows.update({j: np.zeros(S, np.uint8) for j in compared})
            start.append(rows)
            bufs = {r: _buf(rows[r]) for r in rows}
            inputs += [_buf(actual[i]) if i in e or i in compared else None for i in range(n)]
            dst += [bufs[i] if i in wanted else None for i in range(n)]
            chk += [bufs[i] if i in compared else None for i in range(n)]
            ex += [i in e for i in range(n)]
        szs = (ctypes.c_size_t * B)(*sizes)
        # stripe 5 expects one shard too few; stripe 7 has size 0
        ex[5 * n + st[5][0][9]] = False
        szs[7] = 0
        status = (ctypes.c_int * B)(*([99] * B))
        c0 = _counters(native_lib, ctx1)
        rc = L.rs_decode_check_batch(ctx1.handle, k, m, B, szs, _vp(dst), _vp(chk), _u8(ex), _vp(inputs), bits, status)
        d = _delta(c0, _counters(native_lib, ctx1))
        deltas.append(d)
        want_status = [RS_E_TOO_FEW_SHARDS if b == 5 else RS_E_NO_DATA if b == 7 else
                       RS_E_CORRUPT if final and b in damaged else RS_OK for b in range(B)]
        assert list(status) == want_status
        assert rc == next(s for s in want_status if s)  # the first nonzero status in stripe order
        assert d["calls"] == 1 and 1 <= d["chunks"] <= 2 and d["launches"] == d["chunks"], d
        assert d["ragged_calls"] == 1, d
        for b, (e, wanted, compared, actual, implied) in enumerate(st):
            S = sizes[b]
            for i in range(n):
                a = inputs[b * n + i]
                if a is not None:
                    _intact([a], [actual[i]])
                row = dst[b * n + i] if dst[b * n + i] is not None else chk[b * n + i]
                if row is None:
                    continue
                if b in (5, 7) or (final and i in compared):
                    want = start[b][i]
                else:
                    full = implied[i] if i in wanted else implied[i] ^ actual[i]
                    want = full if store else start[b][i] ^ full
                _intact([row], [want])
    assert deltas[1]["copies"] == (2 if store else 3) * deltas[1]["chunks"], deltas


def test_nothing_to_do_moves_no_counter(native_lib, ctx1):
    L = native_lib.lib
    k, m, S, n = 10, 4, 4096, 14
    e = _expected(k, m, 2)
    rest = [i for i in range(n) if i not in e]
    actual, implied = _stripe(k, m, S, e, (), 3)
    rng = np.random.default_rng(1)
    start = {i: rng.integers(0, 256, S, dtype=np.uint8) for i in rest}
    dst = [_buf(start[i]) if i in rest[:2] else None for i in range(n)]
    chk = [_buf(start[i]) if i in rest[2:] else None for i in range(n)]
    inp = [_buf(actual[i]) if i in e else None for i in range(n)]
    none = [None] * n
    ex = _u8([i in e for i in range(n)])
    c0 = _counters(native_lib, ctx1)
    for bits in (0, STORE, FINAL, FINAL | STORE):
        if not bits & FINAL:  # (a final call scans the accumulators)
            assert L.rs_decode_check(ctx1.handle, k, m, S, _vp(dst), _vp(chk), ex, _vp(none), bits) == RS_OK
        assert L.rs_decode_check(ctx1.handle, k, m, S, _vp(dst), _vp(none), ex, _vp(none), bits) == RS_OK
        assert L.rs_decode_check(ctx1.handle, k, m, S, _vp(none), _vp(none), ex, _vp(inp), bits) == RS_OK  # no row
        status = (ctypes.c_int * 2)(9, 9)
        assert L.rs_decode_check_batch(ctx1.handle, k, m, 2, (ctypes.c_size_t * 2)(S, 0), _vp(dst + none),
                                       _vp(none + none), _u8([i in e for i in range(n)] * 2), _vp(none + inp), bits,
                                       status) == RS_OK
        assert list(status) == [RS_OK, RS_OK]
    assert L.rs_decode_check_batch(ctx1.handle, k, m, 0, None, None, None, None, None, 0, None) == RS_OK
    assert _delta(c0, _counters(native_lib, ctx1)) == {name: 0 for name in c0}
    _intact([b for b in dst + chk if b is not None], [start[i] for i in rest])


_CUTS_CHILD = r"""
import ctypes, sys
import numpy as np
from oracle import cref
from callfs_amd import _native as N

k, m, S, B = 4, 2, 300_000, 3
n = k + m
expect, wanted, compared = (0, 2, 4, 5), (1,), (3,)
rng = np.random.default_rng(8)
actual, implied = [], []
for b in range(B):
    data = [rng.integers(1, 256, S, dtype=np.uint8) for _ in range(k)]
    full = np.stack(data + cref.encode(data, k, m))
    if b == 1:
        full[3, 250_000] ^= 0x10   # one byte of the compared shard, in a late column part
    actual.append(full)
    implied.append(np.stack(cref.reconstruct([full[i] if i in expect else None for i in range(n)],
                                             [i in expect for i in range(n)], k, m)))
assert [np.array_equal(actual[b][3], implied[b][3]) for b in range(B)] == [True, False, True]
ctx = N.Context(1)
vp = lambda rows: (ctypes.c_void_p * len(rows))(*[None if r is None else r.ctypes.data for r in rows])
ex = (ctypes.c_uint8 * (B * n))(*[1 if i in expect else 0 for i in range(n)] * B)
szs = (ctypes.c_size_t * B)(*[S] * B)
ok = True


def call(dst, acc, deliver, bits):
    st = (ctypes.c_int * B)(9, 9, 9)
    c0, c1 = N.HostCounters(), N.HostCounters()
    N.lib.rs_host_counters_read(ctx.handle, ctypes.byref(c0))
    rc = N.lib.rs_decode_check_batch(ctx.handle, k, m, B, szs,
                                     vp([dst[b] if i in wanted else None for b in range(B) for i in range(n)]),
                                     vp([acc[b] if i in compared else None for b in range(B) for i in range(n)]), ex,
                                     vp([actual[b][i] if i in deliver else None for b in range(B) for i in range(n)]),
                                     bits, st)
    N.lib.rs_host_counters_read(ctx.handle, ctypes.byref(c1))
    return rc, list(st), c1.chunks - c0.chunks


# the one-shot decode plus Verify, over junk
dst = [implied[b][1] ^ 0xFF for b in range(B)]
acc = [np.full(S, 0x77, np.uint8) for b in range(B)]
rc, st, chunks = call(dst, acc, expect + compared, 3)
good = rc == -6 and st == [0, -6, 0] and chunks >= 3
good = good and all(np.array_equal(dst[b], implied[b][1]) and (acc[b] == 0x77).all() for b in range(B))
if not good:
    print("one-shot: rc=%d status=%r chunks=%d" % (rc, st, chunks))
ok = ok and good
# merged in two calls, then a final call with nothing delivered
dst = [np.zeros(S, np.uint8) for b in range(B)]
acc = [np.zeros(S, np.uint8) for b in range(B)]
rc1, st1, _ = call(dst, acc, (0, 2, 3), 0)
rc2, st2, _ = call(dst, acc, (4, 5), 0)
synd = [actual[b][3] ^ implied[b][3] for b in range(B)]
good = rc1 == 0 and rc2 == 0 and st1 == st2 == [0, 0, 0]
good = good and all(np.array_equal(acc[b], synd[b]) and np.array_equal(dst[b], implied[b][1]) for b in range(B))
rc3, st3, chunks = call(dst, acc, (), 2)
good = good and rc3 == -6 and st3 == [0, -6, 0] and chunks >= 2
good = good and all(np.array_equal(acc[b], synd[b]) and np.array_equal(dst[b], implied[b][1]) for b in range(B))
if not good:
    print("merged: rc=%d,%d,%d status=%r chunks=%d" % (rc1, rc2, rc3, st3, chunks))
ok = ok and good
print("column cuts child:", "ok" if ok else "failed")
ctx.close()
sys.exit(0 if ok else 1)
"""


def test_corrupt_byte_in_a_column_cut_stripe(native_lib):
    """CALLFS_RS_CHUNK_BYTES is read once per process: in a fresh child, under a 256 KiB chunk
    budget, three 300,000-byte stripes are cut into column parts; one corrupt byte in a late part
    of stripe 1 gives RS_E_CORRUPT for that stripe alone, in the one-shot form and when a final
    call with nothing delivered scans accumulators that earlier calls merged."""
    env = dict(os.environ)
    env["CALLFS_RS_CHUNK_BYTES"] = str(256 << 10)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _CUTS_CHILD], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "column cuts child: ok" in r.stdout


def test_errors_and_python_mirror(native_lib, ctx1):
    from callfs_amd import erasure as E
    N = native_lib
    k, m, n, S = 4, 2, 6, 1000
    expect = (0, 1, 3, 5)
    flags = [i in expect for i in range(n)]
    actual, implied = _stripe(k, m, S, expect, (), 12)
    damaged, _ = _stripe(k, m, S, expect, ((4, 999, 0x80),), 12)
    inputs = [np.array(actual[i]) if i in expect or i == 4 else None for i in range(n)]
    none = [None] * n

    def rows():
        return [np.zeros(S, np.uint8) if i == 2 else None for i in range(n)], \
               [np.zeros(S, np.uint8) if i == 4 else None for i in range(n)]

    # two calls, the second final; then the same with the compared shard damaged
    for shard4, raises in ((actual[4], False), (damaged[4], True)):
        dst, chk = rows()
        first = [inputs[i] if i in (0, 5) else None for i in range(n)]
        second = [np.array(shard4) if i == 4 else inputs[i] if i in (1, 3) else None for i in range(n)]
        E.decode_check(dst, chk, flags, first, k, m, context=ctx1)
        acc = chk[4].copy()
        if raises:
            with pytest.raises(E.ErrShardCorrupted):
                E.decode_check(dst, chk, flags, second, k, m, final=True, context=ctx1)
        else:
            E.decode_check(dst, chk, flags, second, k, m, final=True, context=ctx1)
        assert np.array_equal(dst[2], implied[2]) and np.array_equal(chk[4], acc)
    # the one-shot form never reads the accumulator
    dst, chk = rows()
    chk[4][:] = 0x33
    E.decode_check(dst, chk, flags, inputs, k, m, store=True, final=True, context=ctx1)
    assert np.array_equal(dst[2], implied[2]) and (chk[4] == 0x33).all()
    # the batch form: a status per stripe
    d0, c0 = rows()
    d1, c1 = rows()
    bad_in = [np.array(damaged[4]) if i == 4 else inputs[i] for i in range(n)]
    st = E.decode_check_batch([d0, d1, none], [c0, c1, none], [flags, flags, flags[:3] + [False] * 3],
                              [inputs, bad_in, none], k, m, store=True, final=True, context=ctx1)
    assert st == [N.RS_OK, N.RS_E_CORRUPT, N.RS_E_TOO_FEW_SHARDS]
    assert np.array_equal(d0[2], implied[2]) and np.array_equal(d1[2], implied[2])
    # errors
    dst, chk = rows()
    with pytest.raises(E.ErrInvalidInput):  # a check and a dst at one index
        E.decode_check(dst, [dst[i] for i in range(n)], flags, inputs, k, m, context=ctx1)
    with pytest.raises(E.ErrInvalidInput):  # an input that is neither expected nor compared
        E.decode_check(dst, none, flags, inputs, k, m, context=ctx1)
    with pytest.raises(E.ErrInvalidInput):  # a check at an expected index
        E.decode_check(dst, [np.zeros(S, np.uint8) if i == 0 else None for i in range(n)], flags, none, k, m,
                       context=ctx1)
    with pytest.raises(E.ErrTooFewShards):
        E.decode_check(dst, chk, flags[:3] + [False] * 3, none, k, m, context=ctx1)
    with pytest.raises(E.ErrTooFewShards):
        E.decode_check(dst, chk[:-1], flags, inputs, k, m, context=ctx1)
    with pytest.raises(E.ErrShardSize):
        E.decode_check(dst, [np.zeros(S + 1, np.uint8) if i == 4 else None for i in range(n)], flags, inputs, k, m,
                       context=ctx1)
    with pytest.raises(E.ErrInvalidProfile):
        E.decode_check([None] * 4, [None] * 4, [True] * 4, [None] * 4, 4, 0, context=ctx1)
    L = N.lib
    ex = _u8(flags)
    for bits in (4, 8, 1 << 31):
        assert L.rs_decode_check(ctx1.handle, k, m, S, _vp(dst), _vp(chk), ex, _vp(inputs), bits) == RS_E_ARG
    assert L.rs_decode_check(ctx1.handle, k, m, S, _vp(dst), None, ex, _vp(inputs), 0) == RS_E_ARG
    assert L.rs_decode_check(ctx1.handle, k, m, 0, _vp(dst), _vp(chk), ex, _vp(inputs), 0) == RS_E_NO_DATA
    assert L.rs_decode_check(ctx1.handle, k, m, 0, _vp(none), _vp(chk), ex, _vp(none), FINAL) == RS_E_NO_DATA
    assert L.rs_decode_check(ctx1.handle, k, m, 0, _vp(none), _vp(chk), ex, _vp(none), 0) == RS_OK
