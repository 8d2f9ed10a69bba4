"""DecodeRepair on host memory: rs_decode_repair, rs_decode_repair_batch and
their Python mirror. Expected bytes come from the C oracle alone, as in
test_gpu_decode_check_host.py, whose helpers this file uses: a true codeword from cref.encode,
chosen bytes of the delivered shards damaged; repaired wanted shards are the true shards, a zeroed
fix buffer ends as damaged ^ true, a fix buffer holding the shard as delivered ends as the true
shard, counts are the columns the test changed. Every buffer has a sentinel tail, and every
buffer the rule may not write is compared with what it held."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref

import test_gpu_decode_check_host as H

pytestmark = pytest.mark.gpu

ROOT = H.ROOT
RS_OK, RS_E_TOO_FEW_SHARDS, RS_E_NO_DATA, RS_E_CORRUPT, RS_E_UNSUPPORTED, RS_E_ARG = 0, -3, -5, -6, -8, -10
STORE = 1
ctx1 = H.ctx1


def _sets(k, m, b, nchk=3, nwant=1):
    e = H._expected(k, m, b)
    rest = [i for i in range(k + m) if i not in e]
    rest = rest[b % len(rest):] + rest[:b % len(rest)]
    return e, tuple(sorted(rest[nchk:nchk + nwant])), tuple(sorted(rest[:nchk]))


class _Stripe:
    """One stripe's host buffers: the damaged codeword's expected and compared shards, junk in
    the wanted shards, zeroed accumulators, and fix buffers (mode "zero", "delivered", "alias":
    the delivered shard itself, or "null")."""

    def __init__(self, k, m, S, b, damage, seed, fix="zero", nchk=3, nwant=1):
        self.k, self.m, self.n, self.S = k, m, k + m, S
        self.expect, self.wanted, self.compared = _sets(k, m, b, nchk, nwant)
        self.damage = tuple(damage)
        self.actual, self.implied = H._stripe(k, m, S, self.expect, self.damage, seed)
        self.truth = self.actual.copy()
        for shard, off, val in self.damage:
            self.truth[shard, off] ^= val
        rng = np.random.default_rng(seed + 7)
        n = self.n
        given = set(self.expect) | set(self.compared)
        self.shards = [H._buf(self.actual[i]) if i in given else None for i in range(n)]
        self.junk = {w: rng.integers(0, 256, S, dtype=np.uint8) for w in self.wanted}
        self.dst = [H._buf(self.junk[i]) if i in self.wanted else None for i in range(n)]
        self.acc = [H._buf(np.zeros(S, np.uint8)) if i in self.compared else None for i in range(n)]
        self.fixmode = fix
        if fix == "zero":
            self.fix = [H._buf(np.zeros(S, np.uint8)) if i in given else None for i in range(n)]
        elif fix == "delivered":
            self.fix = [H._buf(self.actual[i]) if i in given else None for i in range(n)]
        elif fix == "alias":
            self.fix = list(self.shards)
        else:
            self.fix = [None] * n
        cols = {}
        for shard, off, _ in self.damage:
            cols.setdefault(off, set()).add(shard)
        self.blamed = {off: next(iter(s)) for off, s in cols.items() if len(s) == 1 and nchk >= 3}
        self.unexplained = sorted(set(cols) - set(self.blamed))
        for off, s in cols.items():
            assert off in self.blamed or nchk < 3 or 2 <= len(s) < nchk
        self.counts = [0] * (n + 1)
        for shard in self.blamed.values():
            self.counts[shard] += 1
        self.counts[n] = len(self.unexplained)

    def inputs(self, deliver):
        return [self.shards[i] if i in deliver else None for i in range(self.n)]

    def everything(self):
        return set(self.expect) | set(self.compared)

    def status(self):
        return RS_E_CORRUPT if self.unexplained else RS_OK

    def check_after(self, counts=None):
        """Every buffer after a complete feed that ended in the repair call."""
        S, n = self.S, self.n
        tail = lambda a: (a[S:] == 0xA5).all()  # noqa: E731
        for w in self.wanted:
            row = self.truth[w].copy()
            row[self.unexplained] = self.implied[w][self.unexplained]
            assert np.array_equal(self.dst[w][:S], row) and tail(self.dst[w]), w
        err = self.actual ^ self.truth
        for i in range(n):
            hit = [off for off, s in self.blamed.items() if s == i]
            if self.shards[i] is not None:
                want = self.actual[i].copy()
                if self.fixmode == "alias":
                    want[hit] = self.truth[i][hit]
                assert np.array_equal(self.shards[i][:S], want) and tail(self.shards[i]), i
            if self.fix[i] is not None and self.fixmode in ("zero", "delivered"):
                want = np.zeros(S, np.uint8) if self.fixmode == "zero" else self.actual[i].copy()
                want[hit] ^= err[i][hit]
                assert np.array_equal(self.fix[i][:S], want) and tail(self.fix[i]), i
        if counts is not None:
            assert [int(c) for c in counts] == self.counts


def _call(Nat, ctx, st, deliver, store, counts=True):
    """rs_decode_repair on one stripe; returns (rc, counts)."""
    cn = (ctypes.c_uint64 * (st.n + 1))(*([7] * (st.n + 1)))
    rc = Nat.lib.rs_decode_repair(ctx.handle, st.k, st.m, st.S, H._vp(st.dst), H._vp(st.acc), H._vp(st.fix),
                                  H._u8([i in st.expect for i in range(st.n)]), H._vp(st.inputs(deliver)),
                                  STORE if store else 0, cn if counts else None)
    return rc, list(cn)


def _feed(Nat, ctx, st, deliver):
    """A non-final rs_decode_check merge call."""
    rc = Nat.lib.rs_decode_check(ctx.handle, st.k, st.m, st.S, H._vp(st.dst), H._vp(st.acc),
                                 H._u8([i in st.expect for i in range(st.n)]), H._vp(st.inputs(deliver)), 0)
    assert rc == RS_OK


def _damage(kind, S, e, c):
    if kind == "clean":
        return ()
    if kind == "expected":
        return ((e[3 % len(e)], S // 2, 0x81),)
    if kind == "compared":
        return ((c[1], S - 1, 0x17),)
    if kind == "two-shards":
        return ((e[0], 0, 1), (c[2], S - 1, 2)) if S > 1 else ((e[0], 0, 1),)
    assert kind == "same-column"
    return ((e[1], S // 3, 0x21), (c[0], S // 3, 0x42))


@pytest.mark.parametrize("fix", ["null", "zero", "delivered", "alias"])
@pytest.mark.parametrize("damage", ["clean", "expected", "compared", "two-shards", "same-column"])
@pytest.mark.parametrize("S", [1, 17, 4096, 2 ** 20 + 1])
def test_per_stripe_against_the_oracle_and_the_device_plan(native_lib, ctx1, S, damage, fix):
    """rs_decode_repair per stripe, RS(10,4) with three compared and one wanted shard: in one
    store call over junk, and as two decode-check merge calls from zero with the repair call
    last. Wanted shards, fix buffers, inputs, counts and the return value against the oracle; the
    wanted shard and the counts also against Plan.decode_repair over device copies."""
    import torch
    from callfs_amd.device import Plan
    k, m = 10, 4
    b = S % 3
    for store in (True, False):
        e, w, c = _sets(k, m, b)
        st = _Stripe(k, m, S, b, _damage(damage, S, e, c), seed=S % 1000 + 3, fix=fix)
        if store:
            last = st.everything()
        else:
            for z in st.acc:
                assert z is None or not z[:S].any()
            for wi in st.wanted:
                st.dst[wi][:S] = 0
            third = sorted(st.everything())
            _feed(native_lib, ctx1, st, set(third[0::3]))
            _feed(native_lib, ctx1, st, set(third[1::3]))
            last = set(third[2::3])
            # the shards the repair call no longer sees may be fixed all the same (alias mode)
        acc_before = [None if a is None else a.copy() for a in st.acc]
        rc, counts = _call(native_lib, ctx1, st, last, store)
        assert rc == st.status()
        st.check_after(counts)
        for a, a0 in zip(st.acc, acc_before):  # a check row is never written
            assert a is None or np.array_equal(a, a0)
        if store and S <= 4096:
            dev = torch.device("cuda:0")
            d = torch.from_numpy(np.stack([st.actual[i] for i in range(st.n)])).to(dev)
            out = torch.zeros(S, dtype=torch.uint8, device=dev)
            ptr = lambda i: d[i].data_ptr()  # noqa: E731
            plan = Plan.decode_repair(k, m, [S], [[i in st.expect for i in range(st.n)]],
                                      [ptr(i) if i in last else 0 for i in range(st.n)],
                                      [out.data_ptr() if i in st.wanted else 0 for i in range(st.n)],
                                      [ptr(i) if i in st.compared else 0 for i in range(st.n)], store=True)
            plan.launch()
            assert bool(plan.corrupt_stripes()) == bool(st.damage)
            assert [int(x) for x in plan.blame()[0]] == counts
            assert np.array_equal(out.cpu().numpy(), st.dst[st.wanted[0]][:S])
            plan.close()


def test_batch_of_64_in_one_call(native_lib, ctx1):
    """64 stripes of sizes 1..40,000, every stripe its own sets, every fourth clean, in one call.
    `copies` shows that no fix row went up (4 per store chunk: metadata and inputs, the fix
    pointer table, the rows back, the counts back) and that only the blamed fix rows came back,
    one copy each."""
    k, m = 10, 4
    rng = np.random.default_rng(64)
    sizes = [1, 40_000] + [int(x) for x in rng.integers(2, 40_000, 62)]
    n = k + m
    flat = lambda rows: [x for r in rows for x in r]  # noqa: E731
    for attempt in range(2):  # the first call uploads the run's tables into the lane's cache: one more copy
        sts = []
        for b, S in enumerate(sizes):
            e, w, c = _sets(k, m, b)
            kind = ["expected", "compared", "two-shards", "clean"][b % 4]
            if b % 16 == 6:
                kind = "same-column"
            sts.append(_Stripe(k, m, S, b, _damage(kind, S, e, c), seed=b, fix="zero"))
        status = (ctypes.c_int * 64)(*([5] * 64))
        counts = (ctypes.c_uint64 * (64 * (n + 1)))()
        c0 = H._counters(native_lib, ctx1)
        rc = native_lib.lib.rs_decode_repair_batch(
            ctx1.handle, k, m, 64, (ctypes.c_size_t * 64)(*sizes), H._vp(flat(s.dst for s in sts)),
            H._vp(flat(s.acc for s in sts)), H._vp(flat(s.fix for s in sts)),
            H._u8(flat([i in s.expect for i in range(n)] for s in sts)),
            H._vp(flat(s.inputs(s.everything()) for s in sts)), STORE, status, counts)
        d = H._delta(c0, H._counters(native_lib, ctx1))
    want = [s.status() for s in sts]
    assert list(status) == want and rc == next((x for x in want if x), RS_OK)
    assert RS_E_CORRUPT in want and want.count(RS_OK) > 48
    for b, s in enumerate(sts):
        s.check_after(counts[b * (n + 1):(b + 1) * (n + 1)])
    blamed_rows = sum(len(set(s.blamed.values())) for s in sts)
    assert blamed_rows > 40
    assert d["calls"] == 1 and 1 <= d["chunks"] == d["launches"] <= 4, d
    assert d["copies"] == 4 * d["chunks"] + blamed_rows, d


def test_nothing_to_do_moves_no_counter(native_lib, ctx1):
    k, m, n = 4, 2, 6
    L = native_lib.lib
    c0 = H._counters(native_lib, ctx1)
    assert L.rs_decode_repair_batch(ctx1.handle, k, m, 0, None, None, None, None, None, None, 0, None, None) == RS_OK
    st = _Stripe(k, m, 64, 0, (), seed=1, fix="zero", nchk=2, nwant=0)
    # a wanted shard alone and nothing delivered: in no launch
    dst = [None] * n
    dst[st.compared[0]] = H._buf(np.zeros(64, np.uint8))
    none = H._vp([None] * n)
    cn = (ctypes.c_uint64 * (n + 1))(*([9] * (n + 1)))
    assert L.rs_decode_repair(ctx1.handle, k, m, 64, H._vp(dst), none, none, H._u8([i in st.expect for i in range(n)]),
                              none, 0, cn) == RS_OK
    assert list(cn) == [0] * (n + 1) and not dst[st.compared[0]][:64].any()
    assert H._delta(c0, H._counters(native_lib, ctx1)) == {name: 0 for name in c0}


_CUTS_CHILD = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, "tests")
import test_gpu_decode_repair_host as T
from callfs_amd import _native as N

k, m = 10, 4
S = 2 ** 20 + 1                      # 14 rows of 1 MiB under a 256 KiB budget: many column parts
ctx = N.Context(1)
ok = True
for store in (True, False):
    e, w, c = T._sets(k, m, 2)
    damage = ((e[0], 0, 1), (e[4], 8191, 2), (c[1], 8192, 3), (e[9], 500_000, 4), (c[0], S - 1, 5),
              (e[2], 700_000, 6), (c[2], 700_000, 7))
    st = T._Stripe(k, m, S, 2, damage, seed=11, fix="zero")
    if not store:
        for wi in st.wanted:
            st.dst[wi][:S] = 0
        T._feed(N, ctx, st, set(st.expect[:6]))
    last = st.everything() if store else st.everything() - set(st.expect[:6])
    warm = T._Stripe(k, m, S, 2, (), seed=12, fix="null")   # the run's tables into the lane's cache
    assert T._call(N, ctx, warm, last, store)[0] == (T.RS_OK if store else T.RS_E_CORRUPT)
    c0 = N.HostCounters(); N.lib.rs_host_counters_read(ctx.handle, ctypes.byref(c0))
    rc, counts = T._call(N, ctx, st, last, store)
    c1 = N.HostCounters(); N.lib.rs_host_counters_read(ctx.handle, ctypes.byref(c1))
    chunks = c1.chunks - c0.chunks
    copies = c1.copies - c0.copies
    assert rc == T.RS_E_CORRUPT, rc               # column 700,000 is unexplained; the rest is repaired
    st.check_after(counts)
    assert chunks > 8, chunks
    assert copies == (4 if store else 5) * chunks + 5, (copies, chunks)   # five blamed (part, shard) rows
print("decode-repair cuts child: ok")
"""


def test_damaged_column_cut_stripe(native_lib):
    """CALLFS_RS_CHUNK_BYTES is read once per process: in a fresh child, under a 256 KiB chunk
    budget, a stripe of 2^20 + 1 bytes is cut into column parts; damage in the first part, on
    both sides of a tile edge, in the middle and in the tail is repaired, counts add over the
    parts, an unexplained column makes the stripe RS_E_CORRUPT."""
    env = dict(os.environ)
    env["CALLFS_RS_CHUNK_BYTES"] = str(256 << 10)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _CUTS_CHILD], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "decode-repair cuts child: ok" in r.stdout


def test_errors_and_python_mirror(native_lib, ctx1):
    """The call-level and per-stripe refusals in the header's order, and the Python mirror."""
    from callfs_amd import erasure
    L = native_lib.lib
    k, m, n = 10, 4, 14
    S = 100
    st = _Stripe(k, m, S, 0, (), seed=5, fix="zero")
    ex = H._u8([i in st.expect for i in range(n)])
    every = st.inputs(st.everything())
    status = (ctypes.c_int * 1)()

    def batch(kk=k, mm=m, sizes=(S,), dst=st.dst, chk=st.acc, fix=st.fix, e=ex, inp=every, bits=0, null=()):
        a = {"sizes": (ctypes.c_size_t * 1)(*sizes), "dst": H._vp(dst), "chk": H._vp(chk), "fix": H._vp(fix), "e": e,
             "inp": H._vp(inp), "status": status}
        for name in null:
            a[name] = None
        rc = L.rs_decode_repair_batch(ctx1.handle, kk, mm, 1, a["sizes"], a["dst"], a["chk"], a["fix"], a["e"],
                                      a["inp"], bits, a["status"], None)
        return rc, status[0]

    assert batch(kk=0, null=("sizes",), bits=8)[0] == native_lib.RS_E_INVALID_PROFILE  # the profile first
    assert batch(kk=250, mm=10, null=("fix",))[0] == RS_E_UNSUPPORTED
    for name in ("sizes", "dst", "chk", "fix", "e", "inp", "status"):
        assert batch(null=(name,))[0] == RS_E_ARG, name
    for bits in (2, 3, 4, 1 << 31):
        assert batch(bits=bits)[0] == RS_E_ARG
    few = H._u8([i in st.expect[1:] for i in range(n)])
    fix_wanted = list(st.fix)
    fix_wanted[st.wanted[0]] = H._buf(np.zeros(S, np.uint8))
    in_wanted = list(every)
    in_wanted[st.wanted[0]] = H._buf(np.zeros(S, np.uint8))
    assert batch(e=few, fix=fix_wanted, sizes=(0,)) == (RS_E_TOO_FEW_SHARDS, RS_E_TOO_FEW_SHARDS)
    assert batch(fix=fix_wanted, sizes=(0,)) == (RS_E_ARG, RS_E_ARG)
    assert batch(inp=in_wanted, sizes=(0,)) == (RS_E_ARG, RS_E_ARG)
    assert batch(sizes=(0,)) == (RS_E_NO_DATA, RS_E_NO_DATA)
    assert batch(bits=STORE) == (RS_OK, RS_OK)
    # 17 rows: RS(10,20) with 9 wanted and 8 compared
    k2, m2, n2 = 10, 20, 30
    z = lambda: H._buf(np.zeros(16, np.uint8))  # noqa: E731
    dst = [z() if 10 <= i < 19 else None for i in range(n2)]
    chk = [z() if 19 <= i < 27 else None for i in range(n2)]
    inp = [z() if i < 10 else None for i in range(n2)]
    rc = L.rs_decode_repair(ctx1.handle, k2, m2, 16, H._vp(dst), H._vp(chk), H._vp([None] * n2),
                            H._u8([i < 10 for i in range(n2)]), H._vp(inp), STORE, None)
    assert rc == RS_E_UNSUPPORTED
    # the Python mirror: counts returned, ErrShardCorrupted on an unexplained column, its own errors
    e, w, c = _sets(k, m, 1)
    st = _Stripe(k, m, 4097, 1, _damage("two-shards", 4097, e, c), seed=8, fix="delivered")
    counts = erasure.decode_repair(st.dst, st.acc, st.fix, [i in st.expect for i in range(n)],
                                   st.inputs(st.everything()), k, m, store=True, context=ctx1)
    st.check_after(counts)
    bad = _Stripe(k, m, 4097, 1, _damage("same-column", 4097, e, c), seed=9, fix="zero")
    with pytest.raises(erasure.ErrShardCorrupted):
        erasure.decode_repair(bad.dst, bad.acc, bad.fix, [i in bad.expect for i in range(n)],
                              bad.inputs(bad.everything()), k, m, store=True, context=ctx1)
    bad.check_after()
    sts = [_Stripe(k, m, 300 + b, b, _damage(["expected", "clean", "same-column"][b], 300 + b, *_sets(k, m, b)[::2]),
                   seed=20 + b, fix="zero") for b in range(3)]
    status, cn = erasure.decode_repair_batch([s.dst for s in sts], [s.acc for s in sts], [s.fix for s in sts],
                                             [[i in s.expect for i in range(n)] for s in sts],
                                             [s.inputs(s.everything()) for s in sts], k, m, store=True, context=ctx1)
    assert status == [RS_OK, RS_OK, RS_E_CORRUPT]
    for s, c_ in zip(sts, cn):
        s.check_after(c_)
    with pytest.raises(erasure.ErrTooFewShards):
        erasure.decode_repair(st.dst, st.acc, st.fix[:-1], [i in st.expect for i in range(n)],
                              st.inputs(st.everything()), k, m, context=ctx1)
    with pytest.raises(erasure.ErrShardSize):
        short = list(st.fix)
        short[st.expect[0]] = np.zeros(5, np.uint8)
        erasure.decode_repair(st.dst, st.acc, short, [i in st.expect for i in range(n)],
                              st.inputs(st.everything()), k, m, context=ctx1)
    with pytest.raises(ValueError):
        erasure.decode_repair_batch([st.dst], [st.acc], [], [[True] * n], [every], k, m, context=ctx1)


def test_degraded_read_with_a_bad_sector(native_lib, ctx1):
    """The case that motivates the change: RS(10,4), data shard 3 missing, three extra shards
    fetched, a bad 4 KiB sector in survivor 7. erasure.decode_check ends in ErrShardCorrupted
    with wrong bytes in the rebuilt shard; erasure.decode_repair returns the true shard and names
    the survivor."""
    from callfs_amd import erasure
    k, m, n = 10, 4, 14
    S = 1 << 16
    rng = np.random.default_rng(2026)
    data = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
    truth = np.stack(data + cref.encode(data, k, m))
    delivered = truth.copy()
    delivered[7, 8192:12288] ^= rng.integers(1, 256, 4096, dtype=np.uint8)
    expect = [i != 3 and i < 11 for i in range(n)]           # ten survivors: 0-2, 4-10
    extra = (11, 12, 13)                                     # three more fetched

    def buffers():
        dst = [np.zeros(S, np.uint8) if i == 3 else None for i in range(n)]
        chk = [np.zeros(S, np.uint8) if i in extra else None for i in range(n)]
        inp = [delivered[i].copy() if i != 3 else None for i in range(n)]
        return dst, chk, inp

    dst, chk, inp = buffers()
    with pytest.raises(erasure.ErrShardCorrupted):
        erasure.decode_check(dst, chk, expect, inp, k, m, store=True, final=True, context=ctx1)
    assert not np.array_equal(dst[3], truth[3])               # built from the corrupt survivor
    dst, chk, inp = buffers()
    fix = [None] * n
    fix[7] = inp[7]                                           # repaired where it lies
    counts = erasure.decode_repair(dst, chk, fix, expect, inp, k, m, store=True, context=ctx1)
    assert np.array_equal(dst[3], truth[3])
    assert counts == [4096 if i == 7 else 0 for i in range(n + 1)]
    assert np.array_equal(inp[7], truth[7])
