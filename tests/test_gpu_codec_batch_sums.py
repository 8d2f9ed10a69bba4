"""Checksummed codec batches: rs_codec_encode_batch_sums returns every
shard's SHA-256 beside the shards, rs_codec_decode_batch_sums checks every present shard
against its expected digest, treats a mismatching shard as missing and heals it.

Every digest is compared with hashlib, every shard, object, length and status with the plain
calls (rs_codec_encode_batch / rs_codec_decode_batch) on copies of the same input; a decode
with a mismatch is compared with the plain decode of the same object with that shard's length
zero. The scenarios run in this process (CALLFS_RS_SUMS_DEVICE unset: `auto`) and again in
fresh child processes whose environment picks the route (the knobs are read once per process):
the host (=0) and the device (=1) for every whole-stripe item, and =1 with 64 KiB chunks, where
a 300,000-byte-shard object is cut into column parts and hashed on the host beside
device-hashed items of the same call. One scenario is a batch on which `auto` itself picks the
device (896 messages of a few hundred bytes), told by the launch counter. A child prints one
JSON line of named checks and of digests of everything the calls returned, which must be the
same on every route.

  python tests/test_gpu_codec_batch_sums.py child <route>     # what a child runs
"""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RS_OK, RS_E_SHORT, RS_E_TOO_FEW, RS_E_ARG = 0, -2, -3, -10
SENT = 64
EDGES = [1, 15, 16, 55, 56, 63, 64, 65, 119, 120, 128, 4099]  # shard sizes
BIG = 300000

ROUTES = {
    "host": {"CALLFS_RS_SUMS_DEVICE": "0", "CALLFS_RS_SMALL_MAX_BYTES": "0"},
    "device": {"CALLFS_RS_SUMS_DEVICE": "1", "CALLFS_RS_SMALL_MAX_BYTES": "0"},
    "chunked": {"CALLFS_RS_SUMS_DEVICE": "1", "CALLFS_RS_SMALL_MAX_BYTES": "0",
                "CALLFS_RS_CHUNK_BYTES": "65536"},
}


def _env():
    sys.path.insert(0, ROOT)
    from callfs_amd import _native as Nat
    from callfs_amd import erasure
    return Nat, erasure


def _sha(a):
    return hashlib.sha256(bytes(a)).digest()


def _guard(size, fill=0xA5):
    a = np.full(size + 2 * SENT, 0xA5, np.uint8)
    a[SENT:SENT + size] = fill
    return a


def _body(a):
    return a[SENT:len(a) - SENT]


def _sent_ok(a):
    return bool((a[:SENT] == 0xA5).all() and (a[len(a) - SENT:] == 0xA5).all())


def _ptrs(arrs):
    return (ctypes.c_void_p * max(len(arrs), 1))(*[0 if a is None else a.ctypes.data + SENT for a in arrs])


def _objects(k, sizes, seed):
    """One object per shard size S, its length alternately k*S (no pad) and k*(S-1)+1 (the
    most pad that still gives S)."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, k * S if j % 2 else k * (S - 1) + 1, dtype=np.uint8)
            for j, S in enumerate(sizes)]


def encode(Nat, cx, k, m, objs, sums):
    """rs_codec_encode_batch(_sums) over objs (an empty array is an empty object)."""
    n, B = k + m, len(objs)
    S = [-(-len(o) // k) for o in objs]
    data = [_guard(len(o), 0) for o in objs]
    for d, o in zip(data, objs):
        _body(d)[:] = o
    outs = [_guard(n * s, 0xCC) for s in S]
    lens = (ctypes.c_size_t * B)(*[len(o) for o in objs])
    caps = (ctypes.c_size_t * B)(*[n * s for s in S])
    sizes = (ctypes.c_size_t * B)(*([12345] * B))
    status = (ctypes.c_int * B)(*([99] * B))
    digests = _guard(B * n * 32, 0xEE)
    if sums:
        rc = Nat.lib.rs_codec_encode_batch_sums(cx.handle, k, m, B, _ptrs(data), lens, _ptrs(outs), caps,
                                                sizes, digests.ctypes.data + SENT, status)
    else:
        rc = Nat.lib.rs_codec_encode_batch(cx.handle, k, m, B, _ptrs(data), lens, _ptrs(outs), caps, sizes,
                                           status)
    guards = all(_sent_ok(a) for a in data + outs + [digests])
    return dict(rc=rc, status=list(status), sizes=list(sizes), S=S, shards=[_body(o).copy() for o in outs],
                digests=_body(digests).copy().reshape(B, n, 32), guards=guards)


def check_encode(Nat, cx, k, m, sizes, seed, empty_at=None):
    n = k + m
    objs = _objects(k, sizes, seed)
    if empty_at is not None:
        objs.insert(empty_at, np.zeros(0, np.uint8))
    plain = encode(Nat, cx, k, m, objs, False)
    got = encode(Nat, cx, k, m, objs, True)
    ok = {"guards": got["guards"] and plain["guards"],
          "rc": got["rc"] == plain["rc"] == (RS_E_SHORT if empty_at is not None else RS_OK),
          "status": got["status"] == plain["status"], "sizes": got["sizes"] == plain["sizes"]}
    ok["shards"] = all((a == b).all() for a, b in zip(got["shards"], plain["shards"]))
    dig, untouched = True, True
    for b, o in enumerate(objs):
        if len(o) == 0:
            untouched &= got["status"][b] == RS_E_SHORT and bool((got["digests"][b] == 0xEE).all())
            continue
        S = got["S"][b]
        for i in range(n):
            dig &= got["digests"][b, i].tobytes() == _sha(got["shards"][b][i * S:(i + 1) * S])
    ok["digests"], ok["untouched"] = dig, untouched
    return ok, got


class Stripes:
    """Objects of RS(k, m) as a decode call takes them: shard buffers (guarded), lens, expected
    digests, sizes; `orig` keeps the objects and the true shards."""

    def __init__(self, Nat, cx, k, m, sizes, seed):
        self.k, self.m, self.n = k, m, k + m
        self.objs = _objects(k, sizes, seed)
        enc = encode(Nat, cx, k, m, self.objs, False)  # the plain call: the true shards
        assert enc["rc"] == RS_OK
        self.S = enc["S"]
        self.true = [[e[i * s:(i + 1) * s].copy() for i in range(self.n)] for e, s in zip(enc["shards"], self.S)]
        self.bufs = [[_guard(s, 0) for _ in range(self.n)] for s in self.S]
        for b, row in enumerate(self.bufs):
            for i, a in enumerate(row):
                _body(a)[:] = self.true[b][i]
        self.lens = [[s] * self.n for s in self.S]
        self.expected = np.array([[np.frombuffer(_sha(t), np.uint8) for t in row] for row in self.true])

    def drop(self, b, i):
        self.lens[b][i] = 0
        _body(self.bufs[b][i])[:] = 0x5C

    def flip(self, b, i, byte):
        _body(self.bufs[b][i])[byte] ^= 0x40

    def clone(self):
        c = object.__new__(Stripes)
        c.__dict__.update(self.__dict__)
        c.bufs = [[a.copy() for a in row] for row in self.bufs]
        c.lens = [list(r) for r in self.lens]
        c.expected = self.expected.copy()
        return c


def decode(Nat, cx, st, sums):
    """rs_codec_decode_batch(_sums) on st (mutated like the caller's buffers)."""
    n, B = st.n, len(st.objs)
    flat = [a for row in st.bufs for a in row]
    lens = (ctypes.c_size_t * (B * n))(*[x for r in st.lens for x in r])
    outs = [_guard(len(o), 0xDD) for o in st.objs]
    sizes = (ctypes.c_int64 * B)(*[len(o) for o in st.objs])
    status = (ctypes.c_int * B)(*([99] * B))
    bad = _guard(B * n, 0x77)
    exp = _guard(B * n * 32, 0)
    _body(exp)[:] = st.expected.reshape(-1)
    if sums:
        rc = Nat.lib.rs_codec_decode_batch_sums(cx.handle, st.k, st.m, B, _ptrs(flat), lens,
                                                exp.ctypes.data + SENT, _ptrs(outs), sizes,
                                                bad.ctypes.data + SENT, status)
    else:
        rc = Nat.lib.rs_codec_decode_batch(cx.handle, st.k, st.m, B, _ptrs(flat), lens, _ptrs(outs), sizes, status)
    st.lens = [list(lens[b * n:(b + 1) * n]) for b in range(B)]
    return dict(rc=rc, status=list(status), outs=[_body(o).copy() for o in outs],
                bad=_body(bad).copy().reshape(B, n), guards=all(_sent_ok(a) for a in flat + outs + [bad, exp]))


def _same_state(a, b):
    return a.lens == b.lens and all((x == y).all() for ra, rb in zip(a.bufs, b.bufs) for x, y in zip(ra, rb))


def check_decode_clean(Nat, cx, k, m, seed):
    """Nothing missing, one data shard missing, m missing, at every edge size."""
    st = Stripes(Nat, cx, k, m, EDGES * 3, seed)
    for b in range(len(EDGES), 2 * len(EDGES)):
        st.drop(b, b % k)
    for b in range(2 * len(EDGES), 3 * len(EDGES)):
        for i in range(m):
            st.drop(b, (b + 3 * i) % st.n)
    ref = st.clone()
    want = decode(Nat, cx, ref, False)
    got = decode(Nat, cx, st, True)
    ok = {"guards": got["guards"], "rc": got["rc"] == want["rc"] == RS_OK, "status": got["status"] == want["status"],
          "bad_zero": not got["bad"].any(), "state": _same_state(st, ref),
          "outs": all((a == b).all() and (a == o).all() for a, b, o in zip(got["outs"], want["outs"], st.objs))}
    return ok, got


def check_sweep(Nat, cx, seed):
    """RS(4,2): one flipped byte per object, at every shard index and byte position."""
    k, m, n = 4, 2, 6
    cases = [(130, i, byte) for i in range(n) for byte in (0, 63, 64, 129)]
    cases += [(55, i, 54) for i in range(n)] + [(56, i, 55) for i in range(n)]
    st = Stripes(Nat, cx, k, m, [c[0] for c in cases] + [130, 55, 56], seed)
    for b, (_, i, byte) in enumerate(cases):
        st.flip(b, i, byte)
    got = decode(Nat, cx, st, True)
    want_bad = np.zeros((len(st.objs), n), np.uint8)
    for b, (_, i, _) in enumerate(cases):
        want_bad[b, i] = 1
    ok = {"guards": got["guards"], "rc": got["rc"] == RS_OK, "status": got["status"] == [RS_OK] * len(st.objs),
          "bad": bool((got["bad"] == want_bad).all()),
          "outs": all((a == o).all() for a, o in zip(got["outs"], st.objs)),
          "healed": all((_body(st.bufs[b][i]) == st.true[b][i]).all() for b in range(len(st.objs)) for i in range(n)),
          "lens": all(r == [s] * n for r, s in zip(st.lens, st.S))}
    return ok, got


def check_combos(Nat, cx, seed, big):
    """RS(10,4): the mismatch combinations, each beside the plain decode of the same object
    with the bad shards' lengths zero. big: object 0 has 300,000-byte shards."""
    k, m, n = 10, 4, 14
    st = Stripes(Nat, cx, k, m, [BIG if big else 777, 130, 130, 130, 130, 130, 64, 4099], seed)
    bad = {0: [2], 1: [3], 2: [12], 3: [5], 4: [9], 6: [0, 13]}
    st.flip(0, 2, st.S[0] - 1)           # (the big object:) a corrupt first-k shard
    st.flip(1, 3, 0)                     # a corrupt first-k shard
    st.flip(2, 12, 129)                  # a corrupt compared parity shard
    st.expected[3, 5, 7] ^= 1            # a wrong expected digest for a good shard
    for i in (0, 1, 10, 11):             # m missing plus one mismatch: too few shards left
        st.drop(4, i)
    st.flip(4, 9, 5)
    # 5: clean; 6: two missing plus two mismatches = m; 7: clean
    st.drop(6, 4)
    st.drop(6, 11)
    st.flip(6, 0, 1)
    st.flip(6, 13, 63)
    before = st.clone()
    ref = st.clone()
    for b, idx in bad.items():
        for i in idx:
            ref.lens[b][i] = 0
    want = decode(Nat, cx, ref, False)
    got = decode(Nat, cx, st, True)
    want_bad = np.zeros((len(st.objs), n), np.uint8)
    for b, idx in bad.items():
        want_bad[b, idx] = 1
    ok = {"guards": got["guards"], "bad": bool((got["bad"] == want_bad).all()),
          "status": got["status"] == want["status"] == [RS_OK] * 4 + [RS_E_TOO_FEW] + [RS_OK] * 3,
          "rc": got["rc"] == want["rc"] == RS_E_TOO_FEW}
    ok["outs"] = all((got["outs"][b] == st.objs[b]).all() and (want["outs"][b] == st.objs[b]).all()
                     for b in range(len(st.objs)) if b != 4)
    # the refused object: buffers and lens as given (the corrupt byte too), out untouched
    ok["too_few_untouched"] = st.lens[4] == before.lens[4] and \
        all((x == y).all() for x, y in zip(st.bufs[4], before.bufs[4])) and bool((got["outs"][4] == 0xDD).all())
    # the others: every shard holds its true bytes again, as after the plain decode
    ok["healed"] = all((_body(st.bufs[b][i]) == st.true[b][i]).all()
                       for b in range(len(st.objs)) if b != 4 for i in range(n))
    # (the wrong-digest shard of object 3 is rebuilt over itself: the same bytes)
    ref.lens[4] = before.lens[4]
    ok["state"] = st.lens == ref.lens
    return ok, got


def _counters(Nat, cx):
    c = Nat.HostCounters()
    assert Nat.lib.rs_host_counters_read(cx.handle, ctypes.byref(c)) == 0
    return {n: int(getattr(c, n)) for n, _ in c._fields_}


def check_counters(Nat, device):
    """A clean sums decode against the plain decode of the same (ragged) batch, each on a fresh
    context so that both pay the table upload; then one corrupt object among the 64."""
    k, m = 10, 4
    sizes = [256 + 16 * (b % 5) for b in range(64)]

    def run(prepare, sums, sub=None):
        cx = Nat.Context()
        st = Stripes(Nat, cx, k, m, sizes, 5)
        for b in range(0, 64, 7):
            st.drop(b, b % k)
        prepare(st)
        if sub is not None:
            st.objs, st.bufs, st.lens, st.S = [st.objs[sub]], [st.bufs[sub]], [st.lens[sub]], [st.S[sub]]
            st.expected = st.expected[sub:sub + 1]
        c0 = _counters(Nat, cx)
        r = decode(Nat, cx, st, sums)
        c1 = _counters(Nat, cx)
        cx.close()
        return {key: c1[key] - c0[key] for key in c0}, r

    plain, _ = run(lambda st: None, False)
    clean, r = run(lambda st: None, True)
    ok = {"clean_rc": r["rc"] == RS_OK and not r["bad"].any(),
          "chunks": clean["chunks"] == plain["chunks"] and plain["chunks"] >= 1,
          "copies": clean["copies"] == plain["copies"],
          "launches": clean["launches"] == plain["launches"] + (clean["chunks"] if device else 0)}

    def corrupt(st):
        st.flip(20, 3, 17)

    def as_missing(st):
        st.lens[20][3] = 0

    hurt, r = run(corrupt, True)
    alone, _ = run(as_missing, False, sub=20)
    ok["hurt_rc"] = r["rc"] == RS_OK and int(r["bad"].sum()) == 1 and r["bad"][20, 3] == 1
    ok["rerun_chunks"] = alone["chunks"] >= 1 and hurt["chunks"] == clean["chunks"] + alone["chunks"]
    return ok


def check_auto_rule(Nat, route):
    """A batch on which `auto` picks the device: 64 objects of RS(10,4) are 896 messages, none
    longer than 16 KiB, in one chunk. Correct on every route; RS(10,4) has one launch group, so
    a chunk costs one launch, and one more where it hashed on the device."""
    k, m = 10, 4
    cx = Nat.Context()
    st = Stripes(Nat, cx, k, m, [200 + 16 * (b % 5) for b in range(64)], 61)
    st.drop(7, 2)
    st.flip(9, 12, 0)
    c0 = _counters(Nat, cx)
    got = decode(Nat, cx, st, True)
    c1 = _counters(Nat, cx)
    enc = encode(Nat, cx, k, m, st.objs, True)
    c2 = _counters(Nat, cx)
    cx.close()
    want_bad = np.zeros((64, k + m), np.uint8)
    want_bad[9, 12] = 1
    ok = {"rc": got["rc"] == RS_OK and enc["rc"] == RS_OK, "bad": bool((got["bad"] == want_bad).all()),
          "outs": all((a == o).all() for a, o in zip(got["outs"], st.objs)),
          "healed": all((_body(st.bufs[b][i]) == st.true[b][i]).all() for b in range(64) for i in range(k + m)),
          "digests": bool((enc["digests"] == st.expected).all())}
    hashed = 0 if route == "host" else 1
    if route != "chunked":  # 64 KiB chunks hold fewer than 800 messages each
        # the encode: one chunk; the decode: one chunk, and object 9's run on its own
        ok["encode_launches"] = c2["chunks"] - c1["chunks"] == 1 and c2["launches"] - c1["launches"] == 1 + hashed
        ok["decode_launches"] = c1["chunks"] - c0["chunks"] == 2 and c1["launches"] - c0["launches"] == 2 + hashed
    return ok, got


def check_python(Nat, E, cx):
    prof = E.ErasureProfile(4, 2)
    codec = E.Codec(cx)
    rng = np.random.default_rng(3)
    datas = [rng.integers(0, 256, L, dtype=np.uint8).tobytes() for L in (1, 517, 4096)] + [b""]
    shards, sums, errors = codec.encode_many_sums(datas, prof)
    ok = {"enc_errors": errors[:3] == [None] * 3 and sums[3] is None and shards[3] is None}
    try:
        codec.encode(b"", prof)
    except Exception as e:  # noqa: BLE001
        ok["enc_error_class"] = type(errors[3]) is type(e) and str(errors[3]) == str(e)
    ok["checksums"] = all(sums[b][i] == E.shard_checksum(shards[b][i]) and len(sums[b][i]) == 64
                          for b in range(3) for i in range(6))
    per = [[bytearray(s) for s in shards[b]] for b in range(3)]
    per[1][2][5] ^= 1                 # one corrupt shard: healed
    per[2][0] = None                  # m missing plus a mismatch: too few
    per[2][1] = None
    per[2][4][0] ^= 1
    objs, bad, errs = codec.decode_many_sums(per, sums[:3], prof, [len(d) for d in datas[:3]])
    ok["dec_bad"] = bad == [[], [2], [4]]
    ok["dec_objs"] = bytes(objs[0]) == datas[0] and bytes(objs[1]) == datas[1] and objs[2] is None
    ok["dec_healed"] = bytes(per[1][2]) == bytes(shards[1][2])
    try:
        codec.decode([None, None, bytearray(shards[2][2]), bytearray(shards[2][3]), None, bytearray(shards[2][5])],
                     prof, len(datas[2]))
    except Exception as e:  # noqa: BLE001
        ok["dec_error_class"] = errs[:2] == [None, None] and type(errs[2]) is type(e) and str(errs[2]) == str(e)
    return ok


def _digest(*results):
    h = hashlib.sha256()
    for r in results:
        for key in ("status", "sizes"):
            h.update(repr(r.get(key)).encode())
        for key in ("shards", "outs"):
            for a in r.get(key, []):
                h.update(a.tobytes())
        for key in ("digests", "bad"):
            if key in r:
                h.update(r[key].tobytes())
    return h.hexdigest()


def scenarios(route):
    """Every scenario once: {name: {check: bool}} and a digest of all results."""
    Nat, E = _env()
    cx = Nat.default_context()
    out, results = {}, []
    for k, m in ((4, 2), (10, 4), (16, 4), (3, 18)):
        out[f"encode_{k}_{m}"], r = check_encode(Nat, cx, k, m, EDGES, 11 + k, empty_at=5)
        results.append(r)
    out["encode_big"], r = check_encode(Nat, cx, 10, 4, [64, BIG, 130, 1], 21)
    results.append(r)
    for k, m in ((4, 2), (10, 4)):
        out[f"decode_clean_{k}_{m}"], r = check_decode_clean(Nat, cx, k, m, 31 + k)
        results.append(r)
    out["sweep"], r = check_sweep(Nat, cx, 41)
    results.append(r)
    out["combos"], r = check_combos(Nat, cx, 51, False)
    results.append(r)
    out["combos_big"], r = check_combos(Nat, cx, 52, True)
    results.append(r)
    out["auto_rule"], r = check_auto_rule(Nat, route)
    results.append(r)
    out["python"] = check_python(Nat, E, cx)
    if route in ("host", "device"):
        out["counters"] = check_counters(Nat, route == "device")
    # the call-level argument checks
    L = Nat.lib
    one = (ctypes.c_void_p * 1)()
    sz = (ctypes.c_size_t * 1)(1)
    i64 = (ctypes.c_int64 * 1)(1)
    st = (ctypes.c_int * 1)()
    buf = np.zeros(64, np.uint8).ctypes.data
    out["args"] = {
        "enc_null_digests": L.rs_codec_encode_batch_sums(cx.handle, 4, 2, 1, one, sz, one, sz, sz, None, st) == RS_E_ARG,
        "dec_null_expected": L.rs_codec_decode_batch_sums(cx.handle, 4, 2, 1, one, sz, None, one, i64, buf, st) == RS_E_ARG,
        "dec_null_bad": L.rs_codec_decode_batch_sums(cx.handle, 4, 2, 1, one, sz, buf, one, i64, None, st) == RS_E_ARG,
        "enc_empty": L.rs_codec_encode_batch_sums(cx.handle, 4, 2, 0, None, None, None, None, None, None, None) == RS_OK,
        "dec_empty": L.rs_codec_decode_batch_sums(cx.handle, 4, 2, 0, None, None, None, None, None, None, None) == RS_OK,
        "enc_profile": L.rs_codec_encode_batch_sums(cx.handle, 0, 2, 1, one, sz, one, sz, sz, buf, st) == Nat.RS_E_INVALID_PROFILE,
    }
    return {"checks": out, "digest": _digest(*results)}


@functools.lru_cache(maxsize=None)
def _run(route):
    if route == "auto":
        return scenarios(route)
    env = dict(os.environ)
    for key in ("CALLFS_RS_SUMS_DEVICE", "CALLFS_RS_SMALL_MAX_BYTES", "CALLFS_RS_CHUNK_BYTES",
                "CALLFS_RS_INPLACE_PIPELINE", "CALLFS_RS_RAGGED_BATCH"):
        env.pop(key, None)
    env.update(ROUTES[route])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", route], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert lines, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(lines[-1][len("RESULT "):])


SCENARIOS = ["encode_4_2", "encode_10_4", "encode_16_4", "encode_3_18", "encode_big", "decode_clean_4_2",
             "decode_clean_10_4", "sweep", "combos", "combos_big", "auto_rule", "python", "args"]


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["auto", "host", "device", "chunked"])
@pytest.mark.parametrize("name", SCENARIOS)
def test_scenario(route, name):
    checks = _run(route)["checks"][name]
    assert checks and all(checks.values()), (route, name, checks)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["host", "device"])
def test_counters(route):
    checks = _run(route)["checks"]["counters"]
    assert checks and all(checks.values()), (route, checks)


@pytest.mark.gpu
def test_routes_return_the_same_bytes():
    digests = {route: _run(route)["digest"] for route in ("auto", "host", "device", "chunked")}
    assert len(set(digests.values())) == 1, digests


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "child":
        print("RESULT " + json.dumps(scenarios(sys.argv[2]), default=bool))
    else:
        sys.exit(pytest.main([__file__, "-q", "-m", "gpu"]))
