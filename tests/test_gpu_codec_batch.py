"""Codec-level batch calls: rs_codec_encode_batch / rs_codec_decode_batch take objects in and
give objects out, Split done on the way into the pipeline's staging and the join / trim on the
way out of it.

Every result is compared byte for byte with the CPU oracle (oracle.cref) and with the
per-object calls on copies of the same inputs: Codec.encode, Codec.decode, and rs_codec_decode
itself where an object carries a NULL pointer that the Python codec cannot express. Every
buffer handed to the library carries 64 sentinel bytes on both sides, which no call may change.
The scenarios run in this process with the default settings -- where their staging is under
CALLFS_RS_SMALL_MAX_BYTES they take the one-dispatch in-place transport -- and again in fresh
child processes whose environment selects another transport or path (the settings are read once
per process): the staged transport (CALLFS_RS_SMALL_MAX_BYTES=0), column cuts over many chunks
(CALLFS_RS_CHUNK_BYTES=65536, with and without CALLFS_RS_INPLACE_PIPELINE=1) and the per-group
path (CALLFS_RS_RAGGED_BATCH=0). A child prints one JSON line of named checks.

"Exactly k present, with the data shards all lost": a profile with m < k cannot lose all its
data shards and keep k, so those objects lose m shards, every one of them a data shard.

  python tests/test_gpu_codec_batch.py child <scenario> ...     # what a child runs
"""
import ctypes
import functools
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RS_OK, RS_E_SHORT, RS_E_TOO_FEW, RS_E_SHARD_SIZE, RS_E_NO_DATA = 0, -2, -3, -4, -5
RS_E_CORRUPT, RS_E_INSUFFICIENT, RS_E_ARG = -6, -7, -10
RAN = (RS_OK, RS_E_CORRUPT, RS_E_INSUFFICIENT)  # Reconstruct ran: the missing shards are filled
SENT = 64
SIZE_UNSET = 12345

GRID_4_2 = [1, 2, 3, 4, 5, 63, 64, 65, 16 * 4 + 1, 8192 * 4 - 1, 8192 * 4 + 1]
GRID_10_4 = [1, 2, 3, 4, 5, 10, 11, 159, 160, 16 * 10 + 1, 8192 * 10 - 1, 8192 * 10 + 1]
ROW_PROFILES = [(3, 2), (10, 8), (20, 16), (10, 20), (1, 3)]


def _env():
    sys.path.insert(0, ROOT)
    from callfs_amd import _native as Nat
    from callfs_amd import erasure
    from oracle import cref
    return Nat, erasure, cref


@functools.lru_cache(maxsize=None)
def _ref(k, m, lens, seed):
    """Per object (bytes, S, the n shards back to back) from the oracle; shared, never written."""
    _, _, cref = _env()
    rng = np.random.default_rng(seed)
    out = []
    for L in lens:
        if L == 0:
            out.append(None)
            continue
        obj = rng.integers(0, 256, L, dtype=np.uint8)
        if (k, m, L) == (4, 2, 2):
            obj = np.frombuffer(b"hi", np.uint8).copy()
        S = -(-L // k)
        padded = np.zeros(k * S, np.uint8)
        padded[:L] = obj
        data = [padded[i * S:(i + 1) * S].copy() for i in range(k)]
        flat = np.concatenate(data + [np.ascontiguousarray(p) for p in cref.encode(data, k, m)])
        flat.setflags(write=False)
        obj.setflags(write=False)
        out.append((obj, S, flat))
    return out


def _numpy_alloc(nb):
    return np.empty(nb, np.uint8)


def _mk(alloc, size, fill):
    a = alloc(size + 2 * SENT)
    a[:] = 0xA5
    a[SENT:SENT + size] = fill
    return a


def _p(a):
    return a.ctypes.data + SENT


def _body(a):
    return a[SENT:len(a) - SENT]


def _sent_ok(a):
    return bool((a[:SENT] == 0xA5).all() and (a[len(a) - SENT:] == 0xA5).all())


def _ptr_array(ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def _counters(Nat, cx):
    c = Nat.HostCounters()
    assert Nat.lib.rs_host_counters_read(cx.handle, ctypes.byref(c)) == 0
    return {n: int(getattr(c, n)) for n, _ in c._fields_}


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


_single_encode_seen = {}


def _single_encode_ok(cx, k, m, lens, seed):
    """Codec.encode of every object alone equals the oracle's codeword (once per process)."""
    key = (k, m, tuple(lens), seed)
    if key not in _single_encode_seen:
        _, E, _ = _env()
        ok = True
        for r in _ref(*key):
            if r is None:
                continue
            obj, S, flat = r
            sh = E.Codec(cx).encode(obj.tobytes(), E.ErasureProfile(k, m))
            ok &= len(sh) == k + m and all(bytes(s) == flat[i * S:(i + 1) * S].tobytes()
                                           for i, s in enumerate(sh))
        _single_encode_seen[key] = bool(ok)
    return _single_encode_seen[key]


def encode_case(Nat, cx, k, m, lens, seed=1, inplace=False, alloc=None, bad=None, pageable=(),
                single=True):
    """One rs_codec_encode_batch. lens[b] == 0 is an empty object; bad[b] in {"null_data",
    "null_out", "short_cap"}; pageable: objects whose buffers come from numpy whatever `alloc`."""
    n, B, bad = k + m, len(lens), bad or {}
    ref = _ref(k, m, tuple(lens), seed)
    alloc = alloc or _numpy_alloc
    dbufs, sbufs, dptr, sptr, caps, want = [], [], [], [], [], []
    for b, L in enumerate(lens):
        S = -(-L // k)
        al = _numpy_alloc if b in pageable else alloc
        if inplace and L:
            s = _mk(al, n * S, 0x77)
            _body(s)[:L] = ref[b][0]
            d = s
        else:
            d = _mk(al, L, 0)
            if L:
                _body(d)[:] = ref[b][0]
            s = _mk(al, n * S if L else 8, 0x77)
        kind = bad.get(b)
        dbufs.append(d)
        sbufs.append(s)
        dptr.append(0 if kind == "null_data" else _p(d))
        sptr.append(0 if kind == "null_out" else _p(s))
        caps.append(n * S - 1 if kind == "short_cap" else n * S)
        want.append(RS_E_SHORT if L == 0 else RS_E_ARG if kind else RS_OK)
    d0 = [d.copy() for d in dbufs]
    s0 = [s.copy() for s in sbufs]
    sizes = (ctypes.c_size_t * B)(*[SIZE_UNSET] * B)
    status = (ctypes.c_int * B)(*[77] * B)
    c0 = _counters(Nat, cx)
    rc = Nat.lib.rs_codec_encode_batch(cx.handle, k, m, B, _ptr_array(dptr),
                                       (ctypes.c_size_t * B)(*lens), _ptr_array(sptr),
                                       (ctypes.c_size_t * B)(*caps), sizes, status)
    counters = _delta(c0, _counters(Nat, cx))
    ck = dict(bytes=True, sentinels=True, inputs=True, sizes=True, bad_untouched=True)
    for b, L in enumerate(lens):
        if want[b] == RS_OK:
            ck["bytes"] &= bool(np.array_equal(_body(sbufs[b]), ref[b][2]))
            ck["sentinels"] &= _sent_ok(sbufs[b])
            ck["sizes"] &= sizes[b] == ref[b][1]
            if not inplace:
                ck["inputs"] &= bool(np.array_equal(dbufs[b], d0[b]))
        else:
            ck["bad_untouched"] &= bool(np.array_equal(sbufs[b], s0[b]) and
                                        np.array_equal(dbufs[b], d0[b]) and sizes[b] == SIZE_UNSET)
    if single:
        ck["single"] = _single_encode_ok(cx, k, m, lens, seed)
    res = {"rc": rc, "status": list(status), "want": want, "checks": ck, "counters": counters}
    if (k, m) == (4, 2) and 2 in lens and want[lens.index(2)] == RS_OK:
        res["hi"] = _body(sbufs[lens.index(2)]).tobytes().hex()
    return res


def _decode_class(E, st):
    return {RS_E_CORRUPT: E.ErrShardCorrupted, RS_E_INSUFFICIENT: E.ErrInsufficientShards,
            RS_E_TOO_FEW: E.ErrTooFewShards, RS_E_SHARD_SIZE: E.ErrShardSize,
            RS_E_NO_DATA: E.ErrShardNoData}.get(st)


def decode_case(Nat, cx, k, m, lens, masks, origs, seed=1, flips=(), wrong_len=(), null_shard=(),
                null_out=(), alloc=None, pageable=(), single=True):
    """One rs_codec_decode_batch. masks[b]: the missing shard indices of object b; origs[b]: its
    original_size. flips: (object, shard, byte) flipped in a compared shard (present, beyond the
    first k present). wrong_len: (object, shard) given a length one less. null_shard: (object,
    shard) present with a NULL pointer. null_out: objects whose out pointer is NULL."""
    Nat, E, _ = _env()
    n, B = k + m, len(lens)
    ref = _ref(k, m, tuple(lens), seed)
    alloc = alloc or _numpy_alloc
    bufs, outs, ptrs, optr, want = [], [], [], [], []
    ln = (ctypes.c_size_t * (B * n))()
    for b, L in enumerate(lens):
        _, S, flat = ref[b]
        al = _numpy_alloc if b in pageable else alloc
        for i in range(n):
            gone = i in masks[b]
            a = _mk(al, S, 0x5A if gone else flat[i * S:(i + 1) * S])
            ln[b * n + i] = 0 if gone else S
            bufs.append(a)
            ptrs.append(0 if (b, i) in null_shard else _p(a))
        o = _mk(al, origs[b], 0x33)
        outs.append(o)
        optr.append(0 if b in null_out else _p(o))
    for b, i, at in flips:
        _body(bufs[b * n + i])[at] ^= 0x10
    for b, i in wrong_len:
        ln[b * n + i] -= 1
    for b in range(B):
        S = ref[b][1]
        np_ = n - len(masks[b])
        if np_ == 0:
            w = RS_E_NO_DATA
        elif any(x == b for x, _ in wrong_len):
            w = RS_E_SHARD_SIZE
        elif np_ < k:
            w = RS_E_TOO_FEW
        elif any(x == b for x, _ in null_shard) or (b in null_out and origs[b] > 0):
            w = RS_E_ARG
        elif any(x == b for x, _, _ in flips):
            w = RS_E_CORRUPT
        elif origs[b] > k * S:
            w = RS_E_INSUFFICIENT
        else:
            w = RS_OK
        want.append(w)
    before = [a.copy() for a in bufs]
    out0 = [o.copy() for o in outs]
    ln0 = list(ln)
    sz = (ctypes.c_int64 * B)(*origs)
    status = (ctypes.c_int * B)(*[77] * B)
    c0 = _counters(Nat, cx)
    rc = Nat.lib.rs_codec_decode_batch(cx.handle, k, m, B, _ptr_array(ptrs), ln, _ptr_array(optr), sz,
                                       status)
    counters = _delta(c0, _counters(Nat, cx))
    st = list(status)
    ck = dict(joined=True, rebuilt=True, untouched=True, lens=True, sentinels=True)
    for b in range(B):
        _, S, flat = ref[b]
        ran = st[b] in RAN
        for i in range(n):
            a = bufs[b * n + i]
            if i in masks[b] and ran:
                ck["rebuilt"] &= bool(np.array_equal(_body(a), flat[i * S:(i + 1) * S]))
                ck["sentinels"] &= _sent_ok(a)
                ck["lens"] &= ln[b * n + i] == S
            else:  # present shards, and every shard of an object that did not run: never written
                ck["untouched"] &= bool(np.array_equal(a, before[b * n + i]))
                ck["lens"] &= ln[b * n + i] == ln0[b * n + i]
        ck["sentinels"] &= _sent_ok(outs[b])
        if st[b] == RS_OK:
            ck["joined"] &= bool(np.array_equal(_body(outs[b]), flat[:origs[b]]))
        elif not ran:
            ck["untouched"] &= bool(np.array_equal(outs[b], out0[b]))
    if single:
        # each object alone, on copies of what the batch was given
        ok = True
        for b in range(B):
            _, S, flat = ref[b]
            has_null = b in null_out or any(x == b for x, _ in null_shard)
            if has_null:
                cp = [before[b * n + i].copy() for i in range(n)]
                o = out0[b].copy()
                l1 = (ctypes.c_size_t * n)(*ln0[b * n:(b + 1) * n])
                r1 = Nat.lib.rs_codec_decode(cx.handle, k, m, _ptr_array(
                    [0 if (b, i) in null_shard else _p(cp[i]) for i in range(n)]), l1,
                    None if b in null_out else _p(o), origs[b])
                ok &= r1 == st[b]
                continue
            sh = [None if ln0[b * n + i] == 0 else bytearray(_body(before[b * n + i])[:ln0[b * n + i]])
                  for i in range(n)]
            try:
                got = E.Codec(cx).decode(sh, E.ErasureProfile(k, m), origs[b])
                ok &= st[b] == RS_OK and bytes(got) == _body(outs[b]).tobytes()
            except E.ErasureError as e:
                ok &= type(e) is _decode_class(E, st[b])
            if st[b] in RAN:
                ok &= all(bytes(sh[i]) == _body(bufs[b * n + i]).tobytes() for i in range(n))
        ck["single"] = bool(ok)
    return {"rc": rc, "status": st, "want": want, "checks": ck, "counters": counters}


def _lens_for(k, count, seed, hi=40_000):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(2, hi, count)]


def _mask_kinds(k, m):
    """nothing missing; one data shard; one parity shard; m missing across both (m >= 2), else
    one; exactly k present with every lost shard a data shard."""
    n = k + m
    across = tuple(sorted({1 % k, n - 1} | set(range(k, k + m - 2)))) if m >= 2 else (n - 1,)
    return [(), (k - 1,), (k,), across, tuple(range(min(m, k)))]


def _decode_grid(k, m, seed):
    """Every mask kind with every original size of {0, 1, L, L - 1, k * S}."""
    kinds = _mask_kinds(k, m)
    lens = _lens_for(k, 5 * len(kinds), seed, hi=20_000)
    masks, origs = [], []
    for j, L in enumerate(lens):
        S = -(-L // k)
        masks.append(kinds[j % len(kinds)])
        origs.append([0, 1, L, L - 1, k * S][j // len(kinds)])
    return lens, masks, origs


# ---- scenarios: each returns a dict of named results ------------------------------------------

def sc_enc_grid(Nat, cx):
    out = {}
    for (k, m), grid in (((4, 2), GRID_4_2), ((10, 4), GRID_10_4)):
        for inplace in (False, True):
            out[f"{k}_{m}_{'inplace' if inplace else 'separate'}"] = encode_case(
                Nat, cx, k, m, grid, seed=k, inplace=inplace)
    return out


def sc_rows(Nat, cx):
    out = {}
    for k, m in ROW_PROFILES:
        n = k + m
        lens = _lens_for(k, 6, seed=100 * k + m)
        out[f"enc_{k}_{m}"] = encode_case(Nat, cx, k, m, lens, seed=100 * k + m, inplace=(k % 2 == 0))
        kinds = _mask_kinds(k, m)
        masks = [kinds[(b + 1) % len(kinds)] for b in range(6)]
        out[f"dec_{k}_{m}"] = decode_case(Nat, cx, k, m, lens, masks, lens, seed=100 * k + m)
        assert all(len(x) <= m and n - len(x) >= k for x in masks)
    return out


def sc_dec_grid(Nat, cx):
    out = {}
    for k, m in ((10, 4), (4, 2)):
        lens, masks, origs = _decode_grid(k, m, seed=50 + k)
        out[f"{k}_{m}"] = decode_case(Nat, cx, k, m, lens, masks, origs, seed=50 + k)
    return out


STATUS_S = [700, 33, 5000, 901, 64, 17, 1200, 4095, 16467, 300, 2048, 8193, 40, 77]


def _status_batch():
    k, m = 10, 4
    lens = [k * S - (b % k) for b, S in enumerate(STATUS_S)]
    masks = [(0,), (0, 1, 2, 3, 4), (), (2,), tuple(range(14)), (13,), (1,), (1,), (13,), (), (3, 12),
             (0, 11), (), (5, 6)]
    origs = list(lens)
    origs[9] = k * STATUS_S[9] + 1    # insufficient
    origs[10] = k * STATUS_S[10] + 5  # insufficient and corrupt: corrupt wins
    kw = dict(wrong_len=[(3, 5)], null_shard=[(6, 2)], null_out=[12],
              flips=[(7, 12, 1000), (8, 12, 16467 - 2), (10, 13, 7)])
    want = [0, RS_E_TOO_FEW, 0, RS_E_SHARD_SIZE, RS_E_NO_DATA, 0, RS_E_ARG, RS_E_CORRUPT, RS_E_CORRUPT,
            RS_E_INSUFFICIENT, RS_E_CORRUPT, 0, RS_E_ARG, 0]
    return k, m, lens, masks, origs, kw, want


def sc_statuses(Nat, cx):
    k, m, lens, masks, origs, kw, want = _status_batch()
    dec = decode_case(Nat, cx, k, m, lens, masks, origs, seed=21, **kw)
    dec["expected"] = want
    elens = [900, 0, 41, 5000, 77, 12, 65]
    enc = encode_case(Nat, cx, k, m, elens, seed=22, bad={2: "null_data", 4: "short_cap", 5: "null_out"})
    enc_in = encode_case(Nat, cx, k, m, elens, seed=22, inplace=True, bad={4: "short_cap"})
    return {"dec": dec, "enc": enc, "enc_inplace": enc_in}


CUT_LENS = [4 * 100_003 - 1, 4 * 700, 4 * 40_003 - 2, 61, 9, 4 * 8192 + 1]


def sc_cuts(Nat, cx):
    k, m = 4, 2
    masks = [(1,), (0, 5), (0, 1), (2, 3), (), (4,)]
    origs = [CUT_LENS[0], CUT_LENS[1] - 1, CUT_LENS[2], 1, 9, 4 * 8193]
    return {"enc": encode_case(Nat, cx, k, m, CUT_LENS, seed=7),
            "enc_inplace": encode_case(Nat, cx, k, m, CUT_LENS, seed=7, inplace=True),
            # object 0's parts are 8,192 wide at this budget: byte 9,000 of compared shard 5 lies
            # in the second part
            "dec": decode_case(Nat, cx, k, m, CUT_LENS, masks, origs, seed=7, flips=[(0, 5, 9000)])}


def sc_uniform(Nat, cx):
    lens = [9993] * 8
    return {"enc": encode_case(Nat, cx, 10, 4, lens, seed=6),
            "enc_inplace": encode_case(Nat, cx, 10, 4, lens, seed=6, inplace=True),
            "dec": decode_case(Nat, cx, 10, 4, lens, [(2,)] * 8, lens, seed=6)}


COUNTER_LENS = [10 * (1 + 331 * b) - (b % 10) for b in range(16)]


def _presplit_counters(Nat, k, m, lens, seed, masks):
    """Counter deltas of rs_encode_batch (masks None) / rs_reconstruct_batch with verify on the
    objects pre-split, on a fresh context of one device."""
    n, B = k + m, len(lens)
    ref = _ref(k, m, tuple(lens), seed)
    cx = Nat.Context(1)
    try:
        rows = [[np.array(flat[i * S:(i + 1) * S]) for i in range(n)] for _, S, flat in ref]
        sizes = (ctypes.c_size_t * B)(*[S for _, S, _ in ref])
        status = (ctypes.c_int * B)()
        c0 = _counters(Nat, cx)
        if masks is None:
            rc = Nat.lib.rs_encode_batch(cx.handle, k, m, B, sizes,
                                         _ptr_array([a.ctypes.data for r in rows for a in r[:k]]),
                                         _ptr_array([a.ctypes.data for r in rows for a in r[k:]]), status)
        else:
            ln = (ctypes.c_size_t * (B * n))(*[0 if i in masks[b] else ref[b][1]
                                              for b in range(B) for i in range(n)])
            rc = Nat.lib.rs_reconstruct_batch(cx.handle, k, m, B,
                                              _ptr_array([a.ctypes.data for r in rows for a in r]), ln, 1,
                                              status)
        assert rc == 0
        return _delta(c0, _counters(Nat, cx))
    finally:
        cx.close()


def sc_counters(Nat, cx):
    """Fresh contexts throughout (cx is not used): a ragged batch and a uniform one."""
    out = {}
    k, m = 10, 4
    for name, lens in (("ragged", COUNTER_LENS), ("uniform", [5000] * 6)):
        masks = [((b * 3) % 14,) for b in range(len(lens))] if name == "ragged" else [(1,)] * len(lens)
        for leg in ("enc", "enc_inplace", "dec"):
            fresh = Nat.Context(1)
            try:
                if leg == "dec":
                    r = decode_case(Nat, fresh, k, m, lens, masks, lens, seed=8, single=False)
                else:
                    r = encode_case(Nat, fresh, k, m, lens, seed=8, inplace=leg == "enc_inplace", single=False)
            finally:
                fresh.close()
            r["presplit"] = _presplit_counters(Nat, k, m, lens, 8, masks if leg == "dec" else None)
            out[f"{name}_{leg}"] = r
    return out


SCENARIOS = {f.__name__[3:]: f for f in (sc_enc_grid, sc_rows, sc_dec_grid, sc_statuses, sc_cuts,
                                         sc_uniform, sc_counters)}


def _run(names, Nat, cx):
    return {n: SCENARIOS[n](Nat, cx) for n in names}


def _child(names):
    Nat, _, _ = _env()
    one = Nat.Context(1)
    print(json.dumps(_run(names, Nat, one)))


@functools.lru_cache(maxsize=None)
def _spawn(names, env_items):
    env = dict(os.environ, **dict(env_items))
    for name in ("CALLFS_RS_CHUNK_BYTES", "CALLFS_RS_SMALL_MAX_BYTES", "CALLFS_RS_INPLACE_PIPELINE",
                 "CALLFS_RS_RAGGED_BATCH", "CALLFS_RS_ZERO_COPY_MIN_BYTES"):
        if name not in dict(env_items):
            env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", *names], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.splitlines()[-1])


def _staged():
    return _spawn(("enc_grid", "rows", "dec_grid", "statuses", "counters"),
                  (("CALLFS_RS_SMALL_MAX_BYTES", "0"),))


def _toggle_off():
    return _spawn(("enc_grid", "dec_grid"), (("CALLFS_RS_RAGGED_BATCH", "0"),))


@pytest.fixture(scope="module")
def here():
    """The scenarios in this process, default settings, on a context of one device."""
    Nat, _, _ = _env()
    cx = Nat.Context(1)
    yield _run(("enc_grid", "rows", "dec_grid", "statuses", "uniform", "counters"), Nat, cx)
    cx.close()


def _where(here, where):
    return {"inplace": lambda: here, "staged": _staged, "toggle_off": _toggle_off}[where]()


def _check(r, want=None):
    """No object skipped: every status is the expected one, every check holds, and the call
    returns the first nonzero status."""
    want = r["want"] if want is None else want
    assert r["status"] == want
    assert r["want"] == want, "the test's own expectation disagrees with its status rule"
    assert r["rc"] == next((s for s in want if s), RS_OK)
    bad = [name for name, ok in r["checks"].items() if not ok]
    assert not bad, f"failed checks: {bad}"


# ---- encode -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("where", ["inplace", "staged", "toggle_off"])
@pytest.mark.parametrize("profile", ["4_2", "10_4"])
@pytest.mark.parametrize("form", ["separate", "inplace"])
def test_encode_length_grid(here, where, profile, form):
    r = _where(here, where)["enc_grid"][f"{profile}_{form}"]
    _check(r, [RS_OK] * len(r["status"]))
    assert r["counters"]["calls"] == 1
    assert r["counters"]["ragged_calls"] == (0 if where == "toggle_off" else 1)
    if profile == "4_2":
        assert r["hi"] == "686900" "00191e"  # "hi" -> h, i, 00, 00, 19, 1e


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", ROW_PROFILES)
@pytest.mark.parametrize("where", ["inplace", "staged"])
def test_row_counts(here, where, k, m):
    res = _where(here, where)["rows"]
    _check(res[f"enc_{k}_{m}"], [RS_OK] * 6)
    _check(res[f"dec_{k}_{m}"], [RS_OK] * 6)
    # one launch per group of 16 rows per chunk: RS(10,20) has two groups
    assert res[f"enc_{k}_{m}"]["counters"]["launches"] == \
        res[f"enc_{k}_{m}"]["counters"]["chunks"] * ((m + 15) // 16)


# ---- decode -----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("where", ["inplace", "staged", "toggle_off"])
@pytest.mark.parametrize("profile", ["10_4", "4_2"])
def test_decode_masks_and_original_sizes(here, where, profile):
    r = _where(here, where)["dec_grid"][profile]
    _check(r, [RS_OK] * 25)
    assert r["counters"]["ragged_calls"] == (0 if where == "toggle_off" else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["inplace", "staged"])
def test_statuses_among_healthy_objects(here, where):
    res = _where(here, where)["statuses"]
    _check(res["dec"], res["dec"]["expected"])
    assert res["dec"]["rc"] == RS_E_TOO_FEW  # object 1: the first nonzero status
    want = [RS_OK, RS_E_SHORT, RS_E_ARG, RS_OK, RS_E_ARG, RS_E_ARG, RS_OK]
    _check(res["enc"], want)
    assert res["enc"]["rc"] == RS_E_SHORT
    _check(res["enc_inplace"], [RS_OK, RS_E_SHORT, RS_OK, RS_OK, RS_E_ARG, RS_OK, RS_OK])


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [False, True])
def test_column_cuts_over_many_chunks(inplace):
    """CALLFS_RS_CHUNK_BYTES=65536: the 400,011- and 160,010-byte objects of RS(4,2) become
    column parts of 8,192 bytes among the small objects, over more than three chunks on three
    slots; tees and joins are exact at every cut, and a flipped byte in the second part of
    object 0 flags that object alone."""
    env = [("CALLFS_RS_CHUNK_BYTES", "65536"), ("CALLFS_RS_SMALL_MAX_BYTES", "0")]
    if inplace:
        env.append(("CALLFS_RS_INPLACE_PIPELINE", "1"))
    res = _spawn(("cuts",), tuple(env))["cuts"]
    for name in ("enc", "enc_inplace"):
        _check(res[name], [RS_OK] * 6)
        assert res[name]["counters"]["chunks"] > 3
    _check(res["dec"], [RS_E_CORRUPT] + [RS_OK] * 5)
    assert res["dec"]["counters"]["chunks"] > 3


@pytest.mark.gpu
def test_uniform_batch_keeps_its_path(here):
    for name in ("enc", "enc_inplace", "dec"):
        r = here["uniform"][name]
        _check(r, [RS_OK] * 8)
        assert r["counters"]["ragged_calls"] == 0 and r["counters"]["calls"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["inplace", "staged"])
@pytest.mark.parametrize("leg", ["enc", "enc_inplace", "dec"])
@pytest.mark.parametrize("shape", ["ragged", "uniform"])
def test_counters_equal_the_shard_level_batch(here, where, shape, leg):
    """On fresh contexts a codec batch counts calls, ragged_calls, chunks, launches and copies
    exactly as rs_encode_batch / rs_reconstruct_batch given the same objects pre-split."""
    r = _where(here, where)["counters"][f"{shape}_{leg}"]
    _check(r, [RS_OK] * len(r["status"]))
    assert r["counters"] == r["presplit"]
    assert r["counters"]["ragged_calls"] == (1 if shape == "ragged" else 0)


# ---- direct transport -------------------------------------------------------------------------

@pytest.mark.gpu
def test_direct_on_pinned_buffers_and_staged_fallback():
    """Every buffer from rs_host_alloc, six objects of 0.6 to 1.6 MB: the kernels run on the
    caller's bytes (one chunk; the copies are the metadata, the tables and the status words) and
    the tees and joins are copy-pool work. The same batch with one pageable object takes the
    staged transport. Both are bit-exact with the oracle, hence with each other."""
    Nat, _, _ = _env()
    cx = Nat.Context(1)
    pin = Nat.PinnedBuffer(96 << 20, cx)
    at = [0]

    def alloc(nb):  # carved from one allocation, 64-B aligned, the sentinels inside it
        a = pin.array[at[0]:at[0] + nb]
        at[0] += (nb + 63) // 64 * 64
        assert at[0] <= pin.nbytes
        return a

    k, m = 10, 4
    lens = [k * (60_000 + 20_000 * b) - (b % k) for b in range(6)]
    masks = [(), (0,), (12,), (1, 13), (0, 1, 2, 3), (9,)]
    origs = [lens[0], lens[1] - 1, 0, lens[3], lens[4], 1]
    try:
        for inplace in (False, True):
            r = encode_case(Nat, cx, k, m, lens, seed=9, inplace=inplace, alloc=alloc, single=not inplace)
            _check(r, [RS_OK] * 6)
            assert r["counters"]["chunks"] == 1 and r["counters"]["launches"] == 1
            assert r["counters"]["copies"] <= 3 and r["counters"]["ragged_calls"] == 1
        # compared shard 13 of object 2 (mask (12,)) carries a flipped byte
        r = decode_case(Nat, cx, k, m, lens, masks, origs, seed=9, alloc=alloc, flips=[(2, 13, 70_001)])
        _check(r, [RS_OK, RS_OK, RS_E_CORRUPT, RS_OK, RS_OK, RS_OK])
        assert r["counters"]["chunks"] == 1 and r["counters"]["launches"] == 1
        assert r["counters"]["copies"] <= 3
        at[0] = 0
        r = encode_case(Nat, cx, k, m, lens, seed=9, alloc=alloc, pageable={3}, single=False)
        _check(r, [RS_OK] * 6)
        assert r["counters"]["copies"] >= 2 * r["counters"]["chunks"]  # staged: H2D and D2H per chunk
        r = decode_case(Nat, cx, k, m, lens, masks, origs, seed=9, alloc=alloc, pageable={3}, single=False)
        _check(r, [RS_OK] * 6)
        assert r["counters"]["copies"] >= 2 * r["counters"]["chunks"]
    finally:
        pin.close()
        cx.close()


# ---- concurrency ------------------------------------------------------------------------------

@pytest.mark.gpu
def test_eight_threads_on_one_context():
    Nat, _, _ = _env()
    cx = Nat.default_context()
    k, m = 10, 4
    lens = [7, 3000, 40_961, 90_001, 333]
    kinds = _mask_kinds(k, m)
    _ref(k, m, tuple(lens), 11)  # shared reference, computed once
    errors = []

    def work(t):
        try:
            for _ in range(2):
                _check(encode_case(Nat, cx, k, m, lens, seed=11, inplace=bool(t & 1), single=False))
                masks = kinds[t % 5:] + kinds[:t % 5]
                origs = [L - (t % 2) for L in lens]
                _check(decode_case(Nat, cx, k, m, lens, masks, origs, seed=11, single=False), [RS_OK] * 5)
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]


# ---- the Python mirror ------------------------------------------------------------------------

def _raised(f):
    try:
        return f(), None
    except Exception as e:  # noqa: BLE001 - compared with the batch's error object
        return None, e


@pytest.mark.gpu
def test_python_error_identity():
    """errors[b] of encode_many / decode_many has the class and text Codec.encode / Codec.decode
    raise for that object alone; results and the mutation of the shard lists agree too."""
    Nat, E, _ = _env()
    codec = E.Codec(Nat.default_context())
    k, m = 4, 2
    n, prof = k + m, E.ErasureProfile(4, 2)
    rng = np.random.default_rng(5)
    datas = [b"", rng.integers(0, 256, 1001, dtype=np.uint8).tobytes(), b"hi", bytearray(b"x" * 4096)]
    shards, errors = codec.encode_many(datas, prof)
    assert len(shards) == len(errors) == len(datas)
    for b, d in enumerate(datas):
        got, err = _raised(lambda: codec.encode(d, prof))
        if err is None:
            assert errors[b] is None and [bytes(s) for s in shards[b]] == [bytes(s) for s in got]
        else:
            assert shards[b] is None and type(errors[b]) is type(err) and str(errors[b]) == str(err)
    assert isinstance(errors[0], E.ErrShortData) and errors[1] is None

    full = [[bytearray(s) for s in sh] for sh in shards[1:]]  # three healthy codewords

    def variants():
        a = [bytearray(s) for s in full[0]]
        a[0] = None
        a[5] = None
        few = [bytearray(s) for s in full[0]]
        few[0] = few[1] = few[2] = None
        bad = [bytearray(s) for s in full[2]]
        bad[1] = b""
        bad[5][100] ^= 1
        short = [bytearray(s) for s in full[0]]
        short[2] = short[2][:-1]
        return [(a, 1001), (few, 1001), (bad, 4096), ([bytearray(s) for s in full[1]], 5),
                ([None] * n, 7), (short, 1001), ([bytearray(s) for s in full[1]][:n - 1], 2),
                ([bytearray(s) for s in full[1]], 2), ([bytearray(s) for s in full[2]], 0),
                ([bytearray(s) for s in full[1]], -1)]

    batch, alone = variants(), variants()
    objects, errors = codec.decode_many([s for s, _ in batch], prof, [z for _, z in batch])
    for b, (sh, size) in enumerate(alone):
        got, err = _raised(lambda: codec.decode(sh, prof, size))
        if err is None:
            assert errors[b] is None and bytes(objects[b]) == bytes(got)
        else:
            assert objects[b] is None and type(errors[b]) is type(err) and str(errors[b]) == str(err), b
        assert [None if s is None else bytes(s) for s in batch[b][0]] == \
            [None if s is None else bytes(s) for s in sh], b
    kinds = [type(e) for e in errors]
    assert kinds[:7] == [type(None), E.ErrTooFewShards, E.ErrShardCorrupted, E.ErrInsufficientShards,
                         E.ErrShardNoData, E.ErrShardSize, E.ErrTooFewShards]
    assert kinds[7:9] == [type(None), type(None)] and kinds[9] is Nat.NativeError
    with pytest.raises(E.ErrInvalidProfile):
        codec.encode_many([b"x"], E.ErasureProfile(0, 2))
    with pytest.raises(E.ErrInvalidProfile):
        codec.decode_many([], E.ErasureProfile(4, 0), [])
    with pytest.raises(E.ErrUnsupportedProfile):
        codec.encode_many([b"x"], E.ErasureProfile(200, 100))
    assert codec.encode_many([], prof) == ([], []) and codec.decode_many([], prof, []) == ([], [])


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "child":
    _child(sys.argv[2:])
