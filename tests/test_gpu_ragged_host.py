"""Heterogeneous host batches: rs_encode_batch / rs_reconstruct_batch over stripes of different
shard sizes and erasure patterns run as one ragged pipeline.

Every result is compared byte for byte with the CPU oracle (oracle.cref), stripe by stripe.
The scenarios below run in this process with the default settings -- where their staging is
under CALLFS_RS_SMALL_MAX_BYTES they take the one-dispatch in-place transport
(rs_apply_small_ragged) -- and again in fresh child processes whose environment selects
another transport or path (the settings are read once per process): the staged transport
(CALLFS_RS_SMALL_MAX_BYTES=0), column cuts over many chunks (CALLFS_RS_CHUNK_BYTES=65536, with
and without CALLFS_RS_INPLACE_PIPELINE=1), the per-group path (CALLFS_RS_RAGGED_BATCH=0) and the
nibble-table fallback (CALLFS_RS_BITSLICE=0). A child prints one JSON line of named checks.

Counters: tables are cached per lane, so a call that must upload none (`copies` rising by 0)
is measured on a context of one device after a first call of the same profile and patterns.

  python tests/test_gpu_ragged_host.py child <scenario> ...     # what a child runs
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

RS_OK, RS_E_TOO_FEW, RS_E_SHARD_SIZE, RS_E_CORRUPT = 0, -3, -4, -6
SENT = 32  # sentinel bytes after every buffer the library may write

SIZES_A = [1, 5, 15, 16, 17, 40, 4095, 4096, 4097, 8191, 8192, 8193, 8208, 2 * 8192 + 83]
SIZES_ROWS = [17, 8193, 20000]
SIZES_CUTS = [100_003, 700, 40_003, 16, 9]
SIZES_SMALL = [1 + 97 * b for b in range(32)]
SIZES_COUNT = [1 + 331 * b for b in range(64)]


def _env():
    sys.path.insert(0, ROOT)
    from callfs_amd import _native as Nat
    from callfs_amd import erasure
    from oracle import cref
    return Nat, erasure, cref


@functools.lru_cache(maxsize=None)
def _codewords(k, m, sizes, seed):
    """Full codewords (n arrays per stripe) from the oracle; shared, never written."""
    _, _, cref = _env()
    rng = np.random.default_rng(seed)
    out = []
    for S in sizes:
        data = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
        full = data + [np.ascontiguousarray(p) for p in cref.encode(data, k, m)]
        for a in full:
            a.setflags(write=False)
        out.append(full)
    return out


def _buf(S, fill=0xA5):
    return np.full(S + SENT, fill, np.uint8)


def _ptr_array(ptrs):
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)


def _counters(Nat, ctx):
    c = Nat.HostCounters()
    assert Nat.lib.rs_host_counters_read(ctx, ctypes.byref(c)) == 0
    return {n: int(getattr(c, n)) for n, _ in c._fields_}


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def encode_case(Nat, ctx, k, m, sizes, seed=1, alloc=None):
    """One rs_encode_batch; `alloc(nbytes)` gives a writable uint8 array (default numpy)."""
    cw = _codewords(k, m, tuple(sizes), seed)
    alloc = alloc or (lambda nb: np.empty(nb, np.uint8))
    data, par = [], []
    for st, S in zip(cw, sizes):
        for i in range(k):
            a = alloc(S + SENT)
            a[:S] = st[i]
            a[S:] = 0x3C
            data.append(a)
        for _ in range(m):
            a = alloc(S + SENT)
            a[:] = 0xA5
            par.append(a)
    B = len(sizes)
    status = (ctypes.c_int * B)(*[77] * B)
    c0 = _counters(Nat, ctx)
    rc = Nat.lib.rs_encode_batch(ctx, k, m, B, (ctypes.c_size_t * B)(*sizes),
                                 _ptr_array([a.ctypes.data for a in data]),
                                 _ptr_array([a.ctypes.data for a in par]), status)
    d = _delta(c0, _counters(Nat, ctx))
    ok_bytes = all(np.array_equal(par[b * m + j][:S], cw[b][k + j])
                   for b, S in enumerate(sizes) for j in range(m))
    sentinels = all((par[b * m + j][S:] == 0xA5).all() for b, S in enumerate(sizes) for j in range(m))
    inputs = all(np.array_equal(data[b * k + i][:S], cw[b][i]) and (data[b * k + i][S:] == 0x3C).all()
                 for b, S in enumerate(sizes) for i in range(k))
    return {"rc": rc, "status": list(status), "bytes": ok_bytes, "sentinels": sentinels,
            "inputs": inputs, "counters": d}


def recon_case(Nat, ctx, k, m, sizes, masks, verify, seed=1, flips=(), wrong_len=(), junk_extra=False,
               alloc=None):
    """One rs_reconstruct_batch. masks[b]: the missing shard indices of stripe b. flips:
    (stripe, shard, byte) flipped in a present shard. wrong_len: (stripe, shard) given a length
    one less. junk_extra: every present shard beyond the first k present is overwritten with
    junk (verify off must not look at it). Returns statuses, rc and per-stripe checks."""
    n = k + m
    cw = _codewords(k, m, tuple(sizes), seed)
    alloc = alloc or (lambda nb: np.empty(nb, np.uint8))
    B = len(sizes)
    bufs, lens = [], (ctypes.c_size_t * (B * n))()
    junked = set()
    for b, S in enumerate(sizes):
        seen = 0
        for i in range(n):
            a = alloc(S + SENT)
            a[S:] = 0xA5
            if i in masks[b]:
                a[:S] = 0x5A
                lens[b * n + i] = 0
            else:
                a[:S] = cw[b][i]
                lens[b * n + i] = S
                seen += 1
                if junk_extra and seen > k:
                    a[:S] ^= 0xFF
                    junked.add((b, i))
            bufs.append(a)
    for b, i, at in flips:
        bufs[b * n + i][at] ^= 0x10
    for b, i in wrong_len:
        lens[b * n + i] -= 1
    before = [a.copy() for a in bufs]
    lens0 = list(lens)
    status = (ctypes.c_int * B)(*[77] * B)
    c0 = _counters(Nat, ctx)
    rc = Nat.lib.rs_reconstruct_batch(ctx, k, m, B, _ptr_array([a.ctypes.data for a in bufs]), lens,
                                      int(verify), status)
    d = _delta(c0, _counters(Nat, ctx))
    st = list(status)
    rebuilt, untouched, lens_ok = [], [], []
    for b, S in enumerate(sizes):
        ran = st[b] in (RS_OK, RS_E_CORRUPT)
        rb, ut, lo = True, True, True
        for i in range(n):
            a = bufs[b * n + i]
            if i in masks[b] and ran:
                rb &= bool(np.array_equal(a[:S], cw[b][i]))
                ut &= bool((a[S:] == 0xA5).all())
                lo &= lens[b * n + i] == S
            else:  # present shards, and every shard of a stripe that did not run: never written
                ut &= bool(np.array_equal(a, before[b * n + i]))
                lo &= lens[b * n + i] == lens0[b * n + i]
        rebuilt.append(rb)
        untouched.append(ut)
        lens_ok.append(lo)
    return {"rc": rc, "status": st, "rebuilt": all(rebuilt), "untouched": all(untouched),
            "lens": all(lens_ok), "counters": d}


def _masks_a(k, m, count):
    """A mask per stripe of RS(k, m) with m >= 2: data-only, parity-only and mixed losses, one
    stripe with nothing missing, at least five distinct patterns."""
    n = k + m
    base = [(0,), (k,), (0, k), (), (1, 2), (n - 1,), (k - 1, n - 1), (2,)]
    return [base[b % len(base)] for b in range(count)]


# ---- scenarios: each returns a dict of named results ------------------------------------------

def sc_encode_a(Nat, ctx):
    return {"enc": encode_case(Nat, ctx, 10, 4, SIZES_A)}


def sc_recon_a(Nat, ctx):
    k, m, n = 10, 4, 14
    masks = [list(x) for x in _masks_a(k, m, len(SIZES_A))]
    # stripe 6 (S 4095, mask (k-1, n-1)): flipped byte in a compared shard, vector part
    # stripe 13 (S 16467, mask (n-1,)): flipped byte in its S % 16 tail
    # stripe 9 (S 8191): k - 1 shards; stripe 11 (S 8193): a wrong-length shard
    masks[9] = list(range(5))
    flips = [(6, 11, 1000), (13, 12, 16467 - 2)]
    r = recon_case(Nat, ctx, k, m, SIZES_A, masks, True, flips=flips, wrong_len=[(11, 5)])
    r["distinct_patterns"] = len({tuple(x) for b, x in enumerate(masks) if b not in (9, 11)})
    return {"rec": r}


def sc_recon_noverify(Nat, ctx):
    k, m = 10, 4
    sizes = [17, 4097, 8193, 40, 16467, 8192, 5]
    masks = [(0,), (1, 11), (0, 3, 7, 12), (13,), (2, 9), (), (4, 5, 6, 10)]
    return {"nov": recon_case(Nat, ctx, k, m, sizes, masks, False, junk_extra=True)}


def sc_rows(Nat, ctx):
    out = {}
    for k, m in [(10, 8), (20, 12), (10, 20), (1, 3), (3, 2)]:
        n = k + m
        out[f"enc_{k}_{m}"] = encode_case(Nat, ctx, k, m, SIZES_ROWS, seed=k * 100 + m)
        masks = [(0,), tuple(range(n - m, n)), (k - 1, n - 1) if m >= 2 else (n - 1,)]
        out[f"rec_{k}_{m}"] = recon_case(Nat, ctx, k, m, SIZES_ROWS, masks, True, seed=k * 100 + m)
    return out


def sc_cuts(Nat, ctx):
    k, m = 4, 2
    enc = encode_case(Nat, ctx, k, m, SIZES_CUTS, seed=7)
    masks = [(1,), (0, 5), (4,), (2, 3), ()]
    # stripe 0's parts are 8,192 wide at this budget: byte 9,000 of compared shard 5 lies in
    # the second part
    rec = recon_case(Nat, ctx, k, m, SIZES_CUTS, masks, True, seed=7, flips=[(0, 5, 9000)])
    return {"enc": enc, "rec": rec}


def sc_small(Nat, ctx):
    k, m, n = 10, 4, 14
    out = {"enc": encode_case(Nat, ctx, k, m, SIZES_SMALL, seed=3)}
    # two calls in a row: the sequence number and the block counter are reused, and the
    # second finds its tables cached on the lane
    out["enc2"] = encode_case(Nat, ctx, k, m, SIZES_SMALL, seed=3)
    masks = [((b % n),) if b % 3 else ((b % n), (b * 5 + 1) % n) for b in range(32)]
    masks = [tuple(sorted(set(x))) for x in masks]
    # stripe 20 (S 1941): mask (6,); shard 13 is compared
    out["rec"] = recon_case(Nat, ctx, k, m, SIZES_SMALL, masks, True, seed=3, flips=[(20, 13, 1900)])
    out["r1"] = recon_case(Nat, ctx, 16, 4, [100, 3000, 17, 900], [(0,), (5,), (19,), (16,)], False, seed=4)
    sizes = [33, 2000, 5000]
    out["enc_20_12"] = encode_case(Nat, ctx, 20, 12, sizes, seed=5)
    out["rec_20_12"] = recon_case(Nat, ctx, 20, 12, sizes, [(0, 1, 2), tuple(range(20, 32)), (31,)], True, seed=5)
    return out


def sc_uniform(Nat, ctx):
    return {"enc": encode_case(Nat, ctx, 10, 4, [1000] * 8, seed=6),
            "rec": recon_case(Nat, ctx, 10, 4, [1000] * 8, [(2,)] * 8, True, seed=6)}


def sc_count_staged(Nat, ctx):
    return {"enc": encode_case(Nat, ctx, 10, 4, SIZES_COUNT, seed=8)}


SCENARIOS = {f.__name__[3:]: f for f in (sc_encode_a, sc_recon_a, sc_recon_noverify, sc_rows, sc_cuts,
                                         sc_small, sc_uniform, sc_count_staged)}


def _run(names, Nat=None, ctx=None):
    if Nat is None:
        Nat, _, _ = _env()
    ctx = ctx or Nat.default_context().handle
    return {n: SCENARIOS[n](Nat, ctx) for n in names}


def _child(names):
    Nat, _, _ = _env()
    one = Nat.Context(1)  # one device: counters of consecutive calls see one lane's caches
    print(json.dumps(_run(names, Nat, one.handle)))


@functools.lru_cache(maxsize=None)
def _spawn(names, env_items):
    env = dict(os.environ, **dict(env_items))
    for name in ("CALLFS_RS_CHUNK_BYTES", "CALLFS_RS_SMALL_MAX_BYTES", "CALLFS_RS_INPLACE_PIPELINE",
                 "CALLFS_RS_RAGGED_BATCH", "CALLFS_RS_BITSLICE"):
        if name not in dict(env_items):
            env.pop(name, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", *names], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.splitlines()[-1])


def _staged():
    return _spawn(("encode_a", "recon_a", "recon_noverify", "rows", "small", "count_staged"),
                  (("CALLFS_RS_SMALL_MAX_BYTES", "0"),))


def _toggle_off():
    return _spawn(("encode_a", "recon_a", "small"), (("CALLFS_RS_RAGGED_BATCH", "0"),))


@pytest.fixture(scope="module")
def here():
    """The scenarios in this process, default settings, on a context of one device."""
    Nat, _, _ = _env()
    ctx = Nat.Context(1)
    yield _run(("encode_a", "recon_a", "recon_noverify", "rows", "small", "uniform", "count_staged"),
               Nat, ctx.handle)
    ctx.close()


def _check_enc(r, count):
    assert r["rc"] == RS_OK and r["status"] == [RS_OK] * count
    assert r["bytes"], "parity != oracle"
    assert r["sentinels"], "bytes after a parity buffer were written"
    assert r["inputs"], "an input buffer changed"


def _check_rec(r, want_status):
    assert r["status"] == want_status
    assert r["rc"] == next((s for s in want_status if s), RS_OK)
    assert r["rebuilt"], "a rebuilt shard != oracle"
    assert r["untouched"], "a present shard, an unrun stripe or a sentinel was written"
    assert r["lens"], "lens changed for a shard that was not rebuilt (or not for one that was)"


def _want_recon_a():
    want = [RS_OK] * len(SIZES_A)
    want[6] = want[13] = RS_E_CORRUPT
    want[9] = RS_E_TOO_FEW
    want[11] = RS_E_SHARD_SIZE
    return want


# ---- shape cases ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("where", ["inplace", "staged", "toggle_off"])
def test_encode_mixed_sizes(here, where):
    r = {"inplace": lambda: here, "staged": _staged, "toggle_off": _toggle_off}[where]()["encode_a"]["enc"]
    _check_enc(r, len(SIZES_A))
    assert r["counters"]["ragged_calls"] == (0 if where == "toggle_off" else 1)
    assert r["counters"]["calls"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["inplace", "staged", "toggle_off"])
def test_reconstruct_verify_mask_per_stripe(here, where):
    r = {"inplace": lambda: here, "staged": _staged, "toggle_off": _toggle_off}[where]()["recon_a"]["rec"]
    assert r["distinct_patterns"] >= 5
    _check_rec(r, _want_recon_a())
    assert r["counters"]["ragged_calls"] == (0 if where == "toggle_off" else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["inplace", "staged"])
def test_reconstruct_without_verify_by_missing_count(here, where):
    """Stripes with 1, 2 and 4 missing shards in one call (one stripe with none); the present
    shards beyond the first k are junk and must not be flagged."""
    r = (here if where == "inplace" else _staged())["recon_noverify"]["nov"]
    _check_rec(r, [RS_OK] * 7)
    assert r["counters"]["ragged_calls"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("k,m", [(10, 8), (20, 12), (10, 20), (1, 3), (3, 2)])
@pytest.mark.parametrize("where", ["inplace", "staged"])
def test_row_counts(here, where, k, m):
    res = (here if where == "inplace" else _staged())["rows"]
    _check_enc(res[f"enc_{k}_{m}"], 3)
    _check_rec(res[f"rec_{k}_{m}"], [RS_OK] * 3)
    # one launch per group of 16 rows per chunk
    assert res[f"enc_{k}_{m}"]["counters"]["launches"] == (m + 15) // 16


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [False, True])
def test_column_cuts_over_many_chunks(inplace):
    """CALLFS_RS_CHUNK_BYTES=65536: the 100,003- and 40,003-byte stripes of RS(4,2) become
    parts of 8,192 columns among the small stripes, over more than three chunks on three slots;
    a flipped byte in the second part of stripe 0 flags that stripe alone."""
    env = [("CALLFS_RS_CHUNK_BYTES", "65536"), ("CALLFS_RS_SMALL_MAX_BYTES", "0")]
    if inplace:
        env.append(("CALLFS_RS_INPLACE_PIPELINE", "1"))
    res = _spawn(("cuts",), tuple(env))["cuts"]
    _check_enc(res["enc"], 5)
    assert res["enc"]["counters"]["chunks"] > 3
    assert res["enc"]["counters"]["copies"] == (0 if inplace else 2 * res["enc"]["counters"]["chunks"]) + 1
    _check_rec(res["rec"], [RS_E_CORRUPT, RS_OK, RS_OK, RS_OK, RS_OK])
    assert res["rec"]["counters"]["chunks"] > 3


# ---- the small in-place path ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("where", ["inplace", "staged", "toggle_off"])
def test_small_batches(here, where):
    res = {"inplace": lambda: here, "staged": _staged, "toggle_off": _toggle_off}[where]()["small"]
    _check_enc(res["enc"], 32)
    _check_enc(res["enc2"], 32)
    want = [RS_OK] * 32
    want[20] = RS_E_CORRUPT
    _check_rec(res["rec"], want)
    if where != "toggle_off":
        _check_rec(res["r1"], [RS_OK] * 4)
        _check_enc(res["enc_20_12"], 3)
        _check_rec(res["rec_20_12"], [RS_OK] * 3)


# ---- counters ------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_counters_staged_batch_is_one_round_trip(here):
    """64 RS(10,4) stripes of sizes 1 + 331 b: about 9.3 MB of staging, one default chunk."""
    c = here["count_staged"]["enc"]["counters"]
    _check_enc(here["count_staged"]["enc"], 64)
    assert c["launches"] == 1 and c["chunks"] == 1 and c["copies"] <= 3 and c["ragged_calls"] == 1


@pytest.mark.gpu
def test_counters_small_batch_is_one_dispatch(here):
    """The second of two equal small calls (tables cached on the lane): one dispatch, no copy."""
    c = here["small"]["enc2"]["counters"]
    assert c["launches"] == 1 and c["copies"] == 0 and c["chunks"] == 1 and c["ragged_calls"] == 1
    assert here["small"]["enc"]["counters"]["launches"] == 1
    assert here["small"]["enc"]["counters"]["copies"] <= 1  # the table upload, if any


@pytest.mark.gpu
def test_counters_per_group_path_launches_per_size():
    c = _toggle_off()["small"]["enc2"]["counters"]
    assert c["launches"] == 32 and c["ragged_calls"] == 0


@pytest.mark.gpu
def test_uniform_batch_keeps_its_path(here):
    for name, count in (("enc", 8), ("rec", 8)):
        assert here["uniform"][name]["counters"]["ragged_calls"] == 0
        assert here["uniform"][name]["counters"]["calls"] == 1
    _check_enc(here["uniform"]["enc"], 8)
    _check_rec(here["uniform"]["rec"], [RS_OK] * 8)


# ---- direct path -------------------------------------------------------------------------------

@pytest.mark.gpu
def test_direct_on_pinned_buffers():
    """Every buffer from rs_host_alloc, eight stripes of 60,000..200,000 bytes: the kernels run
    on the caller's bytes (no chunk staging: copies are the metadata, the tables and the status
    words), bit-exact, sentinels inside the allocation intact."""
    Nat, _, _ = _env()
    ctx = Nat.Context(1)
    pins = [Nat.PinnedBuffer(48 << 20, ctx)]
    at = [0]

    def alloc(nb):  # carved from one allocation, 16-B aligned, the sentinels inside it
        a = pins[0].array[at[0]:at[0] + nb]
        at[0] += (nb + 15) // 16 * 16
        assert at[0] <= pins[0].nbytes
        return a

    sizes = [60_000 + 20_000 * b + (b % 3) for b in range(8)]
    k, m = 10, 4
    try:
        enc = encode_case(Nat, ctx.handle, k, m, sizes, seed=9, alloc=alloc)
        _check_enc(enc, 8)
        assert enc["counters"] == {"calls": 1, "chunks": 1, "launches": 1, "copies": 2, "ragged_calls": 1}
        masks = [(b % 14,) if b % 2 else (b % 14, (b + 3) % 14) for b in range(8)]
        rec = recon_case(Nat, ctx.handle, k, m, sizes, masks, True, seed=9, flips=[(3, 13, 70_001)],
                         alloc=alloc)
        want = [RS_OK] * 8
        want[3] = RS_E_CORRUPT
        _check_rec(rec, want)
        assert rec["counters"]["chunks"] == 1 and rec["counters"]["launches"] == 1
        assert rec["counters"]["copies"] <= 3
    finally:
        for p in pins:
            p.close()
        ctx.close()


# ---- concurrency, fallback ---------------------------------------------------------------------

@pytest.mark.gpu
def test_eight_threads_on_one_context():
    Nat, _, _ = _env()
    ctx = Nat.default_context().handle
    sizes = [7, 300, 4097, 9000, 33]
    masks = [(0,), (1, 12), (), (13,), (3, 4)]
    _codewords(10, 4, tuple(sizes), 11)  # shared reference, computed once
    errors = []

    def work(t):
        try:
            for _ in range(3):
                _check_enc(encode_case(Nat, ctx, 10, 4, sizes, seed=11), 5)
                rot = masks[t % 5:] + masks[:t % 5]
                _check_rec(recon_case(Nat, ctx, 10, 4, sizes, rot, bool(t & 1), seed=11), [RS_OK] * 5)
        except BaseException as e:  # noqa: BLE001 - reported by the main thread
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors[0]


@pytest.mark.gpu
def test_nibble_fallback_setting_does_not_reach_the_ragged_path():
    """CALLFS_RS_BITSLICE=0: a heterogeneous call runs the ragged kernels as always (they have
    no bit-sliced form and ask for no compile)."""
    res = _spawn(("encode_a", "recon_a"), (("CALLFS_RS_BITSLICE", "0"),))
    _check_enc(res["encode_a"]["enc"], len(SIZES_A))
    _check_rec(res["recon_a"]["rec"], _want_recon_a())
    assert res["encode_a"]["enc"]["counters"]["ragged_calls"] == 1


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "child":
    _child(sys.argv[2:])
