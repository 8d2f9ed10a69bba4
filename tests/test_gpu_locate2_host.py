"""Pair locate and heal on host memory: rs_locate_batch_ex with max_errors
= 2 gives the pair device plan's counts over the same bytes, column parts of a chunked stripe
included; rs_heal_batch_ex, rs_codec_decode_heal_ex and Codec.decode_heal(max_errors=2) repair
stripes in which shards are corrupt in the same byte columns, two per column, where the single
calls answer RS_E_CORRUPT. Expected values are what the test corrupted and the C oracle's
encode."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stripe(k, m, S, seed):
    """n writable shards of a consistent stripe."""
    rng = np.random.default_rng(seed)
    data = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
    par = cref.encode(data, k, m)
    return [bytearray(d.tobytes()) for d in data] + [bytearray(np.asarray(p).tobytes()) for p in par]


def _flip(shard, cols, seed=1):
    rng = np.random.default_rng(seed)
    for c in cols:
        shard[c] ^= int(rng.integers(1, 256))


def _copy(st):
    return [[None if s is None else bytearray(s) for s in row] for row in st]


_CHUNK_CHILD = r"""
import sys
import numpy as np
import torch
from oracle import cref
from callfs_amd import _native as N
from callfs_amd.device import Plan, RaggedBatch
from callfs_amd.erasure import host_counters, locate, locate_batch

k, m, n = 10, 4, 14
sizes = [40000, 9, 8192 + 21, 100, 16, 70001]
lost = [(), (3,), (), (1, 2, 5, 12), (), (11,)]
rng = np.random.default_rng(9)
stripes = []
for S in sizes:
    data = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
    par = cref.encode(data, k, m)
    stripes.append([np.array(x, dtype=np.uint8) for x in data] + [np.array(p, dtype=np.uint8) for p in par])
# 14 shards of 40,000 bytes do not fit a 256 KiB chunk: stripe 0 is cut into column parts at
# multiples of 8,192 bytes; two shards are corrupt in the same columns on both sides of every
# possible cut
cuts = [c for c in range(8192, 40000, 8192)]
both = [0] + [c - 1 for c in cuts] + cuts + [39999]
hits = {(0, 4): both + [5], (0, 12): both + [77, 78],
        (2, 0): [8191, 8192, 8212], (2, 13): [8191, 8192, 8212],
        (4, 6): [15], (4, 7): [15]}
exp = np.zeros((len(sizes), n + 1), dtype=np.uint64)
for (b, i), cols in hits.items():
    for c in cols:
        stripes[b][i][c] ^= 0x31 + i
    exp[b, i] = len(cols)
# stripe 5 has r' = 3: a same-column pair is unexplained, a single is blamed
for i in (0, 13):
    stripes[5][i][70000] ^= 0x55
stripes[5][2][1001] ^= 1
exp[5, n] = 1
exp[5, 2] = 1
host = [[None if i in lost[b] else stripes[b][i] for i in range(n)] for b in range(len(sizes))]
c0 = host_counters()
counts, status = locate_batch(host, k, m, max_errors=2)
c1 = host_counters()
bad = 0
if not np.array_equal(counts, exp):
    print("host counts", np.argwhere(counts != exp)[:8].tolist())
    bad += 1
C = N.RS_E_CORRUPT
if status != [C, 0, C, 0, C, C]:
    print("status", status)
    bad += 1
if c1["calls"] - c0["calls"] != 1 or c1["chunks"] - c0["chunks"] < 3 or \
        c1["launches"] - c0["launches"] != c1["chunks"] - c0["chunks"]:
    print("counters", c0, c1)
    bad += 1
# the pair device plan over the same bytes
rb = RaggedBatch(k, m, sizes, torch.device("cuda:0"))
masks = [[i not in lost[b] for i in range(n)] for b in range(len(sizes))]
for b in range(len(sizes)):
    for i in range(n):
        rb.shard(b, i).copy_(torch.from_numpy(stripes[b][i]))
plan = Plan.for_ragged(rb, present=masks, locate=True, max_errors=2)
plan.launch()
dev = plan.blame()
plan.close()
if not np.array_equal(dev, counts):
    print("device counts differ", np.argwhere(dev != counts)[:8].tolist())
    bad += 1
one = locate(host[0], k, m, max_errors=2)
if not np.array_equal(one, exp[0]):
    print("rs_locate_ex", one.tolist())
    bad += 1
# max_errors = 1 over the same bytes: the single call's counts
old, st_old = locate_batch(host, k, m)
one1, st1 = locate_batch(host, k, m, max_errors=1)
if not np.array_equal(old, one1) or st_old != st1 or int(old[0, n]) != len(both) or int(old[0, 4]) != 1:
    print("max_errors=1", old[0].tolist(), one1[0].tolist())
    bad += 1
print("chunked pair locate child:", "ok" if not bad else "%d mismatches" % bad)
sys.exit(1 if bad else 0)
"""


def test_locate_batch_ex_chunked_matches_device_plan(native_lib):
    """CALLFS_RS_CHUNK_BYTES is read once per process: a fresh child with 256 KiB chunks."""
    env = dict(os.environ)
    env["CALLFS_RS_CHUNK_BYTES"] = str(256 << 10)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _CHUNK_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "chunked pair locate child: ok" in r.stdout


def test_heal_batch_ex(native_lib):
    from callfs_amd import _native as N
    from callfs_amd.erasure import heal_batch
    k, m, n = 10, 4, 14
    C = N.RS_E_CORRUPT
    sizes = [8192 + 37, 5000, 300, 16]
    full = [_stripe(k, m, S, 70 + b) for b, S in enumerate(sizes)]
    st = _copy(full)
    # 0: two shards corrupt in overlapping columns (a valid and a compared one)
    _flip(st[0][2], [0, 17, 8191, 8192, sizes[0] - 1] + list(range(100, 164)), 2)
    _flip(st[0][12], [17, 8192, sizes[0] - 1, 4000] + list(range(132, 200)), 3)
    # 1: three shards corrupt in pairwise-overlapping, never triply-overlapping columns:
    # present - |B| = k + 1
    _flip(st[1][0], list(range(0, 40)) + list(range(1000, 1040)), 4)
    _flip(st[1][5], list(range(20, 40)) + list(range(2000, 2040)) + [4999], 5)
    _flip(st[1][13], list(range(1000, 1020)) + list(range(2020, 2040)) + [4999], 6)
    # 2: clean; 3: one corrupt shard (the single rule's verdict)
    _flip(st[3][7], [15], 7)
    probe = _copy(st)
    status, healed = heal_batch(probe, k, m)
    assert status == [C, C, 0, 0] and healed == [[], [], [], [7]]
    before = _copy(st)
    status, healed = heal_batch(st, k, m, max_errors=2)
    assert status == [0, 0, 0, 0]
    assert healed == [[2, 12], [0, 5, 13], [], [7]]
    for b in range(len(sizes)):
        assert [bytes(s) for s in st[b]] == [bytes(s) for s in full[b]], b
    # max_errors = 1 is the old call
    one = _copy(before)
    status1, healed1 = heal_batch(one, k, m, max_errors=1)
    assert status1 == [C, C, 0, 0] and healed1 == [[], [], [], [7]]


def test_heal_rs106_one_missing_two_corrupt(native_lib):
    from callfs_amd import _native as N
    from callfs_amd.erasure import heal_batch
    k, m, n = 10, 6, 16
    S = 8192 + 5
    full = _stripe(k, m, S, 90)
    st = [[bytearray(s) for s in full]]
    st[0][4] = None
    cols = [0, 15, 16, 4095, 8191, 8192, S - 1]
    _flip(st[0][0], cols, 2)
    _flip(st[0][11], cols + [77], 3)
    probe = _copy(st)
    status, healed = heal_batch(probe, k, m)
    assert status == [N.RS_E_CORRUPT] and healed == [[]]
    status, healed = heal_batch(st, k, m, max_errors=2)
    assert status == [0] and healed == [[0, 11]]
    assert [bytes(s) for s in st[0]] == [bytes(s) for s in full]


def test_rs63_pair_stays_corrupt(native_lib):
    """r' = 3: a same-column pair is beyond a pair plan too; present shards are not written."""
    from callfs_amd import _native as N
    from callfs_amd.erasure import heal_batch, locate
    k, m, n = 6, 3, 9
    full = _stripe(k, m, 3000, 91)
    for me in (1, 2):
        st = [[bytearray(s) for s in full]]
        _flip(st[0][1], [17, 2999], 2)
        _flip(st[0][7], [17, 2999], 3)
        before = [bytes(s) for s in st[0]]
        counts = locate(st[0], k, m, max_errors=me)
        assert int(counts[n]) == 2 and not counts[:n].any()
        status, healed = heal_batch(st, k, m, max_errors=me)
        assert status == [N.RS_E_CORRUPT] and healed == [[]]
        assert [bytes(s) for s in st[0]] == before


def test_decode_heal_max_errors(native_lib):
    import ctypes
    from callfs_amd import (Codec, ErasureProfile, ErrInsufficientShards, ErrShardCorrupted,
                            ErrShardNoData, ErrShardSize, ErrTooFewShards)
    from callfs_amd import _native as N
    codec = Codec()
    p = ErasureProfile(10, 4)
    data = np.random.default_rng(3).integers(0, 256, 123_457, dtype=np.uint8).tobytes()
    full = [bytes(s) for s in codec.encode(data, p)]
    S = len(full[0])

    def damaged():
        sh = [bytearray(s) for s in full]
        _flip(sh[1], [5, 1000, S - 1], 2)
        _flip(sh[11], [5, 1000, S - 1, 9], 3)
        return sh

    with pytest.raises(ErrShardCorrupted):
        codec.decode_heal(damaged(), p, len(data))
    with pytest.raises(ErrShardCorrupted):
        codec.decode_heal(damaged(), p, len(data), max_errors=1)
    sh = damaged()
    out, healed = codec.decode_heal(sh, p, len(data), max_errors=2)
    assert bytes(out) == data and healed == [1, 11]
    assert [bytes(s) for s in sh] == full
    # one corrupt and one missing shard, clean: as decode_heal()
    sh = [bytearray(s) for s in full]
    _flip(sh[3], [0, S - 1])
    sh[0] = None
    out, healed = codec.decode_heal(sh, p, len(data), max_errors=2)
    assert bytes(out) == data and healed == [3] and [bytes(s) for s in sh] == full
    sh = [None if i == 2 else bytearray(s) for i, s in enumerate(full)]
    out, healed = codec.decode_heal(sh, p, len(data), max_errors=2)
    assert bytes(out) == data and healed == [] and bytes(sh[2]) == full[2]
    # every other error precedes as in decode_heal()
    p42 = ErasureProfile(4, 2)
    s42 = [bytearray(s) for s in codec.encode(b"x" * 100, p42)]
    with pytest.raises(ErrInsufficientShards):
        codec.decode_heal([bytearray(s) for s in s42], p42, 101, max_errors=2)
    with pytest.raises(ErrShardNoData):
        codec.decode_heal([None] * 6, p42, 10, max_errors=2)
    bad = [bytearray(s) for s in s42]
    bad[1] = bad[1][:-1]
    with pytest.raises(ErrShardSize):
        codec.decode_heal(bad, p42, 100, max_errors=2)
    with pytest.raises(ErrTooFewShards):
        codec.decode_heal([None, None, None] + s42[3:], p42, 100, max_errors=2)
    for me, code in ((0, N.RS_E_ARG), (3, N.RS_E_UNSUPPORTED)):
        with pytest.raises(N.NativeError) as ei:
            codec.decode_heal([bytearray(s) for s in full], p, len(data), max_errors=me)
        assert ei.value.code == code
    # the C call itself
    sh = damaged()
    n = 14
    ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof((ctypes.c_char * len(s)).from_buffer(s)) for s in sh])
    lens = (ctypes.c_size_t * n)(*[len(s) for s in sh])
    out = bytearray(len(data))
    healed = (ctypes.c_uint8 * n)()
    rc = N.lib.rs_codec_decode_heal_ex(N.default_context().handle, 10, 4, ptrs, lens,
                                       ctypes.addressof((ctypes.c_char * len(out)).from_buffer(out)),
                                       len(data), healed, 2)
    assert rc == 0 and list(healed) == [int(i in (1, 11)) for i in range(n)]
    assert bytes(out) == data and [bytes(s) for s in sh] == full


def test_statuses_equal_the_single_calls(native_lib):
    from callfs_amd import _native as N
    from callfs_amd.erasure import heal_batch, host_counters, locate, locate_batch, reconstruct_batch
    k, m, n = 4, 2, 6

    def stripes():
        good = _stripe(k, m, 50, 1)
        short = _stripe(k, m, 50, 2)
        short[2] = short[2][:-1]
        few = [None, None, None] + _stripe(k, m, 50, 3)[3:]
        bad = _stripe(k, m, 50, 4)
        bad[5][49] ^= 1
        return [good, [None] * n, short, few, bad, _stripe(k, m, 50, 5)[:4] + [None, None]]

    counts, status = locate_batch(stripes(), k, m, max_errors=2)
    c1, s1 = locate_batch(stripes(), k, m)
    assert status == s1 == reconstruct_batch(stripes(), k, m, verify=True)
    assert status == [0, N.RS_E_NO_DATA, N.RS_E_SHARD_SIZE, N.RS_E_TOO_FEW_SHARDS, N.RS_E_CORRUPT, 0]
    assert np.array_equal(counts, c1) and int(counts[4, 5]) == 1 and int(counts.sum()) == 1
    hs2, hl2 = heal_batch(stripes(), k, m, max_errors=2)
    hs1, hl1 = heal_batch(stripes(), k, m)
    assert hs2 == hs1 and hl2 == hl1
    # exactly k present: zero counts, RS_OK, no device work
    c0 = host_counters()
    only_k = _stripe(k, m, 50, 6)[:4] + [None, None]
    assert not locate(only_k, k, m, max_errors=2).any()
    counts, status = locate_batch([only_k, list(only_k)], k, m, max_errors=2)
    assert status == [0, 0] and not counts.any()
    assert host_counters() == c0
    for me, code in ((0, N.RS_E_ARG), (3, N.RS_E_UNSUPPORTED)):
        with pytest.raises(N.NativeError) as ei:
            locate(only_k, k, m, max_errors=me)
        assert ei.value.code == code
