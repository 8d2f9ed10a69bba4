"""Correct on host memory: rs_correct / rs_correct_batch leave the bytes,
counts and statuses of the device plan over the same bytes, column parts of a chunked stripe
included, and copy back only the shards they changed; rs_codec_decode_correct and
Codec.decode_correct decode what decode and decode_heal refuse. Expected values are what the
test corrupted and the C oracle's encode."""
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


_CHUNK_CHILD = r"""
import sys
import numpy as np
import torch
from oracle import cref
from callfs_amd import _native as N
from callfs_amd.device import Plan, RaggedBatch
from callfs_amd.erasure import correct, correct_batch, host_counters, locate_batch

k, m, n = 10, 4, 14
sizes = [40000, 9, 8192 + 21, 100, 16, 70001, 3000]
lost = [(), (3,), (0, 13), (1, 2, 5, 12), (), (11,), ()]
rng = np.random.default_rng(9)
pristine = []
for S in sizes:
    data = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
    par = cref.encode(data, k, m)
    pristine.append([np.array(x, dtype=np.uint8) for x in data] + [np.array(p, dtype=np.uint8) for p in par])
stripes = [[s.copy() for s in st] for st in pristine]
# 14 shards of 40,000 bytes do not fit a 256 KiB chunk: stripe 0 is cut into column parts at
# multiples of 8,192 bytes; corrupt it on both sides of every possible cut
cuts = [c for c in range(8192, 40000, 8192)]
hits = {(0, 4): [0] + [c - 1 for c in cuts] + [39999], (0, 12): cuts + [5],
        (2, 7): [8191, 8192, 8212],                       # r' = 2: counted, not written
        (5, 0): list(range(0, 70001, 1001)), (5, 13): [70000],   # r' = 3
        (5, 2): [33, 50000], (5, 9): [33, 50000],         # two shards in the same columns: left
        (3, 0): [7],                                      # exactly k present: no device work
        (6, 1): [0, 2999]}
exp = np.zeros((len(sizes), n + 1), dtype=np.uint64)
want = [[s.copy() for s in st] for st in pristine]
for (b, i), cols in hits.items():
    for c in cols:
        stripes[b][i][c] ^= 0x31
for b in range(len(sizes)):
    for i in range(n):
        if i in lost[b]:
            stripes[b][i][:] = rng.integers(0, 256, sizes[b], dtype=np.uint8)  # junk, never read
            want[b][i] = stripes[b][i].copy()
exp[0, 4], exp[0, 12] = len(hits[(0, 4)]), len(hits[(0, 12)])
exp[2, n] = 3
want[2][7] = stripes[2][7].copy()
exp[5, 0], exp[5, 13], exp[5, n] = len(hits[(5, 0)]), 1, 2
want[5][2], want[5][9] = stripes[5][2].copy(), stripes[5][9].copy()
want[3][0] = stripes[3][0].copy()
exp[6, 1] = 2
damaged = [[s.copy() for s in st] for st in stripes]
host = [[None if i in lost[b] else stripes[b][i] for i in range(n)] for b in range(len(sizes))]
_, loc_status = locate_batch(host, k, m)
c0 = host_counters()
counts, status = correct_batch(host, k, m)
c1 = host_counters()
bad = 0
if not np.array_equal(counts, exp):
    print("host counts", np.argwhere(counts != exp)[:8].tolist())
    bad += 1
C = N.RS_E_CORRUPT
if status != [0, 0, C, 0, 0, C, 0] or loc_status != [C, 0, C, 0, 0, C, C]:
    print("status", status, loc_status)
    bad += 1
for b in range(len(sizes)):
    for i in range(n):
        if not np.array_equal(stripes[b][i], want[b][i]):
            print("bytes", b, i, np.flatnonzero(stripes[b][i] != want[b][i])[:8].tolist())
            bad += 1
chunks = c1["chunks"] - c0["chunks"]
# per chunk one H2D and one D2H of status words and counts; beside them one D2H per (part, shard)
# that was changed: stripe 0's shards 4 and 12 in every part they were damaged in, stripe 5's
# shards 0 and 13 likewise, stripe 6's shard 1; and at most one upload of tables
if c1["calls"] - c0["calls"] != 1 or chunks < 3 or c1["launches"] - c0["launches"] != chunks:
    print("counters", c0, c1)
    bad += 1
back = c1["copies"] - c0["copies"] - 2 * chunks
if not 5 <= back <= 5 + 2 * (len(cuts) + 1) + 2 * 9 + 1:
    print("copies back", back, c0, c1)
    bad += 1
# the device plan over the same damaged bytes
rb = RaggedBatch(k, m, sizes, torch.device("cuda:0"))
masks = [[i not in lost[b] for i in range(n)] for b in range(len(sizes))]
for b in range(len(sizes)):
    for i in range(n):
        rb.shard(b, i).copy_(torch.from_numpy(damaged[b][i]))
plan = Plan.correct(k, m, sizes, rb.pointers(), present=masks)
plan.launch()
dev = plan.blame()
flagged = plan.corrupt_stripes()
plan.close()
if not np.array_equal(dev, counts):
    print("device counts differ", np.argwhere(dev != counts)[:8].tolist())
    bad += 1
if flagged != [b for b, s in enumerate(loc_status) if s == C]:
    print("device flags", flagged)
    bad += 1
for b in range(len(sizes)):
    for i in range(n):
        if not np.array_equal(rb.shard(b, i).cpu().numpy(), stripes[b][i]):
            print("device bytes differ", b, i)
            bad += 1
# a second call over the repaired stripes: the leftovers again, nothing copied back
c2 = host_counters()
counts2, status2 = correct_batch(host, k, m)
c3 = host_counters()
if counts2[:, :n].any() or counts2[:, n].tolist() != exp[:, n].tolist() or status2 != status:
    print("second call", counts2.tolist(), status2)
    bad += 1
if c3["copies"] - c2["copies"] != 2 * (c3["chunks"] - c2["chunks"]):
    print("second call copied shards back", c2, c3)
    bad += 1
# rs_correct on the chunked stripe, damaged afresh
for i, cols in ((4, hits[(0, 4)]), (12, hits[(0, 12)])):
    for c in cols:
        host[0][i][c] ^= 0x77
one = correct(host[0], k, m)
if not np.array_equal(one, exp[0]) or any(not np.array_equal(host[0][i], pristine[0][i]) for i in range(n)):
    print("rs_correct", one.tolist())
    bad += 1
print("chunked correct child:", "ok" if not bad else "%d mismatches" % bad)
sys.exit(1 if bad else 0)
"""


def test_correct_batch_chunked_matches_device_plan(native_lib):
    """CALLFS_RS_CHUNK_BYTES is read once per process: a fresh child with 256 KiB chunks, on one
    device so that the copy counts are one lane's."""
    env = dict(os.environ)
    env["CALLFS_RS_CHUNK_BYTES"] = str(256 << 10)
    env["CALLFS_RS_DEVICE_MASK"] = "1"
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _CHUNK_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "chunked correct child: ok" in r.stdout


def test_clean_and_exactly_k_calls_copy_nothing_back(native_lib):
    from callfs_amd import _native as N
    from callfs_amd import erasure
    ctx = N.Context(1)  # one device: the tables stay in one lane from call to call

    def correct(*a):
        return erasure.correct(*a, context=ctx)

    def correct_batch(*a):
        return erasure.correct_batch(*a, context=ctx)

    def host_counters():
        return erasure.host_counters(ctx)

    k, m, n = 10, 4, 14
    full = [_stripe(k, m, S, 20 + b) for b, S in enumerate([5000, 17, 8192])]
    st = [[bytearray(s) for s in f] for f in full]
    st[1][3] = None
    correct_batch(st, k, m)  # the lane holds these tables from here on
    c0 = host_counters()
    counts, status = correct_batch(st, k, m)
    c1 = host_counters()
    assert status == [0, 0, 0] and not counts.any()
    chunks = c1["chunks"] - c0["chunks"]
    assert c1["calls"] - c0["calls"] == 1 and chunks >= 1
    # one H2D and one D2H of status words and counts per chunk, and not one shard row
    assert c1["copies"] - c0["copies"] == 2 * chunks
    assert [[None if s is None else bytes(s) for s in row] for row in st] == \
        [[None if i == 3 and b == 1 else bytes(s) for i, s in enumerate(f)] for b, f in enumerate(full)]
    # one damaged byte: one shard row more
    st[2][12][8191] ^= 0x40
    counts, status = correct_batch(st, k, m)
    c2 = host_counters()
    assert status == [0, 0, 0] and int(counts[2, 12]) == 1 and int(counts.sum()) == 1
    assert c2["copies"] - c1["copies"] == 2 * (c2["chunks"] - c1["chunks"]) + 1
    assert bytes(st[2][12]) == bytes(full[2][12])
    # exactly k present: zero counts, RS_OK, no device work, whatever the shards hold
    c0 = host_counters()
    only_k = [bytearray(s) for s in full[0][:k]] + [None] * m
    only_k[0][5] ^= 1
    was = [None if s is None else bytes(s) for s in only_k]
    assert not correct(only_k, k, m).any()
    counts, status = correct_batch([only_k, list(only_k)], k, m)
    assert status == [0, 0] and not counts.any()
    assert host_counters() == c0
    assert [None if s is None else bytes(s) for s in only_k] == was
    ctx.close()


def test_status_against_locate_batch(native_lib):
    """Stripe errors are rs_locate_batch's; only a stripe whose every mismatching column was
    corrected differs (RS_OK where locate says RS_E_CORRUPT)."""
    from callfs_amd import _native as N
    from callfs_amd.erasure import correct_batch, locate_batch
    k, m, n = 6, 3, 9

    def stripes():
        good = _stripe(k, m, 50, 1)
        short = _stripe(k, m, 50, 2)
        short[2] = short[2][:-1]
        few = [None, None, None, None] + _stripe(k, m, 50, 3)[4:]
        fixed = _stripe(k, m, 50, 4)
        fixed[8][49] ^= 1
        fixed[0][3] ^= 0x80
        left = _stripe(k, m, 50, 5)
        left[1][7] ^= 1
        left[7][7] ^= 2
        two = _stripe(k, m, 50, 6)  # r' = 2: located, not corrected
        two[4] = None
        two[2][9] ^= 9
        return [good, [None] * n, short, few, fixed, left, two, _stripe(k, m, 50, 7)[:k] + [None] * m]

    loc_counts, loc_status = locate_batch(stripes(), k, m)
    st = stripes()
    counts, status = correct_batch(st, k, m)
    C = N.RS_E_CORRUPT
    assert loc_status == [0, N.RS_E_NO_DATA, N.RS_E_SHARD_SIZE, N.RS_E_TOO_FEW_SHARDS, C, C, C, 0]
    assert status == [0, N.RS_E_NO_DATA, N.RS_E_SHARD_SIZE, N.RS_E_TOO_FEW_SHARDS, 0, C, C, 0]
    assert np.array_equal(counts[:6], loc_counts[:6])
    assert int(counts[4, 8]) == 1 and int(counts[4, 0]) == 1 and int(counts[5, n]) == 1
    assert int(loc_counts[6, 2]) == 1 and int(counts[6, n]) == 1 and int(counts[6].sum()) == 1
    assert [bytes(s) for s in st[4]] == [bytes(s) for s in _stripe(k, m, 50, 4)]
    ref = stripes()
    for b in (5, 6):
        assert [None if s is None else bytes(s) for s in st[b]] == [None if s is None else bytes(s) for s in ref[b]]


def _scatter(shards, S, rng):
    """Every shard damaged, in pairwise disjoint columns."""
    n = len(shards)
    cols = rng.permutation(S)[:40 * n]
    for i in range(n):
        for c in cols[40 * i:40 * (i + 1)]:
            shards[i][int(c)] ^= int(rng.integers(1, 256))


def test_decode_correct(native_lib):
    import ctypes
    from callfs_amd import (Codec, ErasureProfile, ErrInsufficientShards, ErrShardCorrupted,
                            ErrShardNoData, ErrShardSize, ErrTooFewShards)
    from callfs_amd import _native as N
    codec = Codec()
    p = ErasureProfile(10, 4)
    n = 14
    data = np.random.default_rng(3).integers(0, 256, 123_457, dtype=np.uint8).tobytes()
    full = [bytes(s) for s in codec.encode(data, p)]
    # every one of the 14 shards damaged, in pairwise disjoint columns: decode and decode_heal
    # refuse, decode_correct returns the object and every shard is restored
    sh = [bytearray(s) for s in full]
    _scatter(sh, len(full[0]), np.random.default_rng(4))
    with pytest.raises(ErrShardCorrupted):
        codec.decode([bytearray(s) for s in sh], p, len(data))
    with pytest.raises(ErrShardCorrupted):
        codec.decode_heal([bytearray(s) for s in sh], p, len(data))
    out, corrected = codec.decode_correct(sh, p, len(data))
    assert bytes(out) == data and corrected == list(range(n))
    assert [bytes(s) for s in sh] == full
    # one shard missing (r' = 3), one corrupt
    sh = [bytearray(s) for s in full]
    _flip(sh[12], [0, 1000, len(full[0]) - 1])
    sh[7] = None
    out, corrected = codec.decode_correct(sh, p, len(data))
    assert bytes(out) == data and corrected == [12] and [bytes(s) for s in sh] == full
    # clean: decode's bytes, nothing corrected
    sh = [None if i == 2 else bytearray(s) for i, s in enumerate(full)]
    out, corrected = codec.decode_correct(sh, p, len(data))
    assert bytes(out) == data and corrected == [] and bytes(sh[2]) == full[2]
    # beyond repair: two shards in the same column; the single-error column is corrected all
    # the same
    sh = [bytearray(s) for s in full]
    sh[1][5] ^= 1
    sh[11][5] ^= 1
    sh[4][900] ^= 0x55
    with pytest.raises(ErrShardCorrupted):
        codec.decode_correct(sh, p, len(data))
    assert bytes(sh[4]) == full[4] and sh[1][5] == full[1][5] ^ 1 and sh[11][5] == full[11][5] ^ 1
    # every other error precedes as in decode
    p42 = ErasureProfile(4, 2)
    s42 = [bytearray(s) for s in codec.encode(b"x" * 100, p42)]
    bad = [bytearray(s) for s in s42]
    bad[1] = bad[1][:-1]
    for exc, shards, size in ((ErrInsufficientShards, [bytearray(s) for s in s42], 101),
                              (ErrShardNoData, [None] * 6, 10), (ErrShardSize, bad, 100),
                              (ErrTooFewShards, s42[:5], 100),
                              (ErrTooFewShards, [None, None, None] + s42[3:], 100)):
        with pytest.raises(exc):
            codec.decode(list(shards), p42, size)
        with pytest.raises(exc):
            codec.decode_correct(list(shards), p42, size)
    # the C call itself
    sh = [bytearray(s) for s in full]
    sh[9][77] ^= 0x10
    ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof((ctypes.c_char * len(s)).from_buffer(s)) for s in sh])
    lens = (ctypes.c_size_t * n)(*[len(s) for s in sh])
    out = bytearray(len(data))
    corrected = (ctypes.c_uint8 * n)()
    rc = N.lib.rs_codec_decode_correct(N.default_context().handle, 10, 4, ptrs, lens,
                                       ctypes.addressof((ctypes.c_char * len(out)).from_buffer(out)),
                                       len(data), corrected)
    assert rc == 0 and list(corrected) == [int(i == 9) for i in range(n)]
    assert bytes(out) == data and [bytes(s) for s in sh] == full
