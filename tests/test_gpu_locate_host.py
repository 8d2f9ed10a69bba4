"""Locate and heal on host memory: rs_locate / rs_locate_batch give the
device plan's counts over the same bytes, column parts of a chunked stripe included;
rs_heal_batch, rs_codec_decode_heal and Codec.decode_heal repair a stripe whose corrupt
shards the syndromes name and leave every other present shard untouched. Expected values
are what the test corrupted and the C oracle's encode."""
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
from callfs_amd.erasure import host_counters, locate, locate_batch

k, m, n = 10, 4, 14
sizes = [40000, 9, 8192 + 21, 100, 16, 70001]
lost = [(), (3,), (0, 13), (1, 2, 5, 12), (), (11,)]
rng = np.random.default_rng(9)
stripes = []
for S in sizes:
    data = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
    par = cref.encode(data, k, m)
    stripes.append([np.array(x, dtype=np.uint8) for x in data] + [np.array(p, dtype=np.uint8) for p in par])
# 14 shards of 40,000 bytes do not fit a 256 KiB chunk: stripe 0 is cut into column parts at
# multiples of 8,192 bytes; corrupt it on both sides of every possible cut
cuts = [c for c in range(8192, 40000, 8192)]
hits = {(0, 4): [0] + [c - 1 for c in cuts] + [39999], (0, 12): cuts + [5],
        (2, 7): [8191, 8192, 8212], (5, 0): list(range(0, 70001, 1001)), (5, 13): [70000],
        (3, 0): [7]}
exp = np.zeros((len(sizes), n + 1), dtype=np.uint64)
for (b, i), cols in hits.items():
    for c in cols:
        stripes[b][i][c] ^= 0x31
    if len(lost[b]) < m:
        exp[b, i] = len(cols)
host = [[None if i in lost[b] else stripes[b][i] for i in range(n)] for b in range(len(sizes))]
c0 = host_counters()
counts, status = locate_batch(host, k, m)
c1 = host_counters()
bad = 0
if not np.array_equal(counts, exp):
    print("host counts", np.argwhere(counts != exp)[:8].tolist())
    bad += 1
want_status = [N.RS_E_CORRUPT, 0, N.RS_E_CORRUPT, 0, 0, N.RS_E_CORRUPT]
if status != want_status:
    print("status", status)
    bad += 1
if c1["calls"] - c0["calls"] != 1 or c1["chunks"] - c0["chunks"] < 3 or \
        c1["launches"] - c0["launches"] != c1["chunks"] - c0["chunks"]:
    print("counters", c0, c1)
    bad += 1
# the device plan over the same bytes
rb = RaggedBatch(k, m, sizes, torch.device("cuda:0"))
masks = [[i not in lost[b] for i in range(n)] for b in range(len(sizes))]
for b in range(len(sizes)):
    for i in range(n):
        rb.shard(b, i).copy_(torch.from_numpy(stripes[b][i]))
plan = Plan.for_ragged(rb, present=masks, locate=True)
plan.launch()
dev = plan.blame()
plan.close()
if not np.array_equal(dev, counts):
    print("device counts differ", np.argwhere(dev != counts)[:8].tolist())
    bad += 1
one = locate(host[0], k, m)
if not np.array_equal(one, exp[0]):
    print("rs_locate", one.tolist())
    bad += 1
print("chunked locate child:", "ok" if not bad else "%d mismatches" % bad)
sys.exit(1 if bad else 0)
"""


def test_locate_batch_chunked_matches_device_plan(native_lib):
    """CALLFS_RS_CHUNK_BYTES is read once per process: a fresh child with 256 KiB chunks."""
    env = dict(os.environ)
    env["CALLFS_RS_CHUNK_BYTES"] = str(256 << 10)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _CHUNK_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "chunked locate child: ok" in r.stdout


def test_locate_status_values_match_reconstruct_batch(native_lib):
    from callfs_amd import _native as N
    from callfs_amd.erasure import host_counters, locate, locate_batch, reconstruct_batch
    k, m, n = 4, 2, 6

    def stripes():
        good = _stripe(k, m, 50, 1)
        short = _stripe(k, m, 50, 2)
        short[2] = short[2][:-1]
        few = [None, None, None] + _stripe(k, m, 50, 3)[3:]
        bad = _stripe(k, m, 50, 4)
        bad[5][49] ^= 1
        return [good, [None] * n, short, few, bad, _stripe(k, m, 50, 5)[:4] + [None, None]]

    counts, status = locate_batch(stripes(), k, m)
    assert status == reconstruct_batch(stripes(), k, m, verify=True)
    assert status == [0, N.RS_E_NO_DATA, N.RS_E_SHARD_SIZE, N.RS_E_TOO_FEW_SHARDS, N.RS_E_CORRUPT, 0]
    assert int(counts[4, 5]) == 1 and int(counts.sum()) == 1
    # exactly k present: zero counts, RS_OK, no device work
    c0 = host_counters()
    only_k = _stripe(k, m, 50, 6)[:4] + [None, None]
    assert not locate(only_k, k, m).any()
    counts, status = locate_batch([only_k, list(only_k)], k, m)
    assert status == [0, 0] and not counts.any()
    assert host_counters() == c0


@pytest.mark.parametrize("k,m", [(10, 4), (6, 3)])
def test_heal_batch(native_lib, k, m):
    from callfs_amd import _native as N
    from callfs_amd.erasure import heal_batch
    n = k + m
    sizes = [8192 + 37, 100, 5000, 16, 9, 3000, 777]
    full = [_stripe(k, m, S, 10 + b) for b, S in enumerate(sizes)]
    st = [[bytearray(s) for s in f] for f in full]
    # 0: a corrupt valid shard and a missing shard
    _flip(st[0][1], [0, 8191, 8192, sizes[0] - 1])
    st[0][k] = None
    # 1: a corrupt compared shard
    _flip(st[1][n - 1], range(100))
    # 2: two shards corrupt in the same columns: unexplained
    _flip(st[2][0], [17, 4000], 2)
    _flip(st[2][n - 2], [17, 4000], 3)
    # 3: two compared shards left, two shards blamed: present - |B| = k, no row to confirm with
    for i in range(m - 2):
        st[3][k + 2 + i] = None
    _flip(st[3][2], [5])
    _flip(st[3][0], [9])
    # 4: clean; 5: clean with a missing shard
    st[5][0] = None
    # 6: two corrupt shards in disjoint columns, both blamed (m - 2 rows left: RS(10,4) only)
    if m >= 4:
        _flip(st[6][3], [1, 2, 3])
        _flip(st[6][k + 1], [700])
    before = [[None if s is None else bytes(s) for s in row] for row in st]
    status, healed = heal_batch(st, k, m)
    C = N.RS_E_CORRUPT
    assert status == [0, 0, C, C, 0, 0, 0]
    assert healed == [[1], [n - 1], [], [], [], [], [3, k + 1] if m >= 4 else []]
    for b in (0, 1, 4, 5, 6):
        assert [bytes(s) for s in st[b]] == [bytes(s) for s in full[b]], b
    # the present shards nobody blamed are byte-identical to what went in
    assert [bytes(st[2][i]) for i in range(n)] == before[2]
    for i in range(n):
        if before[3][i] is not None and i not in (0, 2):
            assert bytes(st[3][i]) == before[3][i]


def test_heal_rs42_with_one_row_to_spare(native_lib):
    """RS(4,2), everything present, one corrupt shard: r' = 2 and present - |B| = k + 1."""
    from callfs_amd.erasure import heal_batch
    for shard in (2, 5):
        full = _stripe(4, 2, 8192 + 5, 40 + shard)
        st = [[bytearray(s) for s in full]]
        _flip(st[0][shard], [0, 4095, 8192, 8196])
        status, healed = heal_batch(st, 4, 2)
        assert status == [0] and healed == [[shard]]
        assert [bytes(s) for s in st[0]] == [bytes(s) for s in full]


def test_decode_heal(native_lib):
    import ctypes
    from callfs_amd import (Codec, ErasureProfile, ErrInsufficientShards, ErrShardCorrupted,
                            ErrShardNoData, ErrShardSize, ErrTooFewShards)
    from callfs_amd import _native as N
    codec = Codec()
    p = ErasureProfile(10, 4)
    data = np.random.default_rng(3).integers(0, 256, 123_457, dtype=np.uint8).tobytes()
    full = [bytes(s) for s in codec.encode(data, p)]
    for shard, lost in ((3, 0), (12, 7), (0, None)):
        sh = [bytearray(s) for s in full]
        _flip(sh[shard], [0, 1000, len(full[0]) - 1])
        if lost is not None:
            sh[lost] = None
        probe = [None if s is None else bytearray(s) for s in sh]
        with pytest.raises(ErrShardCorrupted):
            codec.decode(probe, p, len(data))
        out, healed = codec.decode_heal(sh, p, len(data))
        assert bytes(out) == data and healed == [shard]
        assert [bytes(s) for s in sh] == full
    # clean: decode's bytes, nothing healed
    sh = [None if i == 2 else bytearray(s) for i, s in enumerate(full)]
    out, healed = codec.decode_heal(sh, p, len(data))
    assert bytes(out) == data and healed == [] and bytes(sh[2]) == full[2]
    # beyond repair: two shards in the same column
    sh = [bytearray(s) for s in full]
    sh[1][5] ^= 1
    sh[11][5] ^= 1
    with pytest.raises(ErrShardCorrupted):
        codec.decode_heal(sh, p, len(data))
    # every other error precedes as in decode
    p42 = ErasureProfile(4, 2)
    s42 = [bytearray(s) for s in codec.encode(b"x" * 100, p42)]
    with pytest.raises(ErrInsufficientShards):
        codec.decode_heal([bytearray(s) for s in s42], p42, 101)
    with pytest.raises(ErrShardNoData):
        codec.decode_heal([None] * 6, p42, 10)
    bad = [bytearray(s) for s in s42]
    bad[1] = bad[1][:-1]
    with pytest.raises(ErrShardSize):
        codec.decode_heal(bad, p42, 100)
    with pytest.raises(ErrTooFewShards):
        codec.decode_heal(s42[:5], p42, 100)
    with pytest.raises(ErrTooFewShards):
        codec.decode_heal([None, None, None] + s42[3:], p42, 100)
    # the C call itself
    sh = [bytearray(s) for s in full]
    sh[9][77] ^= 0x10
    n = 14
    ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof((ctypes.c_char * len(s)).from_buffer(s)) for s in sh])
    lens = (ctypes.c_size_t * n)(*[len(s) for s in sh])
    out = bytearray(len(data))
    healed = (ctypes.c_uint8 * n)()
    rc = N.lib.rs_codec_decode_heal(N.default_context().handle, 10, 4, ptrs, lens,
                                    ctypes.addressof((ctypes.c_char * len(out)).from_buffer(out)),
                                    len(data), healed)
    assert rc == 0 and list(healed) == [int(i == 9) for i in range(n)]
    assert bytes(out) == data and [bytes(s) for s in sh] == full
