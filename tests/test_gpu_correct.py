"""Correct device plans (rs_plan_create_correct): a launch repairs, in place,
every byte column in which one examined shard is corrupt, where the stripe compares three or
more shards, and counts the bytes it changed per shard. Stripes are consistent (parity from the
C oracle) and the test damages them itself, so the expected bytes are exact: the pristine byte
where the guarantee says corrected, the damaged byte where it says untouched -- over the whole
sentinel-guarded allocation, guards included. Expected counts come from the damage alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A
SIZES = [1, 15, 16, 17, 40, 1023, 1024, 8191, 8192, 8193, 2 * 8192 + 83]


@pytest.fixture(autouse=True)
def _no_tuned_forms(native_lib):
    native_lib.lib.rs_tune_table_reset(None)
    yield
    native_lib.lib.rs_tune_table_reset(None)


def _mask(n, lost):
    lost = set(lost)
    return [i not in lost for i in range(n)]


def _examined(k, mask):
    """(valid, cmp): the first k present shards and the next min(present - k, 16)."""
    present = [i for i, p in enumerate(mask) if p]
    return present[:k], present[k:k + 16]


def _bytes(k, sizes, masks):
    return sum(S * (k + len(_examined(k, mk)[1])) for S, mk in zip(sizes, masks) if _examined(k, mk)[1])


class _Arena:
    """Guards and sentinel padding around a RaggedBatch-shaped body. Present shards hold a
    consistent stripe, missing shards junk. `damage(hits)` uploads the pristine image with
    hits = {(stripe, shard): columns} XORed with nonzero bytes; `expected(hits)` gives the
    counts and the whole allocation a correcting launch must leave behind."""

    def __init__(self, k, m, sizes, masks, layout, seed, guard=4096):
        import torch
        from callfs_amd.device import RaggedBatch
        self.torch = torch
        dev = torch.device("cuda:0")
        self.k, self.m, self.n, self.sizes, self.masks = k, m, k + m, list(sizes), masks
        self.rb = rb = RaggedBatch(k, m, sizes, dev, layout=layout)  # for the offsets
        self.rng = rng = np.random.default_rng(seed)
        self.clean = np.full(rb.nbytes, SENTINEL, dtype=np.uint8)
        for b, S in enumerate(sizes):
            data = rng.integers(0, 256, (k, S), dtype=np.uint8)
            par = cref.encode([data[i] for i in range(k)], k, m)
            for i in range(self.n):
                o = rb.offsets[b][i]
                if masks[b][i]:
                    self.clean[o:o + S] = data[i] if i < k else np.asarray(par[i - k])
                else:
                    self.clean[o:o + S] = rng.integers(0, 256, S, dtype=np.uint8)  # junk
        self.raw = torch.full((rb.nbytes + 2 * guard + 256,), SENTINEL, dtype=torch.uint8, device=dev)
        self.lead = guard + (-(self.raw.data_ptr() + guard) % 256)
        base = self.raw.data_ptr() + self.lead
        self.ptrs = [base + o for row in rb.offsets for o in row]
        self.damage({})

    def damage(self, hits):
        img = self.clean.copy()
        for (b, i), cols in hits.items():
            cols = np.unique(np.asarray(cols, dtype=np.int64))
            assert cols.size and 0 <= cols[0] and cols[-1] < self.sizes[b]
            o = self.rb.offsets[b][i]
            img[o + cols] ^= self.rng.integers(1, 256, cols.size, dtype=np.uint8)
        self.damaged = img
        self.raw[self.lead:self.lead + self.rb.nbytes].copy_(self.torch.from_numpy(img))
        self.torch.cuda.synchronize()
        self.before = self.raw.cpu().numpy()

    def expected(self, hits):
        """(counts, allocation) from the hits alone: per column, the examined shards the test
        changed. One, with r' >= 3: that byte pristine again and counted for its shard. Anything
        else that mismatches: the damaged bytes stay, the column is unexplained."""
        exp = np.zeros((len(self.sizes), self.n + 1), dtype=np.uint64)
        img = self.damaged.copy()
        for b, S in enumerate(self.sizes):
            valid, cmp = _examined(self.k, self.masks[b])
            if not cmp:
                continue
            per_col = {}
            for (hb, i), cols in hits.items():
                if hb == b and i in valid + cmp:
                    for c in np.unique(np.asarray(cols)):
                        per_col.setdefault(int(c), []).append(i)
            for c, shards in per_col.items():
                assert len(shards) < len(cmp) or len(shards) == 1, "the rule promises nothing here"
                if len(cmp) >= 3 and len(shards) == 1:
                    exp[b, shards[0]] += 1
                    o = self.rb.offsets[b][shards[0]] + c
                    img[o] = self.clean[o]
                else:
                    exp[b, self.n] += 1
        full = self.before.copy()
        full[self.lead:self.lead + self.rb.nbytes] = img
        return exp, full

    def differs(self, full):
        self.torch.cuda.synchronize()
        return np.flatnonzero(self.raw.cpu().numpy() != full)[:8].tolist()

    def run(self, plan, hits):
        """Damage, one launch; checks the whole allocation and the counts; returns the counts."""
        self.damage(hits)
        plan.launch()
        flagged = plan.corrupt_stripes()
        counts = plan.blame()
        exp, full = self.expected(hits)
        assert self.differs(full) == []
        _same(counts, exp)
        want = sorted({b for b in range(len(self.sizes)) if exp[b].any()})
        assert flagged == want  # every stripe that had a mismatch, corrected or not
        return counts


def _same(counts, exp):
    assert counts.shape == exp.shape and counts.dtype == np.uint64
    bad = np.argwhere(counts != exp)[:6].tolist()
    assert not bad, [(b, i, int(counts[b, i]), int(exp[b, i])) for b, i in bad]


def _edge_columns(S):
    """The first and last 16 columns, both sides of the 512-vector tile edge and of the
    64-vector wave edge, and the S % 16 tail."""
    cols = set(range(min(16, S))) | set(range(max(0, S - 16), S))
    cols |= {c for c in (8191, 8192, 1023, 1024) if c < S}
    cols |= set(range(S - S % 16, S))
    return sorted(cols)


@pytest.mark.parametrize("layout", ["aligned", "packed"])
def test_sizes_layouts_and_single_corruptions(native_lib, layout):
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    rng = np.random.default_rng(5)
    masks = []
    for b in range(len(SIZES)):  # 0, 1 and 2 shards missing in turn: r' = 4, 3, 2
        masks.append(_mask(n, [int(i) for i in rng.choice(n, size=b % 3, replace=False)]))
    ar = _Arena(k, m, SIZES, masks, layout, seed=17)
    plan = Plan.correct(k, m, SIZES, ar.ptrs, present=masks)
    assert plan.forms() == ["correct"] and plan.bytes == _bytes(k, SIZES, masks)
    assert not ar.run(plan, {}).any()
    # one corrupt shard per stripe, every fourth stripe left clean
    picks = {"valid": lambda v, c: v[3], "compared": lambda v, c: c[len(c) // 2],
             "first examined": lambda v, c: v[0], "last examined": lambda v, c: c[-1]}
    for name, pick in picks.items():
        hits = {}
        for b, S in enumerate(SIZES):
            if b % 4 == 3:
                continue
            hits[(b, pick(*_examined(k, masks[b])))] = _edge_columns(S)
        counts = ar.run(plan, hits)
        for (b, i), cols in hits.items():
            if b % 3 == 2:  # r' = 2: nothing written, every damaged column unexplained
                assert int(counts[b, n]) == len(cols) and not counts[b, :n].any(), name
            else:
                assert int(counts[b, i]) == len(cols) and int(counts[b, n]) == 0, name
    # a whole shard: a valid one in even stripes, a compared one in odd stripes
    hits = {}
    for b, S in enumerate(SIZES):
        if b % 4 == 3:
            continue
        v, c = _examined(k, masks[b])
        hits[(b, v[b % k] if b % 2 == 0 else c[b % len(c)])] = np.arange(S)
    counts = ar.run(plan, hits)
    for (b, i) in hits:
        assert int(counts[b, n if b % 3 == 2 else i]) == SIZES[b] and int(counts[b].sum()) == SIZES[b]
    # at r' >= 3 the allocation is the pristine one again
    ok = [b for b in range(len(SIZES)) if b % 3 != 2]
    got = ar.raw.cpu().numpy()[ar.lead:ar.lead + ar.rb.nbytes]
    for b in ok:
        for i in range(n):
            o = ar.rb.offsets[b][i]
            assert np.array_equal(got[o:o + SIZES[b]], ar.clean[o:o + SIZES[b]])
    plan.close()


def _scattered_hits(S, n, rng):
    """Every one of n shards corrupt, in pairwise disjoint columns: shards i and i + 1 share a
    lane's 16 columns at the front (the verdict changes inside a lane's vector), each shard has a run of its own, single columns on the tile and wave edges go to
    different shards, and the S % 16 tail is dealt out byte by byte."""
    hits = {i: [] for i in range(n)}
    for c in range(0, 16 * n):  # vector v: columns 0..5 shard v, 6..7 clean, 8..15 shard v + 1
        v, j = divmod(c, 16)
        if j < 6:
            hits[v].append(c)
        elif j >= 8:
            hits[(v + 1) % n].append(c)
    for i in range(n):  # a run of 40 columns each, whole vectors and more
        hits[i] += list(range(1000 + 50 * i, 1040 + 50 * i))
    for q, c in enumerate([1023 + 1024, 1024 + 1024, 8191, 8192, 8193, 2 * 8192 - 1, 2 * 8192]):
        hits[(3 * q + 1) % n].append(c)
    for c in range(S - S % 16, S):
        hits[c % n].append(c)
    spare = np.setdiff1d(np.arange(3000, S - 16), np.concatenate([np.asarray(v) for v in hits.values()]))
    for c in rng.choice(spare, size=200, replace=False):
        hits[int(rng.integers(0, n))].append(int(c))
    flat = np.concatenate([np.asarray(v) for v in hits.values()])
    assert np.unique(flat).size == flat.size  # pairwise disjoint
    return hits


def test_every_shard_corrupt_in_disjoint_columns_where_heal_refuses(native_lib):
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    from callfs_amd.erasure import heal_batch
    k, m, n = 10, 4, 14
    sizes = [2 * 8192 + 16 * 7 + 11, 4000]
    masks = [_mask(n, ()), _mask(n, ())]
    ar = _Arena(k, m, sizes, masks, "packed", seed=61)
    plan = Plan.correct(k, m, sizes, ar.ptrs, present=masks)
    per = _scattered_hits(sizes[0], n, np.random.default_rng(8))
    hits = {(0, i): cols for i, cols in per.items()}
    ar.damage(hits)
    o = ar.rb.offsets[0]
    host = [[bytearray(ar.damaged[o[i]:o[i] + sizes[0]].tobytes()) for i in range(n)]]
    counts = ar.run(plan, hits)
    for i in range(n):
        assert int(counts[0, i]) == len(per[i])
    assert int(counts[0, n]) == 0 and not counts[1].any()
    got = ar.raw.cpu().numpy()[ar.lead:ar.lead + ar.rb.nbytes]
    assert np.array_equal(got, ar.clean)  # restored exactly
    # the heal needs p - |B| >= k + 1 and has 14 blamed shards
    status, healed = heal_batch(host, k, m)
    assert status == [N.RS_E_CORRUPT] and healed == [[]]
    plan.close()


def test_same_columns_stay_and_second_launch_changes_nothing(native_lib):
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [2 * 8192 + 9, 8192 + 16 * 5 + 3, 7, 5000, 9000]
    masks = [_mask(n, ()), _mask(n, (6,)), _mask(n, (0, 5, 12)), _mask(n, (1, 2, 3, 13)), _mask(n, (4,))]
    ar = _Arena(k, m, sizes, masks, "packed", seed=23)
    plan = Plan.correct(k, m, sizes, ar.ptrs, present=masks)
    assert int(native_lib.lib.rs_plan_groups(plan.handle)) == 1
    S0 = sizes[0]
    same = [0, 1, 15, 16, 1023, 1024, 8191, 8192, 8200, S0 - 16, S0 - 2, S0 - 1]
    hits = {
        # two shards in the same columns (r' = 4): untouched, unexplained ...
        (0, 7): same,
        (0, 11): same,
        # ... while the single-error columns of the same stripe, some in the same lanes, are repaired
        (0, 2): [2, 3, 17, 1025, 8190, 8193, S0 - 3] + list(range(3000, 3100)),
        (0, 13): [4, 18, 8201] + list(range(5000, 5010)),
        # r' = 3, a valid and a compared shard in the same columns and alone
        (1, 0): [5, 8192, sizes[1] - 1, 100],
        (1, 12): [5, 8192, sizes[1] - 1, 200],
        # r' = 1: nothing written
        (2, 3): [0, 6],
        # exactly k present: in no launch
        (3, 0): [0, 17, 4999],
        # a missing shard's buffer is never read or written
        (4, 4): list(range(0, 9000, 7)),
    }
    counts = ar.run(plan, hits)
    assert int(counts[0, n]) == len(same) and int(counts[0, 2]) == 107 and int(counts[0, 13]) == 13
    assert int(counts[1, n]) == 3 and int(counts[1, 0]) == 1 and int(counts[1, 12]) == 1
    assert int(counts[2, n]) == 2 and not counts[3].any() and not counts[4].any()
    # a second launch over the repaired data: no byte changes, shard bins zero, the columns
    # left over are counted again
    after = ar.raw.cpu().numpy()
    plan.launch()
    again = plan.blame()
    assert ar.differs(after) == []
    assert not again[:, :n].any()
    assert again[:, n].tolist() == counts[:, n].tolist()
    assert plan.corrupt_stripes() == [0, 1, 2]
    # blame() clears on read
    assert not plan.blame().any()
    plan.close()


def test_graph_replays_after_fresh_damage(native_lib):
    import torch
    from callfs_amd.device import Plan
    k, m, n = 6, 3, 9
    sizes = [8192 + 21, 16, 3 * 8192]
    masks = [_mask(n, ()), _mask(n, ()), _mask(n, ())]
    ar = _Arena(k, m, sizes, masks, "aligned", seed=7)
    plan = Plan.correct(k, m, sizes, ar.ptrs, present=masks)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        plan.launch(s)
    torch.cuda.synchronize()
    assert not plan.blame(s).any()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch(s)
    assert not plan.blame(s).any()  # capturing ran nothing
    for hits in ({(0, 1): [0, 8191, 8192, 8212], (1, 7): [15], (2, 4): np.arange(3 * 8192)},
                 {(0, 8): np.arange(sizes[0]), (2, 0): [1, 2, 3 * 8192 - 1], (2, 5): [4, 5]}):
        ar.damage(hits)
        exp, full = ar.expected(hits)
        g.replay()
        torch.cuda.synchronize()  # the replay runs on the current stream, the read on s
        assert ar.differs(full) == []
        _same(plan.blame(s), exp)
        assert plan.corrupt_stripes(s) == sorted({b for b, _ in hits})
        assert np.array_equal(ar.raw.cpu().numpy()[ar.lead:ar.lead + ar.rb.nbytes], ar.clean)
    plan.close()


PROFILES = [(1, 3), (4, 2), (6, 3), (16, 4), (10, 8), (20, 12), (10, 20)]


@pytest.mark.parametrize("k,m", PROFILES)
def test_profiles(native_lib, k, m):
    """The 4-, 8- and 16-row instances at one odd size; RS(4,2) has r' = 2 and writes nothing;
    RS(10,20) examines 16 of its 20 compared shards and ignores damage in the other four."""
    from callfs_amd.device import Plan
    n = k + m
    sizes = [8192 + 16 * 3 + 5]
    masks = [_mask(n, ())]
    ar = _Arena(k, m, sizes, masks, "aligned", seed=100 * k + m)
    plan = Plan.correct(k, m, sizes, ar.ptrs, present=masks)
    assert plan.forms() == ["correct"] and plan.bytes == _bytes(k, sizes, masks)
    rng = np.random.default_rng(k * 31 + m)
    v, c = _examined(k, masks[0])
    S = sizes[0]
    edges = [0, 8191, S - 1, 1, 8192, S - 2]
    cols = rng.permutation(np.setdiff1d(np.arange(S), edges))  # no column damaged in two shards
    hits = {(0, v[int(rng.integers(0, len(v)))]): np.concatenate([cols[:37], edges[:3]]),
            (0, c[-1]): np.concatenate([cols[37:60], edges[3:]])}
    if v[0] not in [i for _, i in hits]:
        hits[(0, v[0])] = cols[60:70]
    if m > 16:  # present shards past the 16th compared one: neither read, blamed nor written
        hits[(0, k + 16)] = np.arange(S)
        hits[(0, n - 1)] = cols[:100]
    counts = ar.run(plan, hits)
    examined = sum(np.unique(np.asarray(cl)).size for (_, i), cl in hits.items() if i in v + c)
    assert int(counts[0].sum()) == examined
    if m >= 3:
        assert int(counts[0, n]) == 0
    else:
        assert int(counts[0, n]) == examined
    plan.close()


def test_plan_properties_and_argument_errors_are_the_locate_plans(native_lib):
    import ctypes
    import torch
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [8192 + 16 * 3 + 5, 11, 4000, 16]
    batch = len(sizes)
    masks = [_mask(n, (0,)), _mask(n, (1, 12)), _mask(n, ()), _mask(n, (2, 3, 4, 5))]
    ar = _Arena(k, m, sizes, masks, "aligned", seed=33)

    def code(fn, *a, **kw):
        with pytest.raises(N.NativeError) as ei:
            fn(*a, **kw)
        return ei.value.code

    short = [list(x) for x in masks]
    short[2] = _mask(n, (0, 1, 2, 3, 4))
    for args, kw in (((k, m, [sizes[0], 0, 4000, 16], ar.ptrs), {"present": masks}),
                     ((k, m, sizes, ar.ptrs), {"present": short}),
                     ((0, 4, sizes, ar.ptrs[:4 * batch]), {"present": [mk[:4] for mk in masks]}),
                     ((200, 100, [16], [0] * 300), {})):
        assert code(Plan.correct, *args, **kw) == code(Plan.locate, *args, **kw)
    assert code(Plan.correct, k, m, [sizes[0], 0, 4000, 16], ar.ptrs, present=masks) == N.RS_E_NO_DATA
    with pytest.raises(ValueError):
        Plan.correct(k, m, sizes, ar.ptrs, present=masks[:3])

    L = N.lib
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    plan = Plan.correct(k, m, sizes, ar.ptrs, present=np.array(masks, dtype=bool))
    ref = Plan.locate(k, m, sizes, ar.ptrs, present=masks)
    assert int(L.rs_plan_groups(plan.handle)) == int(L.rs_plan_groups(ref.handle)) == 1
    forms = (ctypes.c_int * 1)()
    assert L.rs_plan_forms(plan.handle, forms, 1) == 1 and forms[0] == 16384 and plan.forms() == ["correct"]
    assert L.rs_plan_forms(ref.handle, forms, 1) == 1 and forms[0] == 8192
    assert plan.bytes == ref.bytes == sizes[0] * 13 + 11 * 12 + 4000 * 14  # stripe 3 has exactly k present
    assert plan.tune() == ref.tune() == ["none"] and L.rs_tune_table_entries() == 0
    assert code(plan.set_orders, ["consecutive"]) == code(ref.set_orders, ["consecutive"]) == N.RS_E_ARG
    plan.set_orders(["none"])
    assert L.rs_plan_launch_ceiling(plan.handle, s, 1) == L.rs_plan_launch_ceiling(ref.handle, s, 1) == N.RS_E_ARG
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    plan.launch(events=(e0, e1))
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) > 0
    assert not plan.blame().any() and not plan.corrupt() and ar.differs(ar.before) == []
    assert L.rs_plan_blame(plan.handle, s, None) == N.RS_E_ARG
    ref.close()
    plan.close()

    # present = None: every shard present
    same = [4000] * batch
    ar2 = _Arena(k, m, same, [_mask(n, ())] * batch, "aligned", seed=34)
    plan = Plan.correct(k, m, same, ar2.ptrs)
    assert plan.forms() == ["correct"] and plan.bytes == 4000 * 14 * batch
    counts = ar2.run(plan, {(2, 13): [3999]})
    assert int(counts[2, 13]) == 1 and int(counts.sum()) == 1
    plan.close()

    # no stripe has a row: no launch group, nothing enqueued, nothing written
    none = [_mask(n, (0, 5, 12, 13)), _mask(n, (1, 2, 3, 4))]
    ar3 = _Arena(k, m, [100, 9000], none, "packed", seed=35)
    plan = Plan.correct(k, m, [100, 9000], ar3.ptrs, present=none)
    assert int(L.rs_plan_groups(plan.handle)) == 0 and plan.forms() == [] and plan.bytes == 0
    plan.launch(events=(e0, e1))
    assert not ar3.run(plan, {(0, 1): [5], (1, 13): [0]}).any()
    plan.close()


_SLICED_CHILD = r"""
import sys
import numpy as np
import torch
from callfs_amd.device import Plan, RaggedBatch

k, m, n = 2, 3, 5
sizes = [53 * 8192 + b % 17 for b in range(40)] + [8192, 5, 8193, 16]
batch = len(sizes)
rb = RaggedBatch(k, m, sizes, torch.device("cuda:0"))
rb.fill_random(11)
enc = Plan.for_ragged(rb)   # encode first, so that the stripes are consistent
enc.launch()
torch.cuda.synchronize()
enc.close()
# stripe b loses shard b % 5 when b % 7 == 2 (r' = 2), every fifth stripe three (no row)
masks = []
for b in range(batch):
    lost = [b % n, (b + 1) % n, (b + 2) % n] if b % 5 == 0 else [b % n] if b % 7 == 2 else []
    masks.append([i not in lost for i in range(n)])
tiles = [max(1, -(-(sizes[b] // 16) // 512)) if sum(masks[b]) > k else 0 for b in range(batch)]
assert sum(tiles) > 1024
pristine = rb.buf.cpu().numpy().copy()
# the slice boundary at tile 1024 falls inside stripe `cut`: corrupt it on both sides
edge = np.cumsum(tiles)
cut = int(np.searchsorted(edge, 1024, side="right"))
assert sum(masks[cut]) == n and edge[cut] - tiles[cut] < 1024 < edge[cut]
col = (1024 - (int(edge[cut]) - tiles[cut])) * 8192
exp = np.zeros((batch, n + 1), dtype=np.uint64)
cols = np.arange(col - 300, col + 500)
rb.shard(cut, 0)[torch.from_numpy(cols).cuda()] ^= 0x21
exp[cut, 0] = cols.size
rb.shard(cut, 4)[col + 600:col + 700] ^= 0x42
exp[cut, 4] = 100
last = batch - 2  # 8193 bytes, everything present
assert sum(masks[last]) == n
rb.shard(last, 3)[8192] ^= 1
exp[last, 3] = 1
want = pristine.copy()
# r' = 2: counted, never written
r2 = next(b for b in range(batch) if sum(masks[b]) == k + 2 and sizes[b] > 8192 and b != cut)
i2 = masks[r2].index(True)
rb.shard(r2, i2)[100:164] ^= 0x80
exp[r2, n] = 64
torch.cuda.synchronize()
want_r2 = rb.shard(r2, i2).cpu().numpy().copy()
plan = Plan.correct(k, m, sizes, rb.pointers(), present=masks)
assert plan.forms() == ["correct"], plan.forms()
plan.launch()
got = plan.blame()
flagged = plan.corrupt_stripes()
bad = int(not np.array_equal(got, exp)) + int(flagged != sorted({cut, r2, last}))
bad += int(not np.array_equal(rb.shard(r2, i2).cpu().numpy(), want_r2))
rb.shard(r2, i2)[100:164] ^= 0x80
torch.cuda.synchronize()
bad += int(not np.array_equal(rb.buf.cpu().numpy(), want))
if bad:
    print("counts", np.argwhere(got != exp)[:8].tolist(), "flagged", flagged, "cut", cut, r2, last)
plan.close()
print("sliced correct child:", "ok" if not bad else "%d mismatches" % bad)
sys.exit(1 if bad else 0)
"""


def test_sliced_grid(native_lib):
    """CALLFS_RS_MAX_TILES_PER_LAUNCH is read once per process: a fresh child runs a batch of
    more than 1,024 tiles in slices of at most 1,024, the cut inside a stripe that is corrupt
    on both sides of it, with stripes that are in no launch; every byte is restored."""
    env = dict(os.environ)
    env["CALLFS_RS_MAX_TILES_PER_LAUNCH"] = "1024"
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _SLICED_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sliced correct child: ok" in r.stdout
