"""Locate device plans (rs_plan_create_locate, rs_plan_blame): a launch
writes nothing and counts, per stripe and shard, the byte columns in which that shard alone
is corrupt. Stripes are consistent (parity from the C oracle); the expected counts are what
the test itself corrupted -- the number of byte columns changed in shard i alone, or
"unexplained" for columns changed in 2..r'-1 examined shards and for every mismatch of a
stripe with one compared shard -- exact, no tolerance. After every launch every byte of the
sentinel-guarded allocation is what it was before."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A
SIZES = [1, 5, 15, 16, 17, 40, 8191, 8192, 8193, 8208, 2 * 8192 + 83, 7]


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
    consistent stripe, missing shards junk. `run(plan, hits)` uploads the clean image with
    hits = {(stripe, shard): columns} XORed with nonzero bytes, launches once, checks that no
    byte changed and returns (counts, flagged stripes)."""

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
        self.upload({})

    def upload(self, hits):
        img = self.clean.copy()
        for (b, i), cols in hits.items():
            cols = np.unique(np.asarray(cols, dtype=np.int64))
            assert cols.size and 0 <= cols[0] and cols[-1] < self.sizes[b]
            o = self.rb.offsets[b][i]
            img[o + cols] ^= self.rng.integers(1, 256, cols.size, dtype=np.uint8)
        self.raw[self.lead:self.lead + self.rb.nbytes].copy_(self.torch.from_numpy(img))
        self.torch.cuda.synchronize()
        self.before = self.raw.cpu().numpy()

    def expected(self, hits):
        """Counts from the hits alone: per column, the examined shards the test changed."""
        exp = np.zeros((len(self.sizes), self.n + 1), dtype=np.uint64)
        for b, S in enumerate(self.sizes):
            valid, cmp = _examined(self.k, self.masks[b])
            if not cmp:
                continue
            per_col = {}
            for (hb, i), cols in hits.items():
                if hb == b and i in valid + cmp:
                    for c in np.unique(np.asarray(cols)):
                        per_col.setdefault(int(c), []).append(i)
            for shards in per_col.values():
                assert len(shards) < len(cmp) or len(cmp) == 1, "the rule promises nothing here"
                if len(cmp) < 2 or len(shards) > 1:
                    exp[b, self.n] += 1
                else:
                    exp[b, shards[0]] += 1
        return exp

    def unchanged(self):
        self.torch.cuda.synchronize()
        return np.flatnonzero(self.raw.cpu().numpy() != self.before)[:8].tolist()

    def run(self, plan, hits):
        self.upload(hits)
        plan.launch()
        flagged = plan.corrupt_stripes()
        counts = plan.blame()
        assert self.unchanged() == []
        return counts, flagged


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
    for b in range(len(SIZES)):  # 0, 1 and 2 shards missing, in turn
        masks.append(_mask(n, [int(i) for i in rng.choice(n, size=b % 3, replace=False)]))
    ar = _Arena(k, m, SIZES, masks, layout, seed=17)
    plan = Plan.locate(k, m, SIZES, ar.ptrs, present=masks)
    assert plan.forms() == ["locate"] and plan.bytes == _bytes(k, SIZES, masks)
    counts, flagged = ar.run(plan, {})
    assert not counts.any() and flagged == []
    # one corrupt shard per stripe, every fourth stripe left clean
    picks = {"valid": lambda v, c: v[3], "compared": lambda v, c: c[len(c) // 2],
             "first examined": lambda v, c: v[0], "last examined": lambda v, c: c[-1]}
    for name, pick in picks.items():
        hits = {}
        for b, S in enumerate(SIZES):
            if b % 4 == 3:
                continue
            hits[(b, pick(*_examined(k, masks[b])))] = _edge_columns(S)
        counts, flagged = ar.run(plan, hits)
        _same(counts, ar.expected(hits))
        assert flagged == sorted({b for b, _ in hits}), name
        assert sum(int(counts[b, i]) for (b, i) in hits) == sum(len(c) for c in hits.values())
    # a whole shard: a valid one in even stripes, a compared one in odd stripes
    hits = {}
    for b, S in enumerate(SIZES):
        if b % 4 == 3:
            continue
        v, c = _examined(k, masks[b])
        hits[(b, v[b % k] if b % 2 == 0 else c[b % len(c)])] = np.arange(S)
    counts, flagged = ar.run(plan, hits)
    _same(counts, ar.expected(hits))
    for (b, i) in hits:
        assert int(counts[b, i]) == SIZES[b] and int(counts[b].sum()) == SIZES[b]
    assert flagged == sorted({b for b, _ in hits})
    # and clean again
    counts, flagged = ar.run(plan, {})
    assert not counts.any() and flagged == []
    plan.close()


def test_several_corrupt_shards_and_ignored_bytes(native_lib):
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [8192 + 16 * 5 + 3, 2 * 8192 + 9, 7, 5000, 9000, 40]
    masks = [_mask(n, ()), _mask(n, ()), _mask(n, (0, 5, 12)), _mask(n, (1, 2, 3, 13)),
             _mask(n, (4,)), _mask(n, (2, 11, 13))]
    ar = _Arena(k, m, sizes, masks, "packed", seed=23)
    plan = Plan.locate(k, m, sizes, ar.ptrs, present=masks)
    assert int(native_lib.lib.rs_plan_groups(plan.handle)) == 1 and plan.forms() == ["locate"]
    assert plan.bytes == _bytes(k, sizes, masks) == sizes[0] * 14 + sizes[1] * 14 + 7 * 11 + 9000 * 13 + 40 * 11
    S0, S1 = sizes[0], sizes[1]
    same = [0, 1, 15, 16, 1023, 1024, 8191, 8192, 8200, S1 - 16, S1 - 2, S1 - 1]
    hits = {
        # two shards in disjoint columns: both blamed, each with its own count
        (0, 2): list(range(0, 40)) + [8191, S0 - 1],
        (0, 12): list(range(40, 100)) + [8192, S0 - 2],
        # two shards in the same columns, r' = 4: unexplained, nobody blamed
        (1, 7): same,
        (1, 11): same,
        # r' = 1 (three missing): one row cannot tell shards apart
        (2, 3): [0, 6],
        (2, 13): [2],
        # exactly k present: in no launch, whatever its shards hold
        (3, 0): [0, 17, 4999],
        # missing shards' buffers are never read
        (4, 4): list(range(0, 9000, 7)),
        # r' = 1, clean
    }
    counts, flagged = ar.run(plan, hits)
    exp = ar.expected(hits)
    _same(counts, exp)
    assert int(counts[0, 2]) == 42 and int(counts[0, 12]) == 62 and int(counts[0, n]) == 0
    assert int(counts[1, n]) == len(same) and not counts[1, :n].any()
    assert int(counts[2, n]) == 3 and not counts[2, :n].any()
    assert not counts[3].any() and not counts[4].any() and not counts[5].any()
    assert flagged == [0, 1, 2]
    plan.close()


PROFILES = [(1, 3), (3, 2), (4, 2), (6, 3), (16, 4), (10, 8), (20, 12), (10, 20)]


@pytest.mark.parametrize("k,m", PROFILES)
def test_profiles(native_lib, k, m):
    """The 4-, 8- and 16-row instances; RS(10,20) examines 16 of its 20 compared shards and
    ignores flipped bytes in the other four."""
    from callfs_amd.device import Plan
    n = k + m
    sizes = [8192 + 16 * 3 + 5, 9, 100, 2 * 8192 + 16, 33]
    masks = [_mask(n, ()), _mask(n, ()), _mask(n, (0,)), _mask(n, (n - 1,)), _mask(n, ())]
    ar = _Arena(k, m, sizes, masks, "aligned", seed=100 * k + m)
    plan = Plan.locate(k, m, sizes, ar.ptrs, present=masks)
    assert plan.forms() == ["locate"] and plan.bytes == _bytes(k, sizes, masks)
    rng = np.random.default_rng(k * 31 + m)
    hits = {}
    for b, S in enumerate(sizes[:4]):
        v, c = _examined(k, masks[b])
        shard = v[int(rng.integers(0, len(v)))] if b % 2 == 0 else c[int(rng.integers(0, len(c)))]
        hits[(b, shard)] = rng.choice(S, size=min(S, 37), replace=False)
    if m > 16:  # present shards past the 16th compared one: neither read nor blamed
        for b in (0, 4):
            hits[(b, k + 16 + b % 4)] = np.arange(sizes[b])
    counts, flagged = ar.run(plan, hits)
    _same(counts, ar.expected(hits))
    assert flagged == [0, 1, 2, 3]
    for b in range(4):
        assert int(counts[b].sum()) == min(sizes[b], 37)
    if m - 1 >= 2:  # every stripe has two compared shards or more: all blamed, none unexplained
        assert not counts[:, n].any()
    plan.close()


def test_reads_accumulate_and_clear(native_lib):
    import torch
    from callfs_amd.device import Plan
    k, m, n = 6, 3, 9
    sizes = [8192 + 21, 16, 3 * 8192]
    masks = [_mask(n, ()), _mask(n, (8,)), _mask(n, (0,))]
    ar = _Arena(k, m, sizes, masks, "aligned", seed=7)
    plan = Plan.locate(k, m, sizes, ar.ptrs, present=masks)
    hits = {(0, 1): [0, 8191, 8192, 8212], (1, 7): [15], (2, 4): np.arange(3 * 8192)}
    exp = ar.expected(hits)
    counts, _ = ar.run(plan, hits)
    _same(counts, exp)
    assert not plan.blame().any()  # the read cleared them
    plan.launch()
    plan.launch()
    _same(plan.blame(), exp * np.uint64(2))
    assert plan.corrupt_stripes() == [0, 1, 2] and plan.corrupt_stripes() == []
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        plan.launch(s)
    torch.cuda.synchronize()
    _same(plan.blame(s), exp)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch(s)
    assert not plan.blame(s).any()  # capturing ran nothing
    g.replay()
    g.replay()
    torch.cuda.synchronize()  # the replays run on the current stream, the read on s
    _same(plan.blame(s), exp * np.uint64(2))
    assert plan.corrupt_stripes(s) == [0, 1, 2]
    assert ar.unchanged() == []
    plan.close()


def test_plan_properties_and_api_edges(native_lib):
    import ctypes
    import torch
    from callfs_amd import _native as N
    from callfs_amd.device import Plan, RaggedBatch
    k, m, n = 10, 4, 14
    sizes = [8192 + 16 * 3 + 5, 11, 4000, 16]
    batch = len(sizes)
    masks = [_mask(n, (0,)), _mask(n, (1, 12)), _mask(n, ()), _mask(n, (2, 3, 4, 5))]
    ar = _Arena(k, m, sizes, masks, "aligned", seed=33)

    def code(fn, *a, **kw):
        with pytest.raises(N.NativeError) as ei:
            fn(*a, **kw)
        return ei.value.code

    assert code(Plan.locate, k, m, [sizes[0], 0, 4000, 16], ar.ptrs, present=masks) == N.RS_E_NO_DATA
    short = [list(x) for x in masks]
    short[2] = _mask(n, (0, 1, 2, 3, 4))
    assert code(Plan.locate, k, m, sizes, ar.ptrs, present=short) == N.RS_E_TOO_FEW_SHARDS
    assert code(Plan.locate, 0, 4, sizes, ar.ptrs[:4 * batch], present=[mk[:4] for mk in masks]) == \
        N.RS_E_INVALID_PROFILE
    with pytest.raises(ValueError):
        Plan.locate(k, m, sizes, ar.ptrs, present=masks[:3])

    L = N.lib
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    plan = Plan.locate(k, m, sizes, ar.ptrs, present=np.array(masks, dtype=bool))
    assert int(L.rs_plan_groups(plan.handle)) == 1 and plan.forms() == ["locate"]
    forms = (ctypes.c_int * 1)()
    assert L.rs_plan_forms(plan.handle, forms, 1) == 1 and forms[0] == 8192
    assert plan.bytes == sizes[0] * 13 + 11 * 12 + 4000 * 14  # stripe 3 has exactly k present
    assert plan.tune() == ["none"] and L.rs_tune_table_entries() == 0
    assert code(plan.set_orders, ["consecutive"]) == N.RS_E_ARG
    plan.set_orders(["none"])
    assert L.rs_plan_launch_ceiling(plan.handle, s, 1) == N.RS_E_ARG
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    plan.launch(events=(e0, e1))
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) > 0
    assert not plan.blame().any() and not plan.corrupt() and ar.unchanged() == []
    assert L.rs_plan_blame(plan.handle, s, None) == N.RS_E_ARG
    plan.close()

    # present = None: every shard present; all sizes equal is still a locate plan
    same = [4000] * batch
    ar2 = _Arena(k, m, same, [_mask(n, ())] * batch, "aligned", seed=34)
    plan = Plan.locate(k, m, same, ar2.ptrs)
    assert plan.forms() == ["locate"] and plan.bytes == 4000 * 14 * batch
    counts, flagged = ar2.run(plan, {(2, 13): [3999]})
    assert int(counts[2, 13]) == 1 and int(counts.sum()) == 1 and flagged == [2]
    plan.close()

    # no stripe has a row: no launch group, nothing enqueued, zero counts
    none = [_mask(n, (0, 5, 12, 13)), _mask(n, (1, 2, 3, 4))]
    ar3 = _Arena(k, m, [100, 9000], none, "packed", seed=35)
    plan = Plan.locate(k, m, [100, 9000], ar3.ptrs, present=none)
    assert int(L.rs_plan_groups(plan.handle)) == 0 and plan.forms() == [] and plan.bytes == 0
    plan.launch(events=(e0, e1))
    counts, flagged = ar3.run(plan, {(0, 1): [5], (1, 13): [0]})
    assert not counts.any() and flagged == []
    plan.close()

    # rs_plan_blame is a locate plan's alone
    rb = RaggedBatch(k, m, sizes, torch.device("cuda:0"))
    rb.fill_random(3)
    ragged = Plan.for_ragged(rb)
    out = (ctypes.c_uint64 * (batch * (n + 1)))()
    assert L.rs_plan_blame(ragged.handle, s, out) == N.RS_E_ARG
    ragged.close()
    via = Plan.for_ragged(rb, locate=True)
    assert via.forms() == ["locate"]
    via.close()


_SLICED_CHILD = r"""
import sys
import numpy as np
import torch
from callfs_amd.device import Plan, RaggedBatch

k, m, n = 2, 2, 4
sizes = [53 * 8192 + b % 17 for b in range(40)] + [8192, 5, 8193, 16]
batch = len(sizes)
rb = RaggedBatch(k, m, sizes, torch.device("cuda:0"))
rb.fill_random(11)
enc = Plan.for_ragged(rb)   # encode first, so that the stripes are consistent
enc.launch()
torch.cuda.synchronize()
enc.close()
# stripe b loses shard b % 4 when b % 7 == 2 (r' = 1), every fifth stripe two (no row)
masks = []
for b in range(batch):
    lost = [b % n, (b + 1) % n] if b % 5 == 0 else [b % n] if b % 7 == 2 else []
    masks.append([i not in lost for i in range(n)])
tiles = [max(1, -(-(sizes[b] // 16) // 512)) if sum(masks[b]) > k else 0 for b in range(batch)]
assert sum(tiles) > 1024
# the slice boundary at tile 1024 falls inside stripe `cut`: corrupt it on both sides
edge = np.cumsum(tiles)
cut = int(np.searchsorted(edge, 1024, side="right"))
assert sum(masks[cut]) == n and edge[cut] - tiles[cut] < 1024 < edge[cut]
col = (1024 - (int(edge[cut]) - tiles[cut])) * 8192
exp = np.zeros((batch, n + 1), dtype=np.uint64)
cols = np.arange(col - 300, col + 500)
rb.shard(cut, 0)[torch.from_numpy(cols).cuda()] ^= 0x21
exp[cut, 0] = cols.size
r1 = next(b for b in range(batch) if sum(masks[b]) == k + 1 and sizes[b] > 8192 and b != cut)
rb.shard(r1, masks[r1].index(True))[100:164] ^= 0x80
exp[r1, n] = 64
last = batch - 2  # 8193 bytes, everything present
assert sum(masks[last]) == n
rb.shard(last, 3)[8192] ^= 1
exp[last, 3] = 1
before = rb.buf.cpu().numpy()
plan = Plan.for_ragged(rb, present=masks, locate=True)
assert plan.forms() == ["locate"], plan.forms()
plan.launch()
got = plan.blame()
flagged = plan.corrupt_stripes()
bad = int(not np.array_equal(got, exp)) + int(flagged != sorted({cut, r1, last}))
bad += int(not np.array_equal(rb.buf.cpu().numpy(), before))
if bad:
    print("counts", np.argwhere(got != exp)[:8].tolist(), "flagged", flagged, "cut", cut, r1, last)
plan.close()
print("sliced locate child:", "ok" if not bad else "%d mismatches" % bad)
sys.exit(1 if bad else 0)
"""


def test_sliced_grid(native_lib):
    """CALLFS_RS_MAX_TILES_PER_LAUNCH is read once per process: a fresh child runs a batch of
    more than 1,024 tiles in slices of at most 1,024, the cut inside a stripe that is corrupt
    on both sides of it, with stripes that are in no launch; the counts are the same."""
    env = dict(os.environ)
    env["CALLFS_RS_MAX_TILES_PER_LAUNCH"] = "1024"
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _SLICED_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sliced locate child: ok" in r.stdout
