"""Pair locate device plans (rs_plan_create_locate_ex with max_errors = 2):
a stripe that compares four or more shards also names the two shards of a byte column in
which two are corrupt, and such a column counts once for each of them. Stripes are consistent
(parity from the C oracle); the expected counts are what the test itself corrupted, every XOR
nonzero -- exact, no tolerance. After every launch every byte of the sentinel-guarded
allocation is what it was before."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A
SIZES = [1, 15, 16, 17, 40, 8191, 8193, 2 * 8192 + 83]


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

    def expected(self, hits, max_errors=2):
        """Counts from the hits alone: per column, the examined shards the test changed."""
        exp = np.zeros((len(self.sizes), self.n + 1), dtype=np.uint64)
        for b, S in enumerate(self.sizes):
            valid, cmp = _examined(self.k, self.masks[b])
            rows = len(cmp)
            if not rows:
                continue
            per_col = {}
            for (hb, i), cols in hits.items():
                if hb == b and i in valid + cmp:
                    for c in np.unique(np.asarray(cols)):
                        per_col.setdefault(int(c), []).append(i)
            for shards in per_col.values():
                e = len(shards)
                if rows == 1:
                    exp[b, self.n] += 1
                elif e == 1:
                    exp[b, shards[0]] += 1
                elif e == 2 and rows >= 4 and max_errors == 2:
                    exp[b, shards[0]] += 1
                    exp[b, shards[1]] += 1
                else:
                    top = rows - 2 if rows >= 4 and max_errors == 2 else rows - 1
                    assert e <= top, "the rule promises nothing here"
                    exp[b, self.n] += 1
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


# (valid, valid) with shard 0, (valid, valid), (valid, compared), (compared, compared)
PAIRS_10_4 = [(0, 7), (3, 9), (5, 12), (10, 13)]


@pytest.mark.parametrize("layout", ["aligned", "packed"])
def test_sizes_layouts_and_pairs(native_lib, layout):
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    masks = [_mask(n, ())] * len(SIZES)
    ar = _Arena(k, m, SIZES, masks, layout, seed=41)
    plan = Plan.locate(k, m, SIZES, ar.ptrs, present=masks, max_errors=2)
    assert plan.forms() == ["locate"] and plan.bytes == sum(SIZES) * n
    counts, flagged = ar.run(plan, {})
    assert not counts.any() and flagged == []
    for a, b2 in PAIRS_10_4:
        # the edge columns, then a whole shard; every fourth stripe left clean
        for whole in (False, True):
            hits = {}
            for b, S in enumerate(SIZES):
                if b % 4 == 3:
                    continue
                cols = np.arange(S) if whole else _edge_columns(S)
                hits[(b, a)] = cols
                hits[(b, b2)] = cols
            counts, flagged = ar.run(plan, hits)
            _same(counts, ar.expected(hits))
            for b, S in enumerate(SIZES):
                want = 0 if b % 4 == 3 else S if whole else len(_edge_columns(S))
                assert int(counts[b, a]) == want and int(counts[b, b2]) == want, (a, b2, b)
                assert int(counts[b].sum()) == 2 * want and int(counts[b, n]) == 0
            assert flagged == [b for b in range(len(SIZES)) if b % 4 != 3]
    counts, flagged = ar.run(plan, {})
    assert not counts.any() and flagged == []
    plan.close()


def test_mixed_columns(native_lib):
    """Single-error columns, pair columns and, in one lane's 16 columns, both; two different
    pairs in one lane; a pair next to a single of one of its shards."""
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [2 * 8192 + 16 * 7 + 5, 4000]
    masks = [_mask(n, ()), _mask(n, ())]
    ar = _Arena(k, m, sizes, masks, "packed", seed=43)
    plan = Plan.locate(k, m, sizes, ar.ptrs, present=masks, max_errors=2)
    S0 = sizes[0]
    hits = {
        # lane of columns 160..175: shard 2 alone in 160..167, shards 2 and 11 in 168..171,
        # shard 11 alone in 172..173, shards 0 and 11 in 174..175
        (0, 2): list(range(160, 172)) + list(range(9000, 9100)),
        (0, 11): list(range(168, 176)) + [8191, 8192, S0 - 1],
        (0, 0): [174, 175, 8191, 8192, S0 - 1] + list(range(300, 340)),
        # stripe 1: a pair over whole lanes, then singles
        (1, 4): list(range(0, 64)) + [3999],
        (1, 13): list(range(32, 96)),
    }
    counts, flagged = ar.run(plan, hits)
    _same(counts, ar.expected(hits))
    assert int(counts[0, n]) == 0 and int(counts[1, n]) == 0
    assert int(counts[0, 2]) == 112 and int(counts[0, 11]) == 11 and int(counts[0, 0]) == 45
    assert int(counts[1, 4]) == 65 and int(counts[1, 13]) == 64
    assert flagged == [0, 1]
    # the single plan over the same bytes: pair columns are unexplained, singles the same
    single = Plan.locate(k, m, sizes, ar.ptrs, present=masks)
    plan1 = Plan.locate(k, m, sizes, ar.ptrs, present=masks, max_errors=1)
    single.launch()
    plan1.launch()
    c1 = single.blame()
    _same(c1, ar.expected(hits, max_errors=1))
    _same(plan1.blame(), c1)
    assert int(c1[0, n]) == 4 + 2 + 3 and int(c1[1, n]) == 32
    for p in (plan, single, plan1):
        p.close()


def test_short_of_four_rows(native_lib):
    """r' = 3, 1 and 0: a pair plan counts what the single plan counts; a same-column pair is
    unexplained."""
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [8192 + 16 * 5 + 3, 9000, 5000, 40]
    masks = [_mask(n, (6,)), _mask(n, (0,)), _mask(n, (1, 2, 12)), _mask(n, (3, 4, 5, 13))]
    ar = _Arena(k, m, sizes, masks, "aligned", seed=47)
    pair = Plan.locate(k, m, sizes, ar.ptrs, present=masks, max_errors=2)
    single = Plan.locate(k, m, sizes, ar.ptrs, present=masks)
    same = [0, 1, 15, 16, 1023, 1024, 8191, 8192, 8200, sizes[0] - 1]
    hits = {
        (0, 2): same + list(range(100, 140)), (0, 11): same, (0, 13): list(range(200, 230)),
        (1, 1): [0, 8999], (1, 12): [0, 8999], (1, 5): list(range(4096, 4200)),
        (2, 0): [1, 7], (2, 13): [9],           # r' = 1
        (3, 0): [0, 39],                        # exactly k present: in no launch
    }
    counts, flagged = ar.run(pair, hits)
    single.launch()
    c1 = single.blame()
    _same(counts, c1)
    _same(counts, ar.expected(hits))
    assert int(counts[0, n]) == len(same) and int(counts[0, 2]) == 40 and int(counts[0, 13]) == 30
    assert int(counts[1, n]) == 2 and int(counts[1, 5]) == 104
    assert int(counts[2, n]) == 3 and not counts[3].any()
    assert flagged == [0, 1, 2]
    pair.close()
    single.close()


def test_three_in_a_column(native_lib):
    """RS(10,6), r' = 6: three shards corrupt in the same columns are exactly unexplained
    (3 <= r' - 2), beside pair and single columns that are blamed."""
    from callfs_amd.device import Plan
    k, m, n = 10, 6, 16
    sizes = [8192 + 16 * 9 + 7, 100]
    masks = [_mask(n, ()), _mask(n, ())]
    ar = _Arena(k, m, sizes, masks, "packed", seed=53)
    plan = Plan.locate(k, m, sizes, ar.ptrs, present=masks, max_errors=2)
    three = _edge_columns(sizes[0])
    four = [2000, 2001, 2017]
    hits = {(0, 0): three + four, (0, 6): three + four, (0, 12): three + four + [4000, 4001],
            (0, 15): four + [4000, 4001, 5000],
            (1, 3): np.arange(100), (1, 10): np.arange(100), (1, 14): np.arange(100)}
    counts, flagged = ar.run(plan, hits)
    _same(counts, ar.expected(hits))
    assert int(counts[0, n]) == len(three) + len(four) and int(counts[1, n]) == 100
    assert int(counts[0, 12]) == 2 and int(counts[0, 15]) == 3 and not counts[1, :n].any()
    assert flagged == [0, 1]
    plan.close()


PROFILES = [(1, 4), (6, 4), (16, 4), (10, 8), (20, 12), (10, 20)]


@pytest.mark.parametrize("k,m", PROFILES)
def test_profiles(native_lib, k, m):
    """The 4-, 8- and 16-row instances, one pair case each: a stripe with everything present
    and, where m > 4, one with two shards missing."""
    from callfs_amd.device import Plan
    n = k + m
    sizes = [8192 + 16 * 3 + 5, 2 * 8192 + 16, 33]
    lost = (0, n - 1) if m > 4 else ()
    masks = [_mask(n, ()), _mask(n, lost), _mask(n, ())]
    ar = _Arena(k, m, sizes, masks, "aligned", seed=100 * k + m)
    plan = Plan.locate(k, m, sizes, ar.ptrs, present=masks, max_errors=2)
    assert plan.forms() == ["locate"]
    rng = np.random.default_rng(k * 31 + m)
    hits, want = {}, {}
    for b, S in enumerate(sizes):
        v, c = _examined(k, masks[b])
        # stripe 0: the first examined shard (shard 0) and a compared one; then two compared
        # ones; then a valid and a compared one
        if b == 0:
            a, b2 = v[0], c[int(rng.integers(0, len(c)))]
        elif b == 1:
            a, b2 = c[0], c[-1]
        else:
            a, b2 = v[-1], c[1]
        cols = np.unique(np.concatenate([rng.choice(S, size=min(S, 37), replace=False), _edge_columns(S)]))
        hits[(b, a)] = cols
        hits[(b, b2)] = cols
        want[b] = (a, b2, cols.size)
    counts, flagged = ar.run(plan, hits)
    _same(counts, ar.expected(hits))
    for b, (a, b2, ncols) in want.items():
        assert int(counts[b, a]) == ncols and int(counts[b, b2]) == ncols and int(counts[b].sum()) == 2 * ncols
    assert flagged == [0, 1, 2]
    plan.close()


def test_max_errors_one_is_the_single_plan(native_lib):
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [8192 + 37, 300, 17]
    masks = [_mask(n, ()), _mask(n, (4,)), _mask(n, ())]
    ar = _Arena(k, m, sizes, masks, "packed", seed=59)
    hits = {(0, 1): _edge_columns(sizes[0]), (0, 12): [0, 5, 8191, 8200], (1, 7): [0, 299], (1, 9): [299],
            (2, 0): [16], (2, 13): [3]}
    old = Plan.locate(k, m, sizes, ar.ptrs, present=masks)
    one = Plan.locate(k, m, sizes, ar.ptrs, present=masks, max_errors=1)
    c_old, f_old = ar.run(old, hits)
    c_one, f_one = ar.run(one, hits)
    _same(c_one, c_old)
    _same(c_old, ar.expected(hits, max_errors=1))
    assert f_one == f_old == [0, 1, 2]
    assert int(c_old[0, n]) == 3 and int(c_old[1, n]) == 1  # columns 0, 5 and 8191; column 299
    assert one.forms() == old.forms() == ["locate"] and one.bytes == old.bytes
    for me, code in ((0, N.RS_E_ARG), (3, N.RS_E_UNSUPPORTED)):
        with pytest.raises(N.NativeError) as ei:
            Plan.locate(k, m, sizes, ar.ptrs, present=masks, max_errors=me)
        assert ei.value.code == code
    old.close()
    one.close()


def test_reads_accumulate_and_clear(native_lib):
    import ctypes
    import torch
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    k, m, n = 6, 4, 10
    sizes = [8192 + 21, 16, 3 * 8192]
    masks = [_mask(n, ()), _mask(n, ()), _mask(n, ())]
    ar = _Arena(k, m, sizes, masks, "aligned", seed=7)
    plan = Plan.locate(k, m, sizes, ar.ptrs, present=masks, max_errors=2)
    forms = (ctypes.c_int * 1)()
    assert N.lib.rs_plan_forms(plan.handle, forms, 1) == 1 and forms[0] == 8192
    assert int(N.lib.rs_plan_groups(plan.handle)) == 1 and plan.bytes == sum(sizes) * n
    whole = np.arange(3 * 8192)
    hits = {(0, 1): [0, 8191, 8192, 8212], (0, 8): [0, 8191, 8192, 8212, 100], (1, 7): [15], (1, 0): [15],
            (2, 4): whole, (2, 5): whole}
    exp = ar.expected(hits)
    assert int(exp[2, 4]) == 3 * 8192 == int(exp[2, 5]) and int(exp[:, n].sum()) == 0
    counts, _ = ar.run(plan, hits)
    _same(counts, exp)
    assert not plan.blame().any()  # the read cleared them
    plan.launch()
    plan.launch()
    _same(plan.blame(), exp * np.uint64(2))
    assert plan.corrupt_stripes() == [0, 1, 2] and plan.corrupt_stripes() == []
    assert ar.unchanged() == []
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


_SLICED_CHILD = r"""
import sys
import numpy as np
import torch
from callfs_amd.device import Plan, RaggedBatch

k, m, n = 2, 4, 6
sizes = [53 * 8192 + b % 17 for b in range(30)] + [8192, 5, 8193, 16]
batch = len(sizes)
rb = RaggedBatch(k, m, sizes, torch.device("cuda:0"))
rb.fill_random(11)
enc = Plan.for_ragged(rb)   # encode first, so that the stripes are consistent
enc.launch()
torch.cuda.synchronize()
enc.close()
# every fifth stripe has exactly k shards (no row), stripe b with b % 7 == 2 loses one (r' = 3)
masks = []
for b in range(batch):
    lost = [(b + j) % n for j in range(4)] if b % 5 == 0 else [b % n] if b % 7 == 2 else []
    masks.append([i not in lost for i in range(n)])
tiles = [max(1, -(-(sizes[b] // 16) // 512)) if sum(masks[b]) > k else 0 for b in range(batch)]
assert sum(tiles) > 1024
# the slice boundary at tile 1024 falls inside stripe `cut`: corrupt two of its shards in the
# same columns on both sides
edge = np.cumsum(tiles)
cut = int(np.searchsorted(edge, 1024, side="right"))
assert sum(masks[cut]) == n and edge[cut] - tiles[cut] < 1024 < edge[cut]
col = (1024 - (int(edge[cut]) - tiles[cut])) * 8192
exp = np.zeros((batch, n + 1), dtype=np.uint64)
cols = torch.from_numpy(np.arange(col - 300, col + 500)).cuda()
rb.shard(cut, 0)[cols] ^= 0x21
rb.shard(cut, 4)[cols] ^= 0x47
exp[cut, 0] = exp[cut, 4] = 800
r3 = next(b for b in range(batch) if sum(masks[b]) == n - 1 and b != cut)
pres = [i for i in range(n) if masks[r3][i]]
rb.shard(r3, pres[0])[100:164] ^= 0x80
rb.shard(r3, pres[-1])[100:164] ^= 0x03
exp[r3, n] = 64   # r' = 3: a same-column pair is unexplained
last = batch - 2  # 8193 bytes, everything present
assert sum(masks[last]) == n
rb.shard(last, 3)[8192] ^= 1
rb.shard(last, 1)[8192] ^= 0xfe
rb.shard(last, 5)[17] ^= 9
exp[last, 3] = exp[last, 1] = exp[last, 5] = 1
before = rb.buf.cpu().numpy()
plan = Plan.for_ragged(rb, present=masks, locate=True, max_errors=2)
assert plan.forms() == ["locate"], plan.forms()
plan.launch()
got = plan.blame()
flagged = plan.corrupt_stripes()
bad = int(not np.array_equal(got, exp)) + int(flagged != sorted({cut, r3, last}))
bad += int(not np.array_equal(rb.buf.cpu().numpy(), before))
if bad:
    print("counts", np.argwhere(got != exp)[:8].tolist(), "flagged", flagged, "cut", cut, r3, last)
plan.close()
print("sliced pair locate child:", "ok" if not bad else "%d mismatches" % bad)
sys.exit(1 if bad else 0)
"""


def test_sliced_grid(native_lib):
    """CALLFS_RS_MAX_TILES_PER_LAUNCH is read once per process: a fresh child runs a batch of
    more than 1,024 tiles in slices of at most 1,024, the cut inside a stripe in which two
    shards are corrupt in the same columns on both sides of it; the counts are the same."""
    env = dict(os.environ)
    env["CALLFS_RS_MAX_TILES_PER_LAUNCH"] = "1024"
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _SLICED_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sliced pair locate child: ok" in r.stdout
