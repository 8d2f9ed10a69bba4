"""Required device plans (rs_plan_create_required): one launch rebuilds only
the missing shards a caller wants, over stripes with their own sizes, masks and wanted sets.
Every case is bit-exact against the C oracle: a wanted shard holds cref.reconstruct's bytes
for it, and every other byte of a sentinel-filled allocation -- the unwanted missing shards
included -- is what it was before the launch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A
SIZES = [1, 5, 15, 16, 17, 40, 8191, 8192, 8193, 8208, 2 * 8192 + 83, 3 * 8192, 7]
UNIFORM_FORMS_EXCLUDED = ("required", "ragged", "mixed", "none")


@pytest.fixture(autouse=True)
def _no_tuned_forms(native_lib):
    native_lib.lib.rs_tune_table_reset(None)
    yield
    native_lib.lib.rs_tune_table_reset(None)


def _mask(n, lost):
    lost = set(lost)
    return [i not in lost for i in range(n)]


def _flags(n, on):
    on = set(on)
    return [i in on for i in range(n)]


def _cases(k, m, batch, seed):
    """Seeded masks with 1..m lost and a seeded wanted subset of the lost shards per stripe
    (plus flags on some present shards, which count for nothing). Stripes 0..3 are fixed:
    w = 0 with c > 0; w = m with c = 0; r = 0 (exactly k present, nothing wanted); every
    missing shard wanted."""
    n = k + m
    rng = np.random.default_rng(seed)
    masks, wanted = [], []
    for _ in range(batch):
        lost = [int(i) for i in rng.choice(n, size=int(rng.integers(1, m + 1)), replace=False)]
        w = [i for i in lost if rng.integers(0, 2)]
        noise = [int(i) for i in rng.choice(n, size=2, replace=False) if int(i) not in lost]
        masks.append(_mask(n, lost))
        wanted.append(_flags(n, w + noise))
    masks[0], wanted[0] = _mask(n, (1,)), _flags(n, (0, n - 1))            # w = 0, c = m - 1
    masks[1], wanted[1] = _mask(n, range(1, m + 1)), _flags(n, range(n))   # w = m, c = 0
    masks[2], wanted[2] = _mask(n, range(k - 1, k - 1 + m)), _flags(n, ())  # r = 0
    masks[3], wanted[3] = _mask(n, (0, n - 1)), _flags(n, (0, n - 1))      # all wanted
    return masks, wanted


def _rows(k, mask, want):
    """(written shard indices, compared shard indices) of one stripe."""
    present = [i for i, p in enumerate(mask) if p]
    return [i for i, p in enumerate(mask) if not p and want[i]], present[k:]


def _bytes(k, sizes, masks, wanted):
    total = 0
    for S, mask, want in zip(sizes, masks, wanted):
        w, c = _rows(k, mask, want)
        if w or c:
            total += S * (k + len(w) + len(c))
    return total


def _groups(k, masks, wanted):
    return (max(sum(map(len, _rows(k, mk, wt))) for mk, wt in zip(masks, wanted)) + 15) // 16


def _stripes(k, m, sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for S in sizes:
        st = np.empty((k + m, S), dtype=np.uint8)
        st[:k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
        par = cref.encode([st[i] for i in range(k)], k, m)
        for j in range(m):
            st[k + j] = par[j]
        out.append(st)
    return out


class _Arena:
    """A sentinel-filled allocation with guards around a RaggedBatch-shaped body: the present
    shards hold a consistent stripe's bytes, every missing shard (wanted or not) and all
    padding hold the sentinel. `want` is the image the launch must leave: the wanted shards
    the oracle's, everything else unchanged."""

    def __init__(self, k, m, sizes, masks, wanted, layout, seed, guard=4096):
        import torch
        from callfs_amd.device import RaggedBatch
        dev = torch.device("cuda:0")
        self.k, self.m, self.n, self.sizes = k, m, k + m, list(sizes)
        self.rb = rb = RaggedBatch(k, m, sizes, dev, layout=layout)  # for the offsets
        self.stripes = _stripes(k, m, sizes, seed)
        start = np.full(rb.nbytes, SENTINEL, dtype=np.uint8)
        want = start.copy()
        for b, (st, mask, wt) in enumerate(zip(self.stripes, masks, wanted)):
            full = cref.reconstruct([st[i] if p else None for i, p in enumerate(mask)], mask, k, m)
            for i in range(self.n):
                o = rb.offsets[b][i]
                if mask[i]:
                    start[o:o + sizes[b]] = st[i]
                    want[o:o + sizes[b]] = st[i]
                elif wt[i]:
                    want[o:o + sizes[b]] = np.asarray(full[i])
        self.raw = torch.full((rb.nbytes + 2 * guard + 256,), SENTINEL, dtype=torch.uint8, device=dev)
        self.lead = guard + (-(self.raw.data_ptr() + guard) % 256)
        self.start = torch.from_numpy(start)
        self.reset()
        self.want = self.raw.cpu().numpy()
        self.want[self.lead:self.lead + rb.nbytes] = want
        base = self.raw.data_ptr() + self.lead
        self.ptrs = [base + o for row in rb.offsets for o in row]

    def reset(self):
        self.raw[self.lead:self.lead + self.rb.nbytes].copy_(self.start)

    def shard(self, b, i):
        o = self.lead + self.rb.offsets[b][i]
        return self.raw[o:o + self.sizes[b]]

    def wrong(self):
        import torch
        torch.cuda.synchronize()
        return np.flatnonzero(self.raw.cpu().numpy() != self.want)[:8].tolist()


def _check(k, m, sizes, masks, wanted, layout="aligned", seed=1):
    from callfs_amd.device import Plan
    ar = _Arena(k, m, sizes, masks, wanted, layout, seed)
    plan = Plan.ragged(k, m, sizes, ar.ptrs, present=masks, required=wanted)
    assert plan.forms() == ["required"] * _groups(k, masks, wanted)
    assert plan.bytes == _bytes(k, sizes, masks, wanted)
    plan.launch()
    assert ar.wrong() == [], (k, m, layout)
    assert not plan.corrupt()
    plan.close()


@pytest.mark.parametrize("layout", ["aligned", "packed"])
@pytest.mark.parametrize("k,m", [(10, 4), (6, 8), (5, 12), (3, 20)])
def test_sizes_and_profiles_vs_oracle(native_lib, k, m, layout):
    """The 4-, 8- and 16-row instances and two launch groups (RS(3,20): 16 + 4 rows, some
    stripes in the first group only), over the tail-only stripe, one vector, vector plus tail,
    both sides of the tile edge and several tiles."""
    masks, wanted = _cases(k, m, len(SIZES), seed=1000 * k + m)
    r = [sum(map(len, _rows(k, mk, wt))) for mk, wt in zip(masks, wanted)]
    w = [len(_rows(k, mk, wt)[0]) for mk, wt in zip(masks, wanted)]
    assert w[0] == 0 and r[0] == m - 1 > 0 and (w[1], r[1]) == (m, m) and r[2] == 0
    assert w[3] == masks[3].count(False)
    assert len({(tuple(a), tuple(b)) for a, b in zip(masks, wanted)}) > 6
    if m > 16:
        assert any(0 < x <= 16 for x in r) and sum(x > 16 for x in r) >= 2
    _check(k, m, SIZES, masks, wanted, layout, seed=k + m)


def test_flags_belong_to_their_stripe(native_lib):
    """A flipped byte in a compared shard of a stripe whose written rows are a strict subset
    of its missing shards flags exactly that stripe, in the vector part and in the S % 16
    tail (and in a stripe that is all tail); a flipped byte in an unwanted missing buffer
    flags nothing and stays."""
    import torch
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [2 * 8192 + 16 * 7 + 5, 9, 8192, 40, 8192 + 16 * 7 + 5, 13]
    masks, wanted = _cases(k, m, len(sizes), seed=31)
    for b in (4, 5):
        masks[b], wanted[b] = _mask(n, (0, 12)), _flags(n, (0,))  # written {0}, compared {11, 13}
        assert _rows(k, masks[b], wanted[b]) == ([0], [11, 13])
    ar = _Arena(k, m, sizes, masks, wanted, "packed", seed=3)
    plan = Plan.ragged(k, m, sizes, ar.ptrs, present=masks, required=wanted)
    assert plan.forms() == ["required"]

    def run():
        plan.launch()
        torch.cuda.synchronize()
        return plan.corrupt_stripes()

    assert run() == [] and ar.wrong() == []
    S = sizes[4]
    for b, i, off in ((4, 13, 16 * 3 + 1), (4, 11, 8192 + 5), (4, 13, S - 2), (5, 11, 12), (5, 13, 0)):
        ar.shard(b, i)[off] ^= 0x40
        assert run() == [b], (b, i, off)
        ar.shard(b, i)[off] ^= 0x40
        assert run() == []
    # the unwanted missing shard: never read, never written
    for b, off in ((4, 100), (4, S - 1), (5, 3)):
        ar.shard(b, 12)[off] ^= 0x40
        assert run() == []
        assert int(ar.shard(b, 12)[off]) == SENTINEL ^ 0x40
        ar.shard(b, 12)[off] ^= 0x40
    assert ar.wrong() == []
    plan.close()


def test_routing(native_lib):
    import torch
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [8192 + 16 * 3 + 5, 11, 4000, 16]
    batch = len(sizes)
    masks = [_mask(n, (0,)), _mask(n, (1, 12)), _mask(n, (3, 13)), _mask(n, (2, 3, 4, 5))]
    every = [[not p for p in mk] for mk in masks]
    ar = _Arena(k, m, sizes, masks, every, "aligned", seed=12)
    # nothing left out: the ragged plan itself
    ref = Plan.ragged(k, m, sizes, ar.ptrs, present=masks)
    for req in (None, every, [[True] * n] * batch):
        plan = Plan.ragged(k, m, sizes, ar.ptrs, present=masks, required=req)
        assert plan.forms() == ref.forms() == ["ragged"]
        assert plan.bytes == ref.bytes == n * sum(sizes)
        ar.reset()
        plan.launch()
        assert ar.wrong() == [] and not plan.corrupt()
        plan.close()
    ref.close()

    # one size, one (mask, wanted) pair: the uniform plan over the wanted rows
    S = 2 * 8192 + 16 * 5 + 3
    mask, want = _mask(n, (0, 12)), _flags(n, (0, 5))
    ar = _Arena(k, m, [S] * batch, [mask] * batch, [want] * batch, "aligned", seed=13)
    plan = Plan.ragged(k, m, [S] * batch, ar.ptrs, present=[mask] * batch, required=[want] * batch)
    forms = plan.forms()
    assert len(forms) == 1 and forms[0] in Plan.ORDER_NAMES.values()
    assert forms[0] not in UNIFORM_FORMS_EXCLUDED
    assert plan.bytes == batch * S * (k + 1 + 2)
    plan.launch()
    assert ar.wrong() == [] and not plan.corrupt()
    ar.shard(2, 13)[S - 1] ^= 1
    plan.launch()
    torch.cuda.synchronize()
    assert plan.corrupt_stripes() == [2]
    plan.close()

    # exactly k present and nothing wanted: no launch group, nothing enqueued
    mask, want = _mask(n, (0, 5, 12, 13)), _flags(n, (1,))
    ar = _Arena(k, m, [S] * batch, [mask] * batch, [want] * batch, "aligned", seed=14)
    plan = Plan.ragged(k, m, [S] * batch, ar.ptrs, present=[mask] * batch, required=[want] * batch)
    assert int(native_lib.lib.rs_plan_groups(plan.handle)) == 0 and plan.forms() == []
    assert plan.bytes == 0
    plan.launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    plan.launch(events=(e0, e1))
    assert ar.wrong() == [] and not plan.corrupt()
    plan.close()

    # a ragged batch whose stripes all have r = 0: a required plan with no launch group
    masks = [_mask(n, (0, 5, 12, 13)), _mask(n, (1, 2, 3, 4))]
    wanted = [_flags(n, ()), _flags(n, (0,))]
    ar = _Arena(k, m, [100, 9000], masks, wanted, "packed", seed=15)
    plan = Plan.ragged(k, m, [100, 9000], ar.ptrs, present=masks, required=wanted)
    assert plan.forms() == [] and plan.bytes == 0
    plan.launch()
    assert ar.wrong() == [] and not plan.corrupt()
    plan.close()


def test_api_edges(native_lib):
    """Errors are rs_plan_create_ragged's; tuning, pinning and ceilings as for a ragged plan;
    the one-shot call reports a flipped compared byte."""
    import ctypes
    import torch
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [8192 + 16 * 3 + 5, 11, 4000, 16]
    batch = len(sizes)
    masks = [_mask(n, (0,)), _mask(n, (1, 12)), _mask(n, ()), _mask(n, (2, 3, 4, 5))]
    wanted = [_flags(n, ()), _flags(n, (1,)), _flags(n, (0,)), _flags(n, (2, 5))]
    ar = _Arena(k, m, sizes, masks, wanted, "aligned", seed=33)

    def code(fn, *a, **kw):
        with pytest.raises(N.NativeError) as ei:
            fn(*a, **kw)
        return ei.value.code

    assert code(Plan.ragged, k, m, [sizes[0], 0, 4000, 16], ar.ptrs, present=masks,
                required=wanted) == N.RS_E_NO_DATA
    short = [list(x) for x in masks]
    short[2] = _mask(n, (0, 1, 2, 3, 4))
    assert code(Plan.ragged, k, m, sizes, ar.ptrs, present=short, required=wanted) == N.RS_E_TOO_FEW_SHARDS
    assert code(Plan.ragged, k, m, [16] * batch, ar.ptrs, present=short,
                required=wanted) == N.RS_E_TOO_FEW_SHARDS
    assert code(Plan.ragged, 0, 4, sizes, ar.ptrs[:4 * batch], present=[mk[:4] for mk in masks],
                required=[w[:4] for w in wanted]) == N.RS_E_INVALID_PROFILE
    with pytest.raises(ValueError):
        Plan.ragged(k, m, sizes, ar.ptrs, present=masks, required=wanted[:3])

    plan = Plan.ragged(k, m, sizes, ar.ptrs, present=masks, required=np.array(wanted, dtype=bool))
    L = N.lib
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert int(L.rs_plan_groups(plan.handle)) == 1 and plan.forms() == ["required"]
    assert plan.tune() == ["none"]
    assert L.rs_tune_table_entries() == 0
    assert code(plan.set_orders, ["consecutive"]) == N.RS_E_ARG
    plan.set_orders(["none"])
    assert L.rs_plan_launch_ceiling(plan.handle, s, 1) == N.RS_E_ARG
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    plan.launch(events=(e0, e1))
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) > 0
    assert ar.wrong() == [] and not plan.corrupt()
    plan.close()

    arr = (ctypes.c_void_p * len(ar.ptrs))(*ar.ptrs)
    szs = (ctypes.c_size_t * batch)(*sizes)
    pres = (ctypes.c_uint8 * (batch * n))(*[1 if p else 0 for mk in masks for p in mk])
    req = (ctypes.c_uint8 * (batch * n))(*[1 if p else 0 for w in wanted for p in w])
    ctx = N.default_context()

    def one_shot():
        torch.cuda.synchronize()
        return L.rs_decode_dev_required(ctx.handle, 0, k, m, batch, szs, pres, req, arr, s)

    ar.reset()
    assert one_shot() == 0 and ar.wrong() == []
    ar.shard(1, 13)[10] ^= 1  # stripe 1: written {1}, compared {11, 13}
    assert one_shot() == N.RS_E_CORRUPT
    ar.shard(1, 13)[10] ^= 1
    assert one_shot() == 0 and ar.wrong() == []


def test_graph_capture(native_lib):
    import torch
    from callfs_amd.device import Plan
    k, m = 10, 4
    sizes = [65_541, 9, 8192, 3 * 8192 + 17, 100, 40_000]
    masks, wanted = _cases(k, m, len(sizes), seed=77)
    ar = _Arena(k, m, sizes, masks, wanted, "aligned", seed=41)
    plan = Plan.ragged(k, m, sizes, ar.ptrs, present=masks, required=wanted)
    assert plan.forms() == ["required"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        plan.launch(s)
    torch.cuda.synchronize()
    assert not plan.corrupt(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch(s)
    for _ in range(2):
        ar.reset()
        torch.cuda.synchronize()
        g.replay()
        assert ar.wrong() == []
        assert not plan.corrupt(s)
    plan.close()


_SLICED_CHILD = r"""
import sys
import numpy as np
import torch
from oracle import cref
from callfs_amd.device import Plan, RaggedBatch

k, m, n = 2, 2, 4
sizes = [53 * 8192 + b % 17 for b in range(56)] + [8192, 5, 8193, 16]
batch = len(sizes)
rb = RaggedBatch(k, m, sizes, torch.device("cuda:0"))
# encode first, so that the stripes are consistent
rb.fill_random(11)
enc = Plan.for_ragged(rb)
enc.launch()
torch.cuda.synchronize()
enc.close()
full = rb.buf.cpu().numpy()

def stripe(img, b):
    return [img[o:o + sizes[b]] for o in rb.offsets[b]]

# stripe b loses shard b % 4 (wanted when b is even); every fifth stripe loses two shards
# and wants neither: no row, in no launch
masks, wanted = [], []
for b in range(batch):
    lost = [b % n] if b % 5 else [b % n, (b + 1) % n]
    masks.append([i not in lost for i in range(n)])
    wanted.append([i in lost and b % 2 == 0 and b % 5 != 0 for i in range(n)])
in_launch = [b for b in range(batch) if b % 5]
assert sum(max(1, -(-(sizes[b] // 16) // 512)) for b in in_launch) > 2048
want = full.copy()
for b in range(batch):
    for i in range(n):
        if not masks[b][i]:
            rb.shard(b, i).fill_(0x5A)
            o = rb.offsets[b][i]
            if not wanted[b][i]:
                want[o:o + sizes[b]] = 0x5A
plan = Plan.for_ragged(rb, present=masks, required=wanted)
assert plan.forms() == ["required"], plan.forms()
plan.launch()
torch.cuda.synchronize()
got = rb.buf.cpu().numpy()
bad = int(plan.corrupt())
for b in range(batch):
    sh = stripe(full, b)
    ref = cref.reconstruct([sh[i] if masks[b][i] else None for i in range(n)], masks[b], k, m)
    for i in range(n):
        exp = np.asarray(ref[i]) if masks[b][i] or wanted[b][i] else np.full(sizes[b], 0x5A, np.uint8)
        if not np.array_equal(stripe(got, b)[i], exp):
            print("mismatch: stripe", b, "shard", i, "size", sizes[b])
            bad += 1
bad += int(not np.array_equal(got, want))
plan.close()
print("sliced required child:", "ok" if not bad else "%d mismatches" % bad)
sys.exit(1 if bad else 0)
"""


def test_sliced_grid(native_lib):
    """CALLFS_RS_MAX_TILES_PER_LAUNCH is read once per process: a fresh child runs an RS(2,2)
    batch of more than 2,048 tiles in slices of at most 1,024, with slice boundaries inside
    stripes and stripes that are in no launch, bit-exact against the oracle."""
    env = dict(os.environ)
    env["CALLFS_RS_MAX_TILES_PER_LAUNCH"] = "1024"
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _SLICED_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sliced required child: ok" in r.stdout
