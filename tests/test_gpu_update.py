"""Update device plans (rs_plan_create_update): upstream Update and EncodeIdx
on device memory. One launch sets parity ^= P[:, changed] * (old ^ new) over stripes with their
own sizes and changed sets. Expected bytes come from the C oracle alone: for Update the parity
is cref.encode of the new data, for EncodeIdx the starting parity XOR cref.apply(P[:, changed],
shards). Every case asserts on the CPU, before the launch, that old != new in every changed
shard and that the expected parity differs from the starting parity of every changed stripe, so
a kernel that does nothing cannot pass; every other byte of a sentinel-filled allocation -- old
shards, new shards, the gaps between all buffers, the parity of unchanged stripes -- must stay
what it was."""
import ctypes
import functools
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


def _cycle(k, batch):
    sets = [(0,), (k - 1,), (3, 7), tuple(range(k)), (), (0, 1, 2)]
    return [tuple(i for i in sets[b % len(sets)] if i < k) for b in range(batch)]


@functools.lru_cache(maxsize=None)
def _reference(k, m, sizes, changed, seed, pair=True):
    """Per stripe (old data [k][S], new data [k][S], starting parity [m][S], expected parity
    [m][S]), computed once per case and shared read-only."""
    rng = np.random.default_rng(seed)
    E = cref.encode_matrix(k, m)
    out = []
    for S, ch in zip(sizes, changed):
        old = rng.integers(0, 256, (k, S), dtype=np.uint8)
        new = old.copy()
        for i in ch:
            new[i] = rng.integers(0, 256, S, dtype=np.uint8)
            new[i][0] = old[i][0] ^ 0x80  # differs whatever the draw
            assert not np.array_equal(new[i], old[i])
        if pair:
            par0 = np.stack(cref.encode(list(old), k, m))
            want = np.stack(cref.encode(list(new), k, m)) if ch else par0
        else:  # EncodeIdx: any starting parity
            par0 = rng.integers(0, 256, (m, S), dtype=np.uint8)
            want = par0 ^ np.stack(cref.apply(E[k:, list(ch)], [new[i] for i in ch])) if ch else par0
        if ch:  # every entry of P is non-zero (MDS): one changed shard changes every parity row
            assert not np.array_equal(want, par0)
            assert len(ch) > 1 or all(not np.array_equal(want[j], par0[j]) for j in range(m))
        for a in (old, new, par0, want):
            a.setflags(write=False)
        out.append((old, new, par0, want))
    return out


class _Arena:
    """A sentinel-filled allocation holding, per stripe, k old shards, the new shards of the
    changed indices and m parity shards, with sentinel gaps between all buffers. aligned: every
    buffer on a 256-B boundary; packed: every buffer at its own odd offset."""

    def __init__(self, k, m, sizes, changed, layout, seed, pair=True, guard=4096):
        import torch
        dev = torch.device("cuda:0")
        self.k, self.m, self.sizes, self.changed, self.pair = k, m, list(sizes), changed, pair
        self.ref = _reference(k, m, tuple(sizes), tuple(changed), seed, pair)
        off = 0

        def take(S):
            nonlocal off
            off += 16
            off = (off + 255) // 256 * 256 if layout == "aligned" else (off + 2 * (len(spans) % 7)) | 1
            spans.append((off, S))
            off += S
            return spans[-1][0]

        spans = []
        self.old_off = [[take(S) for _ in range(k)] for S in sizes]
        self.new_off = [[take(S) if i in ch else None for i in range(k)] for S, ch in zip(sizes, changed)]
        self.par_off = [[take(S) for _ in range(m)] for S in sizes]
        if layout == "packed":
            assert all(o % 2 == 1 for o, _ in spans)
        self.nbytes = off + 16
        start = np.full(self.nbytes, SENTINEL, dtype=np.uint8)
        for b, (old, new, par0, exp) in enumerate(self.ref):
            S = sizes[b]
            for i in range(k):
                start[self.old_off[b][i]:self.old_off[b][i] + S] = old[i]
                if self.new_off[b][i] is not None:
                    start[self.new_off[b][i]:self.new_off[b][i] + S] = new[i]
        want = start.copy()
        for b, (old, new, par0, exp) in enumerate(self.ref):
            S = sizes[b]
            for j in range(m):
                o = self.par_off[b][j]
                start[o:o + S] = par0[j]
                want[o:o + S] = exp[j]
        self.raw = torch.full((self.nbytes + 2 * guard + 256,), SENTINEL, dtype=torch.uint8, device=dev)
        self.lead = guard + (-(self.raw.data_ptr() + guard) % 256)
        self.raw[self.lead:self.lead + self.nbytes].copy_(torch.from_numpy(start))
        torch.cuda.synchronize()
        self.start_img = self.raw.cpu().numpy()
        self.want_img = self.start_img.copy()
        self.want_img[self.lead:self.lead + self.nbytes] = want
        base = self.raw.data_ptr() + self.lead
        # pointers of unchanged shards are never read: null
        self.old_ptrs = [base + self.old_off[b][i] if i in changed[b] else 0
                         for b in range(len(sizes)) for i in range(k)]
        self.new_ptrs = [base + self.new_off[b][i] if i in changed[b] else 0
                         for b in range(len(sizes)) for i in range(k)]
        self.par_ptrs = [base + o for row in self.par_off for o in row]
        self.flags = [[i in ch for i in range(k)] for ch in changed]

    def plan(self):
        from callfs_amd.device import Plan
        return Plan.update(self.k, self.m, self.sizes, self.flags,
                           self.old_ptrs if self.pair else None, self.new_ptrs, self.par_ptrs)

    def wrong(self, image=None):
        import torch
        torch.cuda.synchronize()
        want = self.want_img if image is None else image
        return np.flatnonzero(self.raw.cpu().numpy() != want)[:8].tolist()

    def bytes(self):
        return sum(S * (len(ch) * (2 if self.pair else 1) + 2 * self.m)
                   for S, ch in zip(self.sizes, self.changed) if ch)


def _check(k, m, sizes, changed, layout="aligned", seed=1, pair=True):
    ar = _Arena(k, m, sizes, changed, layout, seed, pair)
    plan = ar.plan()
    groups = (m + 15) // 16 if any(changed) else 0
    assert plan.forms() == ["update"] * groups
    assert plan.bytes == ar.bytes()
    assert ar.wrong(ar.start_img) == []
    plan.launch()
    assert ar.wrong() == [], (k, m, layout)
    assert not plan.corrupt()
    return ar, plan


@pytest.mark.parametrize("layout", ["aligned", "packed"])
def test_sizes_and_changed_sets(native_lib, layout):
    """RS(10,4) over the tail-only stripe, one vector, vector plus tail, both sides of the tile
    edge and several tiles; changed sets {0}, {9}, {3,7}, all ten, none, {0,1,2}."""
    changed = _cycle(10, len(SIZES))
    assert {len(c) for c in changed} == {0, 1, 2, 3, 10}
    ar, plan = _check(10, 4, SIZES, changed, layout, seed=5)
    plan.close()


def test_involution(native_lib):
    """A launch applies the delta: the second restores the starting parity byte for byte, the
    third equals the first."""
    ar, plan = _check(10, 4, SIZES, _cycle(10, len(SIZES)), "packed", seed=6)
    plan.launch()
    assert ar.wrong(ar.start_img) == []
    plan.launch()
    assert ar.wrong() == []
    plan.close()


@pytest.mark.parametrize("k,m", [(1, 3), (3, 2), (16, 4), (10, 8), (20, 12), (10, 20)])
def test_profiles(native_lib, k, m):
    """The 4-, 8- and 16-row instances and two launch groups (RS(10,20): 16 + 4 rows)."""
    sizes = [17, 8193] * 3
    ar, plan = _check(k, m, sizes, _cycle(k, len(sizes)), "packed", seed=100 * k + m)
    assert int(native_lib.lib.rs_plan_groups(plan.handle)) == (m + 15) // 16
    plan.close()


def test_wide_lds(native_lib):
    """RS(200,16) with 130 changed shards: 130 * 512 B of tables, past 64 KiB of LDS."""
    k, m = 200, 16
    changed = [tuple(range(3, 133)), (199,)]
    assert len(changed[0]) * 512 > 64 << 10
    ar, plan = _check(k, m, [40, 40], changed, "aligned", seed=9)
    plan.close()


@pytest.mark.parametrize("layout", ["aligned", "packed"])
def test_encode_idx_from_random_parity(native_lib, layout):
    ar, plan = _check(10, 4, SIZES, _cycle(10, len(SIZES)), layout, seed=7, pair=False)
    plan.close()


def test_encode_idx_progressive(native_lib):
    """k one-shard plans launched in a shuffled order over zeroed parity give cref.encode."""
    import torch
    from callfs_amd.device import Plan
    k, m = 10, 4
    sizes = [17, 8193, 5, 3 * 8192]
    rng = np.random.default_rng(17)
    dev = torch.device("cuda:0")
    data = [rng.integers(1, 256, (k, S), dtype=np.uint8) for S in sizes]
    want = [np.stack(cref.encode(list(d), k, m)) for d in data]
    assert all(w.any() for w in want)
    dd = [torch.from_numpy(d).to(dev) for d in data]
    par = [torch.zeros((m, S), dtype=torch.uint8, device=dev) for S in sizes]
    pp = [par[b][j].data_ptr() for b in range(len(sizes)) for j in range(m)]
    order = [int(i) for i in rng.permutation(k)]
    assert order != sorted(order)
    for i in order:
        flags = [[q == i for q in range(k)]] * len(sizes)
        new = [dd[b][q].data_ptr() if q == i else 0 for b in range(len(sizes)) for q in range(k)]
        plan = Plan.update(k, m, sizes, flags, None, new, pp)
        assert plan.bytes == sum(S * (1 + 2 * m) for S in sizes)
        plan.launch()
        torch.cuda.synchronize()
        plan.close()
    for b in range(len(sizes)):
        assert np.array_equal(par[b].cpu().numpy(), want[b]), b
        assert np.array_equal(dd[b].cpu().numpy(), data[b]), b


def test_graph_capture(native_lib):
    """One replay updates, two replays restore."""
    import torch
    sizes = [65_541, 9, 8192, 3 * 8192 + 17, 100, 40_000]
    ar = _Arena(10, 4, sizes, _cycle(10, len(sizes)), "aligned", seed=41)
    plan = ar.plan()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture: two launches leave the parity as it was
        plan.launch(s)
        plan.launch(s)
    torch.cuda.synchronize()
    assert ar.wrong(ar.start_img) == []
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch(s)
    assert ar.wrong(ar.start_img) == []  # capture runs nothing
    g.replay()
    assert ar.wrong() == []
    g.replay()
    assert ar.wrong(ar.start_img) == []
    plan.close()


_SLICED_CHILD = r"""
import sys
import numpy as np
import torch
from oracle import cref
from callfs_amd.device import Plan

k, m = 2, 1
sizes = [35 * 8192 + b % 17 for b in range(60)] + [8192, 5, 8193, 16]
tiles = sum(max(1, -(-(S // 16) // 512)) for S in sizes)
assert tiles >= 2100 and (tiles // 3) % 35 != 0, tiles   # 3 slices, cut inside stripes
rng = np.random.default_rng(3)
dev = torch.device("cuda:0")
bad = 0
old, new, par, want, flags = [], [], [], [], []
for b, S in enumerate(sizes):
    o = rng.integers(0, 256, (k, S), dtype=np.uint8)
    n = o.copy()
    ch = [b % 2] if b % 5 else [0, 1]
    for i in ch:
        n[i] ^= rng.integers(1, 256, S, dtype=np.uint8)
    p0 = np.stack(cref.encode(list(o), k, m))
    w = np.stack(cref.encode(list(n), k, m))
    assert not np.array_equal(p0, w)
    old.append(torch.from_numpy(o).to(dev)); new.append(torch.from_numpy(n).to(dev))
    par.append(torch.from_numpy(p0).to(dev)); want.append(w)
    flags.append([i in ch for i in range(k)])
B = len(sizes)
plan = Plan.update(k, m, sizes, flags,
                   [old[b][i].data_ptr() for b in range(B) for i in range(k)],
                   [new[b][i].data_ptr() for b in range(B) for i in range(k)],
                   [par[b][j].data_ptr() for b in range(B) for j in range(m)])
assert plan.forms() == ["update"], plan.forms()
plan.launch()
torch.cuda.synchronize()
for b in range(B):
    if not np.array_equal(par[b].cpu().numpy(), want[b]):
        print("mismatch: stripe", b, "size", sizes[b])
        bad += 1
plan.close()
print("sliced update child:", "ok" if not bad else "%d mismatches" % bad)
sys.exit(1 if bad else 0)
"""


def test_sliced_grid(native_lib):
    """CALLFS_RS_MAX_TILES_PER_LAUNCH is read once per process: a fresh child runs an RS(2,1)
    batch of at least 2,100 tiles in slices of at most 1,024, with slice boundaries inside
    stripes, bit-exact against the oracle."""
    env = dict(os.environ)
    env["CALLFS_RS_MAX_TILES_PER_LAUNCH"] = "1024"
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _SLICED_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sliced update child: ok" in r.stdout


def test_api_edges(native_lib):
    """The error order of the header with nothing created; an all-unchanged plan; tuning,
    pinning, ceilings and forms."""
    import torch
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    k, m = 10, 4
    sizes = [8192 + 16 * 3 + 5, 11, 4000, 16]
    B = len(sizes)
    changed = [(0,), (1, 9), (), (2, 3, 4, 5)]
    ar = _Arena(k, m, sizes, changed, "aligned", seed=33)
    L = N.lib
    ctx = N.default_context()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda p: (ctypes.c_void_p * len(p))(*p)  # noqa: E731
    fl = lambda rows: (ctypes.c_uint8 * (B * k))(*[1 if f else 0 for r in rows for f in r])  # noqa: E731
    sz = lambda v: (ctypes.c_size_t * B)(*v)  # noqa: E731

    def create(kk=k, mm=m, sizes_=sizes, flags=ar.flags, old=ar.old_ptrs, new=ar.new_ptrs,
               par=ar.par_ptrs, null=()):
        h = ctypes.c_void_p(0xdead)
        args = {"sizes": sz(sizes_), "changed": fl(flags), "old": vp(old) if old is not None else None,
                "new": vp(new), "parity": vp(par)}
        for name in null:
            args[name] = None
        rc = L.rs_plan_create_update(ctx.handle, 0, kk, mm, B, args["sizes"], args["changed"],
                                     args["old"], args["new"], args["parity"], ctypes.byref(h))
        if rc != 0:
            assert h.value in (None, 0xdead)  # nothing created
        return rc, h

    # 1. the profile, before anything else (here: with NULL arrays, a zero size and NULL pointers too)
    zero = list(sizes)
    zero[0] = 0
    assert create(kk=0, null=("sizes", "new"))[0] == N.RS_E_INVALID_PROFILE
    assert create(kk=250, mm=10, sizes_=zero)[0] == N.RS_E_UNSUPPORTED
    # 2. NULL arrays, before a zero size
    for name in ("sizes", "changed", "new", "parity"):
        assert create(sizes_=zero, null=(name,))[0] == N.RS_E_ARG, name
    assert L.rs_plan_create_update(ctx.handle, 0, k, m, B, sz(sizes), fl(ar.flags), vp(ar.old_ptrs),
                                   vp(ar.new_ptrs), vp(ar.par_ptrs), None) == N.RS_E_ARG
    # 3. a zero size on a changed stripe, before a NULL pointer
    nonew = list(ar.new_ptrs)
    nonew[1 * k + 9] = 0
    assert create(sizes_=zero, new=nonew)[0] == N.RS_E_NO_DATA
    zero_unchanged = list(sizes)
    zero_unchanged[2] = 0  # stripe 2 has no change: its size does not matter
    rc, h = create(sizes_=zero_unchanged)
    assert rc == 0
    L.rs_plan_destroy(h)
    # 4. NULL pointers of a changed shard
    assert create(new=nonew)[0] == N.RS_E_ARG
    noold = list(ar.old_ptrs)
    noold[3 * k + 2] = 0
    assert create(old=noold)[0] == N.RS_E_ARG
    rc, h = create(old=None)  # EncodeIdx mode: no old pointers at all
    assert rc == 0
    L.rs_plan_destroy(h)
    nopar = list(ar.par_ptrs)
    nopar[0 * m + 3] = 0
    assert create(par=nopar)[0] == N.RS_E_ARG
    nopar = list(ar.par_ptrs)
    nopar[2 * m + 1] = 0  # of the unchanged stripe: never read
    rc, h = create(par=nopar)
    assert rc == 0
    L.rs_plan_destroy(h)
    with pytest.raises(ValueError):
        Plan.update(k, m, sizes, ar.flags[:3], ar.old_ptrs, ar.new_ptrs, ar.par_ptrs)

    # an all-unchanged plan: no launch group, nothing enqueued, no bytes
    none = [[False] * k] * B
    plan = Plan.update(k, m, sizes, none, [0] * (B * k), [0] * (B * k), [0] * (B * m))
    assert int(L.rs_plan_groups(plan.handle)) == 0 and plan.forms() == [] and plan.bytes == 0
    plan.launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    plan.launch(events=(e0, e1))
    assert ar.wrong(ar.start_img) == [] and not plan.corrupt()
    plan.close()

    plan = ar.plan()
    assert int(L.rs_plan_groups(plan.handle)) == 1 and plan.forms() == ["update"]
    forms = (ctypes.c_int * 1)()
    assert L.rs_plan_forms(plan.handle, forms, 1) == 1 and forms[0] == 4096  # RS_ORDER_UPDATE
    # the tuner times nothing: the parity is untouched
    assert plan.tune() == ["none"]
    assert ar.wrong(ar.start_img) == []
    assert L.rs_tune_table_entries() == 0
    with pytest.raises(N.NativeError) as ei:
        plan.set_orders(["consecutive"])
    assert ei.value.code == N.RS_E_ARG
    plan.set_orders(["none"])
    for mode in (1, 2):
        assert L.rs_plan_launch_ceiling(plan.handle, s, mode) == N.RS_E_ARG
    assert ar.wrong(ar.start_img) == []
    e0.record()
    e1.record()
    plan.launch(events=(e0, e1))
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) > 0
    assert ar.wrong() == [] and not plan.corrupt()
    plan.close()
