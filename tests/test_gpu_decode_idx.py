"""Decode-idx device plans (rs_plan_create_decode_idx): upstream DecodeIdx on
device memory. A launch adds (or, in store mode, stores) C[:, delivered] * inputs into the wanted
shards of stripes with their own sizes, expected sets and wanted sets; C = E[w] * inv(E[expected]).
Expected bytes come from the C oracle alone: cref.reconstruct with present = expect for a
complete feed, and cref.apply(C[:, delivered], inputs) for a partial one, where C itself is
cref.reconstruct of the k unit vectors. Every case asserts on the CPU, before anything is
launched, that every delivered shard is non-zero in its first byte and that every launch changes
every wanted row of every stripe it covers, so a kernel that does nothing cannot pass; every other
byte of a sentinel-filled allocation -- inputs, unwanted and unexpected shards, the gaps between
all buffers, the guards, stripes in no launch -- must stay what it was."""
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
SIZES = (1, 5, 15, 16, 17, 40, 1023, 1024, 1025, 8191, 8192, 8193, 8208, 2 * 8192 + 83, 7)


def _expected_sets(k, m, batch):
    """Per stripe k of the k+m indices: first k, last k, and two sets that mix data and parity."""
    n = k + m
    evens = (list(range(0, n, 2)) + list(range(1, n, 2)))[:k]  # the even indices, then odd ones up to k
    cyc = [tuple(range(k)), tuple(range(n - k, n)), tuple(sorted(evens)),
           tuple(sorted(set(range(n)) - set(range(1, 1 + m))))]
    assert all(len(set(e)) == k for e in cyc), cyc
    return tuple(cyc[b % 4] for b in range(batch))


def _wanted_sets(k, m, expect):
    """Per stripe: all that are not expected, one, two, none -- cycled out of step with the
    expected sets."""
    out = []
    for b, e in enumerate(expect):
        rest = [i for i in range(k + m) if i not in e]
        out.append(tuple([rest, rest[-1:], rest[:1] + rest[-1:] if len(rest) > 1 else rest, []][(b // 4 + b) % 4]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _coef(k, m, expect):
    """C as an (n, k) array: row w, column j = the coefficient of expected shard V[j] in shard w
    (rows of expected shards are unit rows). cref.reconstruct of the k unit vectors."""
    n = k + m
    shards = [None] * n
    for j, v in enumerate(expect):
        shards[v] = np.zeros(k, dtype=np.uint8)
        shards[v][j] = 1
    full = cref.reconstruct(shards, [i in expect for i in range(n)], k, m)
    C = np.stack(full)
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def _reference(k, m, sizes, expect, feeds, seed):
    """Per stripe (data [k][S] of the expected shards in ascending index order, full [n][S] =
    cref.reconstruct from them, C [n][k]). feeds: per launch the positions in V delivered with it
    (the same positions for every stripe). Data is redrawn until, for every launch, the launch's
    terms are non-zero in the first byte of every shard that is not expected."""
    rng = np.random.default_rng(seed)
    out = []
    for S, e in zip(sizes, expect):
        C = _coef(k, m, e)
        rest = [i for i in range(k + m) if i not in e]
        while True:
            data = rng.integers(0, 256, (k, S), dtype=np.uint8)
            data[:, 0] |= 1  # every delivered shard is non-zero in its first byte
            first = [cref.apply(C[rest][:, list(f)], [data[j][:1] for j in f]) for f in feeds]
            if all(t[0] != 0 for terms in first for t in terms):
                break
        shards = [None] * (k + m)
        for j, v in enumerate(e):
            shards[v] = data[j]
        full = np.stack(cref.reconstruct(shards, [i in e for i in range(k + m)], k, m))
        for j, v in enumerate(e):
            assert np.array_equal(full[v], data[j])
        data.setflags(write=False)
        full.setflags(write=False)
        out.append((data, full, C))
    return out


def _terms(ref, feed, S):
    """[n][S]: the terms a launch delivering the positions `feed` adds to every shard (rows of
    expected shards are not used)."""
    data, full, C = ref
    return np.stack(cref.apply(C[:, list(feed)], [data[j] for j in feed]))


class _Arena:
    """A sentinel-filled allocation holding all k+m shards of every stripe with sentinel gaps
    between all buffers. aligned: every buffer on a 256-B boundary; packed: every buffer at its
    own odd offset. Expected shards hold the data; the others start as `start` says: "zero",
    "junk" (random, and differing from what the first launch leaves in the first byte) or
    "random"."""

    def __init__(self, k, m, sizes, expect, wanted, feeds, layout, seed, start="zero", guard=4096):
        import torch
        dev = torch.device("cuda:0")
        self.k, self.m, self.n, self.sizes = k, m, k + m, list(sizes)
        self.expect, self.wanted, self.feeds = expect, wanted, feeds
        self.ref = _reference(k, m, tuple(sizes), tuple(expect), tuple(tuple(f) for f in feeds), seed)
        rng = np.random.default_rng(seed + 1000)
        off = 0
        spans = []

        def take(S):
            nonlocal off
            off += 16
            off = (off + 255) // 256 * 256 if layout == "aligned" else (off + 2 * (len(spans) % 7)) | 1
            spans.append((off, S))
            off += S
            return spans[-1][0]

        self.off = [[take(S) for _ in range(self.n)] for S in sizes]
        if layout == "packed":
            assert all(o % 2 == 1 for o, _ in spans)
        self.nbytes = off + 16
        img = np.full(self.nbytes, SENTINEL, dtype=np.uint8)
        for b, (data, full, C) in enumerate(self.ref):
            S = sizes[b]
            t0 = _terms(self.ref[b], feeds[0], S) if feeds else None
            for i in range(self.n):
                o = self.off[b][i]
                if i in expect[b]:
                    img[o:o + S] = data[expect[b].index(i)]
                elif start == "zero":
                    img[o:o + S] = 0
                else:
                    img[o:o + S] = rng.integers(0, 256, S, dtype=np.uint8)
                    if start == "junk" and t0 is not None:
                        img[o] = t0[i][0] ^ 0x80
        self.raw = torch.full((self.nbytes + 2 * guard + 256,), SENTINEL, dtype=torch.uint8, device=dev)
        self.lead = guard + (-(self.raw.data_ptr() + guard) % 256)
        self.raw[self.lead:self.lead + self.nbytes].copy_(torch.from_numpy(img))
        torch.cuda.synchronize()
        self.start_img = self.raw.cpu().numpy()
        self.base = self.raw.data_ptr() + self.lead

    def plan(self, feed, store=False, skip=()):
        """The plan that delivers positions `feed` of V in every stripe not in `skip`."""
        from callfs_amd.device import Plan
        inp, dst, flags = [], [], []
        for b in range(len(self.sizes)):
            deliver = set() if b in skip else {self.expect[b][j] for j in feed}
            for i in range(self.n):
                inp.append(self.base + self.off[b][i] if i in deliver else 0)
                dst.append(self.base + self.off[b][i] if i in self.wanted[b] else 0)
            flags.append([i in self.expect[b] for i in range(self.n)])
        return Plan.decode_idx(self.k, self.m, self.sizes, flags, inp, dst, store=store)

    def after(self, image, feed, store=False, skip=()):
        """`image` after a launch of plan(feed, store, skip), from the oracle's terms; asserts
        that every wanted row of every stripe in the launch changes."""
        out = image.copy()
        for b, S in enumerate(self.sizes):
            if b in skip or not self.wanted[b] or not feed:
                continue
            t = _terms(self.ref[b], feed, S)
            for w in self.wanted[b]:
                o = self.lead + self.off[b][w]
                new = t[w] if store else out[o:o + S] ^ t[w]
                assert not np.array_equal(new, out[o:o + S]), (b, w)
                out[o:o + S] = new
        return out

    def complete(self, image):
        """`image` with every wanted shard holding cref.reconstruct's bytes."""
        out = image.copy()
        for b, S in enumerate(self.sizes):
            for w in self.wanted[b]:
                o = self.lead + self.off[b][w]
                out[o:o + S] = self.ref[b][1][w]
        return out

    def wrong(self, image):
        import torch
        torch.cuda.synchronize()
        return np.flatnonzero(self.raw.cpu().numpy() != image)[:8].tolist()

    def bytes(self, feed, store, skip=()):
        return sum(S * (len(feed) + (1 if store else 2) * len(w))
                   for b, (S, w) in enumerate(zip(self.sizes, self.wanted)) if w and feed and b not in skip)


def _feeds(k, kind, seed):
    perm = [int(i) for i in np.random.default_rng(seed).permutation(k)]
    if kind == "all":
        return (tuple(range(k)),)
    if kind == "singles":
        assert k < 3 or perm != sorted(perm)
        return tuple((i,) for i in perm)
    if kind == "3+7":
        return (tuple(sorted(perm[:3])), tuple(sorted(perm[3:])))
    if kind == "halves":
        return tuple(f for f in (tuple(sorted(perm[:k // 2])), tuple(sorted(perm[k // 2:]))) if f)
    raise AssertionError(kind)


def _run_feeds(ar, store_first):
    """Launches the feeds in order (the first in store mode when store_first), checking the image
    after every launch against the oracle's terms and, at the end, against cref.reconstruct."""
    img = ar.start_img
    groups = max((len(w) + 15) // 16 for w in ar.wanted)
    for q, feed in enumerate(ar.feeds):
        store = store_first and q == 0
        want = ar.after(img, feed, store)
        plan = ar.plan(feed, store)
        assert plan.forms() == ["decode-idx"] * groups
        assert plan.bytes == ar.bytes(feed, store)
        plan.launch()
        assert ar.wrong(want) == [], (q, feed, store)
        assert not plan.corrupt()
        plan.close()
        img = want
    assert ar.wrong(ar.complete(ar.start_img)) == []
    return img


@pytest.mark.parametrize("start", ["merge-from-zero", "store-first-over-junk"])
@pytest.mark.parametrize("feed", ["all", "singles", "3+7"])
@pytest.mark.parametrize("layout", ["aligned", "packed"])
def test_sizes_sets_and_feeds(native_lib, layout, feed, start):
    """RS(10,4) over the tail-only stripe, one vector, vector plus tail, both sides of the wave
    edge and the tile edge and a tail behind full tiles; every stripe its own expected set (first
    k, last k, two that mix data and parity) and wanted set (all four, one, two, none)."""
    k, m = 10, 4
    expect = _expected_sets(k, m, len(SIZES))
    wanted = _wanted_sets(k, m, expect)
    assert {len(w) for w in wanted} == {0, 1, 2, 4}
    assert any(any(i >= k for i in e) and any(i < k for i in e) for e in expect)
    store_first = start.startswith("store")
    ar = _Arena(k, m, SIZES, expect, wanted, _feeds(k, feed, 11), layout, seed=5,
                start="junk" if store_first else "zero")
    _run_feeds(ar, store_first)


def test_partial_feed(native_lib):
    """From random destinations a merge launch gives start ^ terms; a second identical launch
    restores the start and a third equals the first. A store launch over junk gives the terms
    exactly, twice. Stripe 2 is delivered nothing and keeps every byte."""
    k, m = 10, 4
    sizes = SIZES[3:]
    expect = _expected_sets(k, m, len(sizes))
    wanted = _wanted_sets(k, m, expect)
    feed = (1, 4, 8)
    ar = _Arena(k, m, sizes, expect, wanted, (feed,), "packed", seed=21, start="random")
    assert wanted[2]
    want = ar.after(ar.start_img, feed, skip=(2,))
    plan = ar.plan(feed, skip=(2,))
    assert plan.bytes == ar.bytes(feed, False, skip=(2,))
    plan.launch()
    assert ar.wrong(want) == []
    plan.launch()
    assert ar.wrong(ar.start_img) == []
    plan.launch()
    assert ar.wrong(want) == []
    plan.close()
    ar = _Arena(k, m, sizes, expect, wanted, (feed,), "aligned", seed=22, start="junk")
    want = ar.after(ar.start_img, feed, store=True, skip=(2,))
    plan = ar.plan(feed, store=True, skip=(2,))
    assert plan.bytes == ar.bytes(feed, True, skip=(2,))
    for _ in range(2):
        plan.launch()
        assert ar.wrong(want) == []
    plan.close()


def test_encode_idx_equivalence(native_lib):
    """expect = the data shards, dst = the parity, one delivered shard: bit for bit what an
    update plan in EncodeIdx mode gives from the same starting parity."""
    import torch
    from callfs_amd.device import Plan
    k, m = 10, 4
    sizes = list(SIZES)
    B = len(sizes)
    expect = tuple(tuple(range(k)) for _ in sizes)
    wanted = tuple(tuple(range(k, k + m)) for _ in sizes)
    feed = (6,)
    a1 = _Arena(k, m, sizes, expect, wanted, (feed,), "packed", seed=31, start="random")
    a2 = _Arena(k, m, sizes, expect, wanted, (feed,), "packed", seed=31, start="random")
    want = a1.after(a1.start_img, feed)
    want2 = a2.after(a2.start_img, feed)
    flags = [[i == 6 for i in range(k)]] * B
    new = [a2.base + a2.off[b][i] if i == 6 else 0 for b in range(B) for i in range(k)]
    par = [a2.base + a2.off[b][k + j] for b in range(B) for j in range(m)]
    up = Plan.update(k, m, sizes, flags, None, new, par)
    up.launch()
    di = a1.plan(feed)
    assert di.bytes == up.bytes
    di.launch()
    torch.cuda.synchronize()
    got = [a.raw.cpu().numpy()[a.lead:a.lead + a.nbytes] for a in (a1, a2)]
    assert np.array_equal(got[0], got[1])
    assert a1.wrong(want) == [] and a2.wrong(want2) == []
    up.close()
    di.close()


@pytest.mark.parametrize("k,m", [(1, 3), (3, 2), (4, 2), (16, 4), (10, 8), (20, 12), (10, 20)])
def test_profiles(native_lib, k, m):
    """The 4-, 8- and 16-row instances in both modes, and two launch groups (RS(10,20): 16 + 4
    rows, beside stripes with fewer than 17 wanted rows, which the second launch leaves alone):
    the first half of the expected shards stored over junk, the second half merged."""
    sizes = [17, 8193] * 4
    expect = _expected_sets(k, m, len(sizes))
    wanted = _wanted_sets(k, m, expect)
    ar = _Arena(k, m, sizes, expect, wanted, _feeds(k, "halves", 100 * k + m), "packed", seed=100 * k + m,
                start="junk")
    groups = (m + 15) // 16
    plan = ar.plan(ar.feeds[0], store=True)
    assert int(native_lib.lib.rs_plan_groups(plan.handle)) == groups
    plan.close()
    _run_feeds(ar, store_first=True)


def test_wide_lds(native_lib):
    """RS(200,16) with 130 delivered shards: 130 * 512 B of tables, past 64 KiB of LDS; then the
    other 70."""
    k, m = 200, 16
    sizes = [40, 40]
    expect = (tuple(range(k)), tuple(range(16, k + 16)))
    wanted = (tuple(range(k, k + m)), (0, 7, 15))
    feeds = (tuple(range(3, 133)), tuple(range(3)) + tuple(range(133, 200)))
    assert len(feeds[0]) * 512 > 64 << 10 and sorted(feeds[0] + feeds[1]) == list(range(k))
    for store_first in (False, True):
        ar = _Arena(k, m, sizes, expect, wanted, feeds, "aligned", seed=9, start="junk" if store_first else "zero")
        _run_feeds(ar, store_first)


def test_graph_capture(native_lib):
    """A captured merge launch: one replay merges, two replays restore."""
    import torch
    k, m = 10, 4
    sizes = [65_541, 9, 8192, 3 * 8192 + 17, 100, 40_000]
    expect = _expected_sets(k, m, len(sizes))
    wanted = _wanted_sets(k, m, expect)
    feed = (0, 9)
    ar = _Arena(k, m, sizes, expect, wanted, (feed,), "aligned", seed=41, start="random")
    want = ar.after(ar.start_img, feed)
    plan = ar.plan(feed)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture: two launches leave the shards as they were
        plan.launch(s)
        plan.launch(s)
    torch.cuda.synchronize()
    assert ar.wrong(ar.start_img) == []
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch(s)
    assert ar.wrong(ar.start_img) == []  # capture runs nothing
    g.replay()
    assert ar.wrong(want) == []
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
n = 3
sizes = [35 * 8192 + b % 17 for b in range(60)] + [8192, 5, 8193, 16]
tiles = sum(max(1, -(-(S // 16) // 512)) for S in sizes)
assert tiles >= 2100 and (tiles // 3) % 35 != 0, tiles   # 3 slices, cut inside stripes
rng = np.random.default_rng(3)
dev = torch.device("cuda:0")
bad = 0
bufs, want, flags, inp, dst = [], [], [], [], []
for b, S in enumerate(sizes):
    e = [(0, 1), (1, 2), (0, 2)][b % 3]
    w = [i for i in range(n) if i not in e][0]
    shards = [None] * n
    for i in e:
        shards[i] = rng.integers(1, 256, S, dtype=np.uint8)
    full = np.stack(cref.reconstruct(shards, [i in e for i in range(n)], k, m))
    assert full[w][0] != 0 or full[w].any()
    start = full.copy()
    start[w] = full[w] ^ 0xFF  # junk that differs everywhere
    t = torch.from_numpy(start).to(dev)
    bufs.append(t); want.append(full)
    flags.append([i in e for i in range(n)])
    inp += [t[i].data_ptr() if i in e else 0 for i in range(n)]
    dst += [t[i].data_ptr() if i == w else 0 for i in range(n)]
plan = Plan.decode_idx(k, m, sizes, flags, inp, dst, store=True)
assert plan.forms() == ["decode-idx"], plan.forms()
plan.launch()
torch.cuda.synchronize()
for b in range(len(sizes)):
    if not np.array_equal(bufs[b].cpu().numpy(), want[b]):
        print("mismatch: stripe", b, "size", sizes[b])
        bad += 1
plan.close()
print("sliced decode-idx child:", "ok" if not bad else "%d mismatches" % bad)
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
    assert "sliced decode-idx child: ok" in r.stdout


def test_api_edges(native_lib):
    """The error order the header states, with nothing created; a plan with nothing delivered;
    tuning, pinning, ceilings, forms, groups and bytes."""
    import torch
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    header = open(os.path.join(ROOT, "include", "callfs_rs.h")).read()
    assert "#define RS_ORDER_DECODE_IDX 32768" in header and "#define RS_DECODE_IDX_STORE 1u" in header
    assert "A MERGE LAUNCH IS NOT IDEMPOTENT" in header
    k, m, n = 10, 4, 14
    sizes = [8192 + 16 * 3 + 5, 11, 4000, 16]
    B = len(sizes)
    expect = _expected_sets(k, m, B)
    wanted = _wanted_sets(k, m, expect)
    feed = (2, 5)
    ar = _Arena(k, m, sizes, expect, wanted, (feed,), "aligned", seed=33, start="random")
    L = N.lib
    ctx = N.default_context()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    flags0 = [[i in expect[b] for i in range(n)] for b in range(B)]
    inp0 = [ar.base + ar.off[b][i] if i in {expect[b][j] for j in feed} else 0 for b in range(B) for i in range(n)]
    dst0 = [ar.base + ar.off[b][i] if i in wanted[b] else 0 for b in range(B) for i in range(n)]
    vp = lambda p: (ctypes.c_void_p * len(p))(*[x or None for x in p])  # noqa: E731
    fl = lambda rows: (ctypes.c_uint8 * (B * n))(*[1 if f else 0 for r in rows for f in r])  # noqa: E731
    sz = lambda v: (ctypes.c_size_t * B)(*v)  # noqa: E731

    def create(kk=k, mm=m, sizes_=sizes, flags=flags0, inp=inp0, dst=dst0, bits=0, null=()):
        h = ctypes.c_void_p(0xdead)
        args = {"sizes": sz(sizes_), "expect": fl(flags), "input": vp(inp), "dst": vp(dst)}
        for name in null:
            args[name] = None
        rc = L.rs_plan_create_decode_idx(ctx.handle, 0, kk, mm, B, args["sizes"], args["expect"],
                                         args["input"], args["dst"], bits, ctypes.byref(h))
        if rc != 0:
            assert h.value in (None, 0xdead)  # nothing created
        return rc, h

    def ok(**kw):
        rc, h = create(**kw)
        assert rc == 0
        L.rs_plan_destroy(h)

    zero = list(sizes)
    zero[0] = 0
    few = [list(r) for r in flags0]
    few[1][expect[1][0]] = False
    many = [list(r) for r in flags0]
    many[3][wanted[3][0] if wanted[3] else [i for i in range(n) if i not in expect[3]][0]] = True
    misplaced_in = list(inp0)
    misplaced_in[2 * n + [i for i in range(n) if i not in expect[2]][0]] = ar.base
    misplaced_dst = list(dst0)
    misplaced_dst[0 * n + expect[0][3]] = ar.base
    # 1. the profile, before anything else
    assert create(kk=0, null=("sizes", "input"), bits=2)[0] == N.RS_E_INVALID_PROFILE
    assert create(kk=250, mm=10, flags=few)[0] == N.RS_E_UNSUPPORTED
    # 2. NULL arrays, counts and flag bits, before the expect count
    for name in ("sizes", "expect", "input", "dst"):
        assert create(flags=few, null=(name,))[0] == N.RS_E_ARG, name
    assert L.rs_plan_create_decode_idx(ctx.handle, 0, k, m, B, sz(sizes), fl(flags0), vp(inp0), vp(dst0), 0,
                                       None) == N.RS_E_ARG
    for bits in (2, 3, 1 << 31):
        assert create(flags=few, bits=bits)[0] == N.RS_E_ARG
    # 3. the expect count, before misplaced pointers and sizes
    assert create(flags=few, inp=misplaced_in, sizes_=zero)[0] == N.RS_E_TOO_FEW_SHARDS
    many_rc = create(flags=many, sizes_=zero)[0]
    assert many_rc == N.RS_E_ARG
    # 4. misplaced pointers, before a zero size
    assert create(inp=misplaced_in, sizes_=zero)[0] == N.RS_E_ARG
    assert create(dst=misplaced_dst, sizes_=zero)[0] == N.RS_E_ARG
    # 5. a zero size on a stripe with both an input and a dst; not on one without
    assert wanted[0] and not wanted[3]
    assert create(sizes_=zero)[0] == N.RS_E_NO_DATA
    idle = list(sizes)
    idle[3] = 0  # stripe 3 wants nothing
    ok(sizes_=idle)
    noin = [0 if i < n else p for i, p in enumerate(inp0)]  # stripe 0 delivered nothing
    ok(sizes_=zero, inp=noin)
    ok(bits=1)
    with pytest.raises(ValueError):
        Plan.decode_idx(k, m, sizes, flags0[:3], inp0, dst0)
    with pytest.raises(ValueError):
        Plan.decode_idx(k, m, sizes, flags0, inp0[:-1], dst0)

    # nothing delivered: no launch group, nothing enqueued, no bytes
    for store in (False, True):
        plan = Plan.decode_idx(k, m, sizes, flags0, [0] * (B * n), dst0, store=store)
        assert int(L.rs_plan_groups(plan.handle)) == 0 and plan.forms() == [] and plan.bytes == 0
        plan.launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        e1.record()
        plan.launch(events=(e0, e1))
        assert ar.wrong(ar.start_img) == [] and not plan.corrupt()
        plan.close()

    plan = ar.plan(feed)
    assert int(L.rs_plan_groups(plan.handle)) == 1 and plan.forms() == ["decode-idx"]
    forms = (ctypes.c_int * 1)()
    assert L.rs_plan_forms(plan.handle, forms, 1) == 1 and forms[0] == 32768  # RS_ORDER_DECODE_IDX
    assert plan.bytes == ar.bytes(feed, False)
    st = ar.plan(feed, store=True)
    assert st.bytes == ar.bytes(feed, True) < plan.bytes
    st.close()
    assert plan.tune() == ["none"]  # the tuner times nothing: no byte is touched
    assert ar.wrong(ar.start_img) == []
    assert L.rs_tune_table_entries() == 0
    with pytest.raises(N.NativeError) as ei:
        plan.set_orders(["consecutive"])
    assert ei.value.code == N.RS_E_ARG
    plan.set_orders(["none"])
    for mode in (1, 2):
        assert L.rs_plan_launch_ceiling(plan.handle, s, mode) == N.RS_E_ARG
    assert ar.wrong(ar.start_img) == []
    want = ar.after(ar.start_img, feed)
    e0.record()
    e1.record()
    plan.launch(events=(e0, e1))
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) > 0
    assert ar.wrong(want) == [] and not plan.corrupt()
    plan.close()
