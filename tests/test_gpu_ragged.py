"""Ragged device plans (rs_plan_create_ragged): one launch encodes, repairs
and verifies a batch in which every stripe has its own shard size and its own presence mask.
Every case is bit-exact against the C oracle (oracle.cref.encode / cref.reconstruct) stripe
by stripe: sizes on both sides of the vector and tile edges in an aligned and a packed
layout, nothing touched past a stripe's size, narrow / 8-row / 16-row / two-group profiles,
corruption flags that belong to their stripe, the all-sizes-equal case (exactly the mixed or
uniform plan), the API edges, a captured graph and a grid cut into slices."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A


@pytest.fixture(autouse=True)
def _no_tuned_forms(native_lib):
    """Forms compared below are the rule's: forget what other tests' tuners recorded."""
    native_lib.lib.rs_tune_table_reset(None)
    yield
    native_lib.lib.rs_tune_table_reset(None)


def _mask(n, lost):
    lost = set(lost)
    return [i not in lost for i in range(n)]


def _random_masks(n, batch, max_loss, seed, min_loss=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(batch):
        lost = rng.choice(n, size=int(rng.integers(min_loss, max_loss + 1)), replace=False)
        out.append(_mask(n, (int(i) for i in lost)))
    return out


def _stripes(k, m, sizes, seed):
    """Consistent stripes on the host: per stripe an [n][sizes[b]] array whose parity the
    oracle computed from random data."""
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


def _image(rb, stripes, fill=0):
    """The batch's whole allocation as a host array: `fill` everywhere, the stripes' shards
    at their offsets."""
    img = np.full(rb.nbytes, fill, dtype=np.uint8)
    for b, st in enumerate(stripes):
        for i in range(rb.n):
            o = rb.offsets[b][i]
            img[o:o + rb.sizes[b]] = st[i]
    return img


def _upload(rb, img):
    import torch
    rb.buf.copy_(torch.from_numpy(img))


def _consistent(k, m, sizes, seed, layout="aligned"):
    """A resident ragged batch of consistent stripes, the stripes and the allocation's image."""
    import torch
    from callfs_amd.device import RaggedBatch
    rb = RaggedBatch(k, m, sizes, torch.device("cuda:0"), layout=layout)
    stripes = _stripes(k, m, sizes, seed)
    img = _image(rb, stripes)
    _upload(rb, img)
    return rb, stripes, img


def _fill_missing(rb, masks, value=0):
    for b, mask in enumerate(masks):
        for i, p in enumerate(mask):
            if not p:
                rb.shard(b, i).fill_(value)


def _oracle(stripes, masks, k, m):
    """cref.reconstruct of every stripe from its present shards: per stripe [n][S]."""
    out = []
    for st, mask in zip(stripes, masks):
        full = cref.reconstruct([st[i] if p else None for i, p in enumerate(mask)], mask, k, m)
        out.append(np.stack([np.asarray(full[i]) for i in range(k + m)]))
    return out


def _check(k, m, sizes, masks, layout="aligned", seed=1):
    """One ragged launch over a consistent batch with each stripe's missing shards zeroed
    (masks None: an encode, the parity zeroed): every shard equals the oracle's, the rest of
    the allocation is untouched and nothing is flagged."""
    import torch
    from callfs_amd.device import Plan
    n, batch = k + m, len(sizes)
    rb, stripes, img = _consistent(k, m, sizes, seed, layout)
    eff = masks if masks is not None else [_mask(n, range(k, n))] * batch
    _fill_missing(rb, eff)
    plan = Plan.for_ragged(rb, present=masks)
    assert plan.S is None and plan.sizes == list(sizes)
    assert plan.forms() == ["ragged"] * ((m + 15) // 16)
    assert plan.bytes == n * sum(sizes)
    plan.launch()
    torch.cuda.synchronize()
    want = _oracle(stripes, eff, k, m)
    for b in range(batch):
        assert np.array_equal(want[b], stripes[b]), b
        got = rb.gather_stripe(b).cpu().numpy()
        for i in range(n):
            assert np.array_equal(got[i], want[b][i]), (b, i, sizes[b], eff[b])
    assert np.array_equal(rb.buf.cpu().numpy(), img)
    assert not plan.corrupt()
    plan.close()


SIZES = [1, 5, 15, 16, 17, 40, 8191, 8192, 8193, 8208, 2 * 8192 + 83, 3 * 8192, 7]


@pytest.mark.parametrize("layout", ["aligned", "packed"])
@pytest.mark.parametrize("mode", ["encode", "decode"])
def test_sizes_vs_oracle(native_lib, layout, mode):
    """The tail-only stripe, one vector, vector plus tail, the tile edge on both sides,
    several tiles and a tiny stripe after a long one, in one RS(10,4) batch."""
    masks = None if mode == "encode" else _random_masks(14, len(SIZES), 4, seed=0xB0B)
    if masks is not None:
        assert len({tuple(x) for x in masks}) > 4
    _check(10, 4, SIZES, masks, layout, seed=5)


@pytest.mark.parametrize("layout", ["packed", "aligned"])
def test_no_byte_past_a_stripes_size(native_lib, layout):
    """Everything is a sentinel but the present shards; the missing shards hold the sentinel
    too. After the launch the missing shards' [0, sizes[b]) are the oracle's bytes and every
    other byte (present shards, the padding between shards, a guard before and after the
    batch) is what it was. packed: adjacent shards touch, so one byte too many lands in a
    neighbour."""
    import torch
    from callfs_amd.device import Plan, RaggedBatch
    k, m, n = 10, 4, 14
    sizes = SIZES
    batch = len(sizes)
    masks = _random_masks(n, batch, 4, seed=0xC0DE)
    masks[-1] = _mask(n, (0, 12, 13))  # the batch's very last shard is written
    masks[0] = _mask(n, (0, 1))        # and its very first
    dev = torch.device("cuda:0")
    rb = RaggedBatch(k, m, sizes, dev, layout=layout)  # for the offsets
    stripes = _stripes(k, m, sizes, seed=8)
    want = _image(rb, stripes, fill=SENTINEL)
    start = want.copy()
    for b, mask in enumerate(masks):
        for i, p in enumerate(mask):
            if not p:
                o = rb.offsets[b][i]
                start[o:o + sizes[b]] = SENTINEL
    guard = 4096
    raw = torch.full((rb.nbytes + 2 * guard + 256,), SENTINEL, dtype=torch.uint8, device=dev)
    lead = guard + (-(raw.data_ptr() + guard) % 256)
    raw[lead:lead + rb.nbytes].copy_(torch.from_numpy(start))
    before = raw.cpu().numpy()
    base = raw.data_ptr() + lead
    ptrs = [base + o for row in rb.offsets for o in row]
    plan = Plan.ragged(k, m, sizes, ptrs, present=masks)
    assert plan.forms() == ["ragged"]
    plan.launch()
    torch.cuda.synchronize()
    assert not plan.corrupt()
    after = raw.cpu().numpy()
    assert np.array_equal(after[:lead], before[:lead]), "bytes before the batch changed"
    assert np.array_equal(after[lead + rb.nbytes:], before[lead + rb.nbytes:]), "bytes after the batch changed"
    body = after[lead:lead + rb.nbytes]
    bad = np.flatnonzero(body != want)
    assert bad.size == 0, (layout, bad[:8].tolist())
    plan.close()


@pytest.mark.parametrize("k,m", [(1, 3), (3, 2), (16, 4), (10, 8), (20, 12), (10, 20)])
def test_profiles_vs_oracle(native_lib, k, m):
    """4 / 8 / 16-row instances (8- and 16-byte entries) and two launch groups (m = 20),
    mixed 1..m losses; one stripe loses its first m shards."""
    sizes = [8193, 16, 3, 2 * 8192 + 5, 8192]
    masks = _random_masks(k + m, len(sizes), m, seed=100 * k + m)
    masks[0] = _mask(k + m, range(m))
    assert len({tuple(x) for x in masks}) > 1
    _check(k, m, sizes, masks, seed=k + m)


def test_flags_belong_to_their_stripe(native_lib):
    import torch
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [3 * 8192 + 37, 9, 8192 + 16 * 7 + 5, 20000, 12, 2 * 8192 + 3]
    batch = len(sizes)
    masks = [_mask(n, range(b, b + b % 4)) for b in range(batch)]
    assert [mk.count(False) for mk in masks] == [0, 1, 2, 3, 0, 1]
    rb, stripes, img = _consistent(k, m, sizes, seed=9)
    _fill_missing(rb, masks)
    plan = Plan.for_ragged(rb, present=masks)
    assert plan.forms() == ["ragged"]

    def run():
        plan.launch()
        torch.cuda.synchronize()
        return plan.corrupt_stripes()

    def flip(b, i, off):
        rb.shard(b, i)[off] ^= 0x40

    assert run() == []
    assert np.array_equal(rb.buf.cpu().numpy(), img)
    cases = set()
    for b, mask in enumerate(masks):
        S = sizes[b]
        present = [i for i in range(n) if mask[i]]
        compared, inputs = present[k:], present[:k]
        assert compared, b  # at most 3 losses: every stripe has a compared row
        offs = []
        nvec = S // 16
        if nvec > 2 * 512:  # a vector of a middle tile
            offs.append(("middle", 8192 + 16 * 100 + 3))
        if nvec:
            offs.append(("vector", 16 * (nvec - 1) + 1))
        if S % 16:
            offs.append(("tiny" if S < 16 else "tail", S - 1))
        for what, off in offs:
            cases.add(what)
            flip(b, compared[-1], off)
            assert run() == [b], (b, what, off)
            flip(b, compared[-1], off)
        # a flipped input: the stripe's compared rows no longer match what it computes
        flip(b, inputs[b % k], S // 2)
        assert run() == [b], b
        flip(b, inputs[b % k], S // 2)
        _fill_missing(rb, masks)  # (the flipped input left junk in the recomputed shards)
    assert cases == {"middle", "vector", "tail", "tiny"}
    assert run() == []
    # junk in a missing shard is overwritten, never compared
    _fill_missing(rb, masks, 0xA5)
    assert run() == []
    assert np.array_equal(rb.buf.cpu().numpy(), img)
    # status clears the flags
    flip(1, 13, 4)
    plan.launch()
    torch.cuda.synchronize()
    assert plan.corrupt()
    assert plan.corrupt_stripes() == []
    flip(1, 13, 4)
    assert run() == []
    plan.close()


def test_equal_sizes_collapse(native_lib):
    import torch
    from callfs_amd.device import Plan
    k, m, n, batch = 10, 4, 14, 4
    S = 2 * 8192 + 16 * 5 + 3
    rb, stripes, img = _consistent(k, m, [S] * batch, seed=21)
    ptrs = rb.pointers()
    # masks differ: the mixed plan
    masks = [_mask(n, (0,)), _mask(n, (1, 12)), _mask(n, ()), _mask(n, (2, 3, 4, 5))]
    ragged = Plan.for_ragged(rb, present=masks)
    mixed = Plan(k, m, S, batch, ptrs, present=masks)
    assert ragged.forms() == mixed.forms() == ["mixed"]
    assert ragged.bytes == mixed.bytes
    outs = []
    for plan in (mixed, ragged):
        _fill_missing(rb, masks)
        plan.launch()
        torch.cuda.synchronize()
        assert not plan.corrupt()
        outs.append(rb.buf.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], img)
    # masks equal too: the uniform plan, as an encode (no masks) and as a decode
    mask = _mask(n, (0, 3, 7, 12))
    for pres_r, pres_u in ((None, None), ([mask] * batch, mask)):
        r = Plan.for_ragged(rb, present=pres_r)
        u = Plan(k, m, S, batch, ptrs, present=pres_u)
        assert r.forms() == u.forms()
        assert "ragged" not in r.forms()[0] and "mixed" not in r.forms()[0]
        assert r.bytes == u.bytes
        _fill_missing(rb, [mask if pres_u else _mask(n, range(k, n))] * batch)
        r.launch()
        torch.cuda.synchronize()
        assert not r.corrupt()
        assert np.array_equal(rb.buf.cpu().numpy(), img)
        r.close()
        u.close()
    ragged.close()
    mixed.close()


def test_api_edges(native_lib):
    import torch
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [8192 + 16 * 3 + 5, 11, 4000, 16]
    batch = len(sizes)
    masks = [_mask(n, (0,)), _mask(n, (1, 12)), _mask(n, ()), _mask(n, (2, 3, 4, 5))]
    rb, stripes, img = _consistent(k, m, sizes, seed=33)
    ptrs = rb.pointers()
    ctx = N.default_context()
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    szs = (ctypes.c_size_t * batch)(*sizes)
    pres = (ctypes.c_uint8 * (batch * n))(*[1 if p else 0 for mk in masks for p in mk])
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def code(fn, *a, **kw):
        with pytest.raises(N.NativeError) as ei:
            fn(*a, **kw)
        return ei.value.code

    # a zero size anywhere: nothing is created, even when all sizes are equal
    assert code(Plan.ragged, k, m, [sizes[0], 0, 4000, 16], ptrs, present=masks) == N.RS_E_NO_DATA
    assert code(Plan.ragged, k, m, [0] * batch, ptrs) == N.RS_E_NO_DATA
    # a stripe with k - 1 present shards, in a ragged batch and in an equal-size one
    short = [list(x) for x in masks]
    short[2] = _mask(n, (0, 1, 2, 3, 4))
    assert code(Plan.ragged, k, m, sizes, ptrs, present=short) == N.RS_E_TOO_FEW_SHARDS
    assert code(Plan.ragged, k, m, [16] * batch, ptrs, present=short) == N.RS_E_TOO_FEW_SHARDS
    # no stripes, and NULL sizes / shards / out
    assert code(Plan.ragged, k, m, [], []) == N.RS_E_ARG
    h = ctypes.c_void_p()
    L = N.lib
    assert L.rs_plan_create_ragged(ctx.handle, 0, k, m, 0, szs, pres, arr, ctypes.byref(h)) == N.RS_E_ARG
    assert L.rs_plan_create_ragged(ctx.handle, 0, k, m, batch, None, pres, arr, ctypes.byref(h)) == N.RS_E_ARG
    assert L.rs_plan_create_ragged(ctx.handle, 0, k, m, batch, szs, pres, None, ctypes.byref(h)) == N.RS_E_ARG
    assert L.rs_plan_create_ragged(ctx.handle, 0, k, m, batch, szs, pres, arr, None) == N.RS_E_ARG
    # profile errors are rs_plan_create_mixed's
    for bk, bm in ((0, 4), (10, 0), (200, 100)):
        want = L.rs_plan_create_mixed(ctx.handle, 0, bk, bm, 16, batch, pres, arr, ctypes.byref(h))
        assert want != 0
        assert L.rs_plan_create_ragged(ctx.handle, 0, bk, bm, batch, szs, pres, arr, ctypes.byref(h)) == want
        assert L.rs_decode_dev_ragged(ctx.handle, 0, bk, bm, batch, szs, pres, arr, s) == want
    # wrong shapes
    with pytest.raises(ValueError):
        Plan.ragged(k, m, sizes, ptrs[:-1])
    with pytest.raises(ValueError):
        Plan.ragged(k, m, sizes, ptrs, present=masks[:3])
    with pytest.raises(ValueError):
        Plan.ragged(k, m, sizes, ptrs, present=masks[0])

    plan = Plan.for_ragged(rb, present=np.array(masks, dtype=bool))
    groups = int(L.rs_plan_groups(plan.handle))
    assert groups == 1 and plan.forms() == ["ragged"]
    assert plan.bytes == n * sum(sizes)
    assert plan.tune() == ["none"] * groups
    assert L.rs_tune_table_entries() == 0
    assert code(plan.set_orders, ["g8"] * groups) == N.RS_E_ARG
    assert code(plan.set_orders, ["consecutive"] * groups) == N.RS_E_ARG
    assert code(plan.set_orders, ["none"] * (groups + 1)) == N.RS_E_ARG
    plan.set_orders(["none"] * groups)
    assert L.rs_plan_launch_ceiling(plan.handle, s, 1) == N.RS_E_ARG
    assert L.rs_plan_launch_ceiling_timed(plan.handle, s, 2, None, None) == N.RS_E_ARG
    _fill_missing(rb, masks)
    plan.launch()
    torch.cuda.synchronize()
    assert not plan.corrupt()
    assert np.array_equal(rb.buf.cpu().numpy(), img)
    # timed launches bracket the kernels
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    plan.launch(events=(e0, e1))
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) > 0
    plan.close()

    # the one-shot call: RS_E_CORRUPT exactly when a compared byte was flipped
    def one_shot(p=pres, eff=masks):
        _fill_missing(rb, eff)
        torch.cuda.synchronize()
        return L.rs_decode_dev_ragged(ctx.handle, 0, k, m, batch, szs, p, arr, s)

    assert one_shot() == 0
    assert np.array_equal(rb.buf.cpu().numpy(), img)
    # (a compared shard of the sub-16-byte stripe, one in a tail, an input of a full stripe)
    for b, i, off in ((1, 13, 10), (0, 13, sizes[0] - 2), (2, 0, 5)):
        assert masks[b][i]
        rb.shard(b, i)[off] ^= 1
        assert one_shot() == N.RS_E_CORRUPT, (b, i, off)
        rb.shard(b, i)[off] ^= 1
        assert one_shot() == 0
    assert np.array_equal(rb.buf.cpu().numpy(), img)
    # no masks: an encode of every stripe
    assert one_shot(None, [_mask(n, range(k, n))] * batch) == 0
    assert np.array_equal(rb.buf.cpu().numpy(), img)


def test_graph_capture(native_lib):
    import torch
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [65_541, 9, 8192, 3 * 8192 + 17, 100, 40_000]
    masks = _random_masks(n, len(sizes), 4, seed=77)
    rb, stripes, img = _consistent(k, m, sizes, seed=41)
    plan = Plan.for_ragged(rb, present=masks)
    assert plan.forms() == ["ragged"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        plan.launch(s)
    torch.cuda.synchronize()
    assert not plan.corrupt(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch(s)
    want = _oracle(stripes, masks, k, m)
    for _ in range(2):
        _fill_missing(rb, masks)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert not plan.corrupt(s)
        for b in range(len(sizes)):
            assert np.array_equal(rb.gather_stripe(b).cpu().numpy(), want[b]), b
        assert np.array_equal(rb.buf.cpu().numpy(), img)
    plan.close()


_SLICED_CHILD = r"""
import sys
import numpy as np
import torch
from oracle import cref
from callfs_amd.device import Plan, RaggedBatch

k, m, n = 2, 1, 3
sizes = [53 * 8192 + b % 17 for b in range(40)] + [8192, 5, 8193, 16]
rb = RaggedBatch(k, m, sizes, torch.device("cuda:0"))
assert sum(max(1, -(-(S // 16) // 512)) for S in sizes) > 2048
rb.fill_random(11)
host = rb.buf.cpu().numpy()

def stripe(img, b):
    return [img[o:o + sizes[b]] for o in rb.offsets[b]]

def compare(want_of):
    torch.cuda.synchronize()
    got = rb.buf.cpu().numpy()
    bad = 0
    for b in range(len(sizes)):
        want = want_of(b)
        for i, sh in enumerate(stripe(got, b)):
            if not np.array_equal(sh, want[i]):
                print("mismatch: stripe", b, "shard", i, "size", sizes[b])
                bad += 1
    return bad

bad = 0
# encode: parity from the data shards
enc = Plan.for_ragged(rb)
assert enc.forms() == ["ragged"], enc.forms()
enc.launch()
parity = [cref.encode(stripe(host, b)[:k], k, m) for b in range(len(sizes))]
bad += compare(lambda b: stripe(host, b)[:k] + [parity[b][0]])
bad += int(enc.corrupt())
enc.close()
full = rb.buf.cpu().numpy()
# decode: every stripe loses one shard, which one differs from stripe to stripe
masks = [[i != b % n for i in range(n)] for b in range(len(sizes))]
for b, mk in enumerate(masks):
    rb.shard(b, b % n).zero_()
dec = Plan.for_ragged(rb, present=masks)
assert dec.forms() == ["ragged"], dec.forms()
dec.launch()
torch.cuda.synchronize()
img = rb.buf.cpu().numpy()
def rebuilt(b):
    sh = stripe(full, b)
    return cref.reconstruct([sh[i] if masks[b][i] else None for i in range(n)], masks[b], k, m)
bad += compare(rebuilt)
bad += int(dec.corrupt())
dec.close()
print("sliced ragged child:", "ok" if not bad else "%d mismatches" % bad)
sys.exit(1 if bad else 0)
"""


def test_sliced_grid(native_lib):
    """CALLFS_RS_MAX_TILES_PER_LAUNCH is read once per process: a fresh child runs an RS(2,1)
    batch of more than 2,048 tiles in slices of at most 1,024, with slice boundaries inside
    stripes, as an encode and a decode, bit-exact against the oracle."""
    env = dict(os.environ)
    env["CALLFS_RS_MAX_TILES_PER_LAUNCH"] = "1024"
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _SLICED_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sliced ragged child: ok" in r.stdout
