"""Mixed device plans (rs_plan_create_mixed): one launch reconstructs and
verifies a batch in which every stripe has its own presence mask. Every case is bit-exact
against the C oracle (oracle.cref.encode / cref.reconstruct) stripe by stripe: the erasure
patterns of RS(10,4) in every layout, narrow / 8-row / 16-row / two-group profiles, the
byte kernel and the tile edges, corruption flags that belong to their stripe, the
all-masks-equal case (exactly the uniform plan), the API edges and a captured graph."""
import ctypes

import numpy as np
import pytest

from oracle import cref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_tuned_forms(native_lib):
    """Forms compared below are the rule's: forget what other tests' tuners recorded."""
    native_lib.lib.rs_tune_table_reset(None)
    yield
    native_lib.lib.rs_tune_table_reset(None)


def _consistent(k, m, S, batch, seed, layout="planar"):
    """A resident batch whose parity the oracle computed (so every stripe is consistent),
    and its host copy [batch][n][S]."""
    import torch
    from callfs_amd.device import StripeBatch
    sb = StripeBatch(k, m, S, batch, torch.device("cuda:0"), layout=layout)
    sb.fill_random(seed)
    host = sb.gather().cpu().numpy()
    for b in range(batch):
        want = cref.encode([host[b, i] for i in range(k)], k, m)
        for j in range(m):
            host[b, k + j] = want[j]
            sb.shard(b, k + j).copy_(torch.from_numpy(want[j]))
    return sb, host


def _mask(n, lost):
    return [i not in lost for i in range(n)]


def _random_masks(n, batch, max_loss, seed, min_loss=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(batch):
        lost = rng.choice(n, size=int(rng.integers(min_loss, max_loss + 1)), replace=False)
        out.append(_mask(n, set(int(i) for i in lost)))
    return out


def _zero_missing(sb, masks):
    for b, mask in enumerate(masks):
        for i, p in enumerate(mask):
            if not p:
                sb.shard(b, i).zero_()


def _oracle(host, masks, k, m):
    """cref.reconstruct of every stripe from its present shards: [batch][n][S]."""
    want = np.empty_like(host)
    for b, mask in enumerate(masks):
        full = cref.reconstruct([host[b, i] if p else None for i, p in enumerate(mask)], mask, k, m)
        for i in range(k + m):
            want[b, i] = full[i]
    return want


def _check(k, m, S, masks, layout="planar", seed=1):
    """One mixed launch over a consistent batch with each stripe's missing shards zeroed:
    every shard equals the oracle's reconstruction (and the original), nothing is flagged."""
    import torch
    from callfs_amd.device import Plan
    batch = len(masks)
    sb, host = _consistent(k, m, S, batch, seed, layout)
    _zero_missing(sb, masks)
    plan = Plan.for_batch(sb, present=masks)
    assert plan.forms() == ["mixed"] * ((m + 15) // 16)
    assert plan.bytes == batch * (k + m) * S
    plan.launch()
    torch.cuda.synchronize()
    got = sb.gather().cpu().numpy()
    want = _oracle(host, masks, k, m)
    assert np.array_equal(want, host)
    for b in range(batch):
        for i in range(k + m):
            assert np.array_equal(got[b, i], want[b, i]), (b, i, masks[b])
    assert not plan.corrupt()
    plan.close()


@pytest.mark.parametrize("layout", ["pitch", "planar", "split", "readall"])
def test_patterns_vs_oracle(native_lib, layout):
    k, m, n = 10, 4, 14
    S = 2 * 8192 + 16 * 5 + 3  # two full tiles, a partial wave, a 3-byte tail
    masks = [_mask(n, ()), _mask(n, (0,)), _mask(n, (9,)), _mask(n, (10,)), _mask(n, (13,)),
             _mask(n, (0, 1, 2, 3)), _mask(n, (0, 3, 7, 12)), _mask(n, (10, 11, 12, 13))]
    masks += _random_masks(n, 4, 4, seed=0xA11)
    assert len(masks) == 12
    _check(k, m, S, masks, layout, seed=3)


@pytest.mark.parametrize("k,m", [(1, 3), (3, 2), (4, 2), (16, 4), (10, 8), (20, 12), (10, 20)])
def test_profiles_vs_oracle(native_lib, k, m):
    """v_perm-sized profiles (k <= 3), 4 / 8 / 16-row instances (8- and 16-byte entries) and
    two launch groups (m = 20), mixed 1..m losses."""
    S = 2 * 8192 + 16 * 5 + 3
    masks = _random_masks(k + m, 6, m, seed=100 * k + m)
    masks[0] = _mask(k + m, range(m))  # m losses, data shards first
    assert len({tuple(x) for x in masks}) > 1
    _check(k, m, S, masks, seed=k + m)


@pytest.mark.parametrize("S", [1, 5, 15, 16, 17, 8192, 8193])
def test_sizes_vs_oracle(native_lib, S):
    """The byte kernel (S < 16), one vector, a vector plus tail, the tile edge."""
    masks = _random_masks(14, 5, 4, seed=S)
    masks[4] = _mask(14, ())
    _check(10, 4, S, masks, seed=S)


def test_flags_belong_to_their_stripe(native_lib):
    import torch
    from callfs_amd.device import Plan
    k, m, n, batch = 10, 4, 14, 6
    S = 65_536 + 45
    masks = [_mask(n, range(b, b + b % 4)) for b in range(batch)]
    assert [mk.count(False) for mk in masks] == [0, 1, 2, 3, 0, 1]
    sb, host = _consistent(k, m, S, batch, seed=9)
    _zero_missing(sb, masks)
    plan = Plan.for_batch(sb, present=masks)

    def run():
        plan.launch()
        torch.cuda.synchronize()
        return plan.corrupt_stripes()

    def flip(b, i, off):
        sb.shard(b, i)[off] ^= 0x40

    assert run() == []
    assert np.array_equal(sb.gather().cpu().numpy(), host)
    for b, mask in enumerate(masks):
        present = [i for i in range(n) if mask[i]]
        compared, inputs = present[k:], present[:k]
        assert compared, b  # at most 3 losses: every stripe has a compared row
        for off in (100, S - 3):  # a vector of the first tile; the S % 16 tail
            flip(b, compared[-1], off)
            assert run() == [b], (b, off)
            flip(b, compared[-1], off)
        # a flipped input: the stripe's compared rows no longer match what it computes
        flip(b, inputs[b % k], 4096 + b)
        assert run() == [b], b
        flip(b, inputs[b % k], 4096 + b)
        _zero_missing(sb, masks)  # (the flipped input left junk in the recomputed shards)
    assert run() == []
    # junk in a missing shard is overwritten, never compared
    for b, mask in enumerate(masks):
        for i in range(n):
            if not mask[i]:
                sb.shard(b, i).fill_(0xA5)
    assert run() == []
    got = sb.gather().cpu().numpy()
    want = _oracle(host, masks, k, m)
    assert np.array_equal(got, want)
    # stripes 0 and 4 lose nothing: all m rows are compared, a flip in any shard flags them
    for b in (0, 4):
        for i in (0, 9, 10, 13):
            flip(b, i, 7 * i + 1)
            assert run() == [b], (b, i)
            flip(b, i, 7 * i + 1)
    assert run() == []
    plan.close()


def test_all_masks_equal_is_the_uniform_plan(native_lib):
    import torch
    from callfs_amd.device import Plan
    k, m, n, batch = 10, 4, 14, 4
    S = 2 * 8192 + 16 * 5 + 3
    mask = _mask(n, (0, 3, 7, 12))
    sb, host = _consistent(k, m, S, batch, seed=21)
    uniform = Plan.for_batch(sb, present=mask)
    same = Plan.for_batch(sb, present=[list(mask) for _ in range(batch)])
    same_np = Plan.for_batch(sb, present=np.array([mask] * batch, dtype=np.uint8))
    assert same.forms() == uniform.forms() == same_np.forms()
    assert "mixed" not in same.forms()[0]
    assert same.bytes == uniform.bytes
    outs = []
    for plan in (uniform, same):
        _zero_missing(sb, [mask] * batch)
        plan.launch()
        torch.cuda.synchronize()
        assert not plan.corrupt()
        outs.append(sb.gather().cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], host)
    for plan in (uniform, same, same_np):
        plan.close()


def test_api_edges(native_lib):
    import torch
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    k, m, n, batch = 10, 4, 14, 4
    S = 8192 + 16 * 3 + 5
    masks = [_mask(n, (0,)), _mask(n, (1, 12)), _mask(n, ()), _mask(n, (2, 3, 4, 5))]
    sb, host = _consistent(k, m, S, batch, seed=33)
    # a stripe with k - 1 present shards: nothing is created
    short = [list(x) for x in masks]
    short[2] = _mask(n, (0, 1, 2, 3, 4))
    with pytest.raises(N.NativeError) as ei:
        Plan.for_batch(sb, present=short)
    assert ei.value.code == N.RS_E_TOO_FEW_SHARDS
    # ... even when every stripe has that same mask
    with pytest.raises(N.NativeError) as ei:
        Plan.for_batch(sb, present=[short[2]] * batch)
    assert ei.value.code == N.RS_E_TOO_FEW_SHARDS
    # wrong shapes
    with pytest.raises(ValueError):
        Plan.for_batch(sb, present=masks[:3])
    with pytest.raises(ValueError):
        Plan.for_batch(sb, present=[x[:-1] for x in masks])
    with pytest.raises(ValueError):
        Plan.for_batch(sb, present=np.ones((batch, n + 1), dtype=np.uint8))
    with pytest.raises(ValueError):
        Plan.for_batch(sb, present=np.ones((2, batch, n), dtype=np.uint8))

    plan = Plan.for_batch(sb, present=np.array(masks, dtype=bool))
    groups = int(N.lib.rs_plan_groups(plan.handle))
    assert groups == 1 and plan.forms() == ["mixed"]
    assert plan.tune() == ["none"] * groups
    with pytest.raises(N.NativeError) as ei:
        plan.set_orders(["g8"] * groups)
    assert ei.value.code == N.RS_E_ARG
    plan.set_orders(["none"] * groups)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert N.lib.rs_plan_launch_ceiling(plan.handle, s, 1) == N.RS_E_ARG
    assert N.lib.rs_plan_launch_ceiling_timed(plan.handle, s, 2, None, None) == N.RS_E_ARG
    _zero_missing(sb, masks)
    plan.launch()
    torch.cuda.synchronize()
    assert not plan.corrupt()
    assert np.array_equal(sb.gather().cpu().numpy(), host)
    # timed launches bracket the kernels
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    plan.launch(events=(e0, e1))
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) > 0
    plan.close()

    # the one-shot call: RS_E_CORRUPT exactly when a compared row was flipped
    ptrs = sb.pointers()
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    pres = (ctypes.c_uint8 * (batch * n))(*[1 if p else 0 for mk in masks for p in mk])
    ctx = N.default_context()

    def one_shot():
        _zero_missing(sb, masks)
        torch.cuda.synchronize()
        return N.lib.rs_decode_dev_mixed(ctx.handle, 0, k, m, S, batch, pres, arr, s)

    assert one_shot() == 0
    assert np.array_equal(sb.gather().cpu().numpy(), host)
    sb.shard(1, 13)[S - 2] ^= 1  # stripe 1 lost {1, 12}: parity 13 is compared
    assert one_shot() == N.RS_E_CORRUPT
    sb.shard(1, 13)[S - 2] ^= 1
    assert one_shot() == 0
    assert N.lib.rs_decode_dev_mixed(ctx.handle, 0, k, m, S, batch, None, arr, s) == N.RS_E_ARG


def test_graph_capture(native_lib):
    import torch
    from callfs_amd.device import Plan
    k, m, n, batch = 10, 4, 14, 6
    S = 65_541
    masks = _random_masks(n, batch, 4, seed=77)
    sb, host = _consistent(k, m, S, batch, seed=41)
    plan = Plan.for_batch(sb, present=masks)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        plan.launch(s)
    torch.cuda.synchronize()
    assert not plan.corrupt(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch(s)
    want = _oracle(host, masks, k, m)
    for _ in range(2):
        _zero_missing(sb, masks)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert not plan.corrupt(s)
        assert np.array_equal(sb.gather().cpu().numpy(), want)
    plan.close()
