"""Verify's corruption flags at every compared row, every edge of a shard and every kernel form.

Every kernel here compares as well as computes: Verify rows are recomputed in
registers and compared with the stored shard, and a mismatch sets the stripe's status word. A
kernel that skips a compared row, a lane, a boundary vector or a tail byte still writes every
output byte correctly, so no byte comparison sees it; the only symptom is a flag that stays 0
on a corrupt shard. The opposite error is a flag raised by bytes that belong to no shard
(pitch padding, the bytes around a misaligned shard, the garbage in a missing shard's buffer).

The sweep: one consistent stripe per shard size (seeded data, parity by the C oracle) is
replicated on the device into a batch inside one allocation in which everything that is not a
shard holds a sentinel, a guard region before and after included. A probe is one flipped bit
(shard, byte position, XOR value 1 << position % 8) in a stripe of its own; every fourth stripe
carries none. All flips of a launch are one indexed XOR on the device, undone the same way.
For every probe the verdict comes from the oracle (`cref.verify`, after `cref.reconstruct` for a
decode, as Codec.Decode does) before the launch, and `corrupt_stripes()` must equal exactly the
set the oracle calls corrupt. After the last launch of a case a clean launch flags nothing and
every byte of the allocation, sentinels included, equals the expected image. `plan.forms()`
must report the form under test at every launch.

  python tests/test_gpu_verify_sweep.py child GROUP     # what the child processes run
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import cref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 8192          # sentinel bytes before and after the batch (at least 4 KiB)
REGION_ALIGN = 8192   # the batch starts on this boundary, so a layout's base offset is the misalignment
DEVICE = "cuda:0"
WINDOW = 64           # columns of a stripe the oracle is asked about, see Sweep.oracle_corrupt

# The v_perm kernel's tile, mirroring rs_kernels.hip ProdOrderPolicy = Policy<WPE 4, U 1, ...,
# BS 512>: a block of BS lanes takes U vectors per lane, BS * 16 bytes apart. With U = 1 a lane
# has one vector, so the class "between a lane's U vectors" does not exist for this kernel and
# both constants below equal the plain 8,192-byte tile: they add no position while U stays 1.
VPERM_BS, VPERM_U = 512, 1
BOUNDARIES = sorted({
    16 * 62, 16 * 63,            # the realigning forms' 62 and 63 vectors per wave
    1024,                        # a wave's window; the bit-sliced lane's second vector
    2048,                        # the bit-sliced wave window
    8 * 16 * 62, 8 * 16 * 63,    # the realigning forms' tiles
    8192, 16384,                 # tiles
    VPERM_BS * VPERM_U * 16,     # the v_perm kernel's tile
    VPERM_BS * 16,               # between a v_perm lane's U vectors
})

S_TILES = 17_399        # two full tiles, 63 vectors, a 7-byte tail
S_IDLE = 16 * 62 + 3    # one partial tile: the tail goes to the idle last wave
S_NOTAIL = 16 * 64      # no tail
VECTOR_SIZES = [S_TILES, S_IDLE, S_NOTAIL]
BYTE_SIZES = [1, 9, 15]  # the byte kernels: every position probed

ALL_ORDER_NAMES = ["consecutive", "g8", "g2", "q8", "q16", "x8", "x32", "realign",
                   "realign-x8", "realign-x32", "wix", "wix-g8", "wix-g2", "wix-q8", "wix-q16",
                   "wix-x8", "wix-x32", "tri", "tri-g2", "tri-x32", "tri-q8", "tri-q16",
                   "tri-x8", "realign-tri", "realign-tri-x8", "realign-tri-x32",
                   "realign64", "realign64-x8", "realign64-x32",
                   "dma", "dma-g2", "dma-q8", "dma-x32", "tridb-g4", "tridb-g8",
                   "bs", "bs-g8", "bs-g2", "bs-q8", "bs-q16", "bs-x8", "bs-x32"]


def positions(S, seed=0x5EED):
    """The byte positions probed in a shard of S bytes: the first and the last 64 (every head
    misalignment, every residue of S % 16, the last full vector), both sides of every wave and
    tile boundary below S, and 32 seeded ones."""
    pos = set(range(min(64, S))) | set(range(max(0, S - 64), S))
    for b in BOUNDARIES:
        if b < S:
            pos |= {b - 1, b}
    rng = np.random.default_rng(seed + S)
    pos |= {int(x) for x in rng.integers(0, S, 32)}
    return sorted(pos)


def xor_of(pos):
    return 1 << (pos % 8)


def stripes_for(nprobes):
    """Batch size for `nprobes` probes, one stripe each: every fourth stripe stays clean, so a
    quarter of the batch is clean and every run of 8 neighbours holds both kinds."""
    return 4 * ((nprobes + 2) // 3)


def probed_stripes(batch):
    return [b for b in range(batch) if b % 4 != 3]


def roles(mask, k):
    """(inputs, compared, missing) of a presence mask: the first k present shards are read, the
    other present ones are compared."""
    present = [i for i, p in enumerate(mask) if p]
    return present[:k], present[k:], [i for i, p in enumerate(mask) if not p]


# ---- layouts: (offs[batch][n] of every shard from the start of the batch, bytes) --------------

def _up(x, a):
    return -(-x // a) * a


def lay_pitch(k, m, sizes):
    n, S = k + m, sizes[0]
    pitch = _up(S, 256)
    offs = np.array([[(b * n + i) * pitch for i in range(n)] for b in range(len(sizes))], np.int64)
    return offs, len(sizes) * n * pitch


def lay_planar(k, m, sizes):
    S, B = sizes[0], len(sizes)
    pitch = _up(S, 256)
    offs = np.array([[(b * k + i) * pitch if i < k else (B * k + b * m + i - k) * pitch
                      for i in range(k + m)] for b in range(B)], np.int64)
    return offs, B * (k + m) * pitch


def lay_split(base):
    """Upstream Split's layout of contiguous objects: shard after shard, the first at `base`."""
    def lay(k, m, sizes):
        n, S = k + m, sizes[0]
        offs = np.array([[base + (b * n + i) * S for i in range(n)] for b in range(len(sizes))],
                        np.int64)
        return offs, base + len(sizes) * n * S + 16
    return lay


def lay_readall(missing):
    """io.ReadAll bodies: data shards back to back in 8 KiB-aligned bodies, parity 64-B aligned at
    a 64-B pitch; the lost shards are rebuilt into fresh 64-B aligned buffers of their own, and
    the places they had in the body are no shards."""
    def lay(k, m, sizes):
        S, B = sizes[0], len(sizes)
        body, pp = _up(k * S, 8192), _up(S, 64)
        par0 = B * body
        fresh0 = _up(par0 + B * m * pp, 256)
        offs = np.zeros((B, k + m), np.int64)
        for b in range(B):
            for i in range(k + m):
                offs[b, i] = b * body + i * S if i < k else par0 + (b * m + i - k) * pp
            for j, i in enumerate(missing):
                offs[b, i] = fresh0 + (b * len(missing) + j) * pp
        return offs, fresh0 + B * len(missing) * pp
    return lay


def lay_ragged(packed):
    def lay(k, m, sizes):
        offs, off = np.zeros((len(sizes), k + m), np.int64), (3 if packed else 0)
        for b, S in enumerate(sizes):
            for i in range(k + m):
                if not packed:
                    off = _up(off, 256)
                offs[b, i] = off
                off += S
        return offs, off + 16
    return lay


# ---- the harness ------------------------------------------------------------------------------

class Sweep:
    """One batch in one guarded allocation, its expected image, its plan and the oracle's
    verdicts. masks[b] is stripe b's presence mask (every stripe has one: nothing lost is a
    read-only Verify)."""

    def __init__(self, k, m, sizes, masks, layout, kind="uniform", seed=7):
        import torch
        from callfs_amd.device import Plan
        self.torch = torch
        self.k, self.m, self.n = k, m, k + m
        self.sizes = [int(s) for s in sizes]
        self.batch = len(self.sizes)
        self.masks = [tuple(bool(p) for p in mk) for mk in masks]
        assert len(self.masks) == self.batch
        self.roles = [roles(mk, k) for mk in self.masks]
        self.offs, region = layout(k, m, self.sizes)
        dev = torch.device(DEVICE)
        self.raw = torch.full((region + 2 * GUARD + REGION_ALIGN,), SENTINEL, dtype=torch.uint8,
                              device=dev)
        self.lead = GUARD + (-(self.raw.data_ptr() + GUARD) % REGION_ALIGN)
        self.region = region
        # no two shards overlap, none leaves the region
        spans = sorted((int(self.offs[b, i]), int(self.offs[b, i]) + self.sizes[b])
                       for b in range(self.batch) for i in range(self.n))
        assert spans[0][0] >= 0 and spans[-1][1] <= region
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
        self.first, self.last = spans[0][0], spans[-1][1]
        starts = np.array([s for s, _ in spans] + [region], np.int64)
        self._starts = starts
        # one consistent stripe per distinct size
        self.proto = {}
        for S in sorted(set(self.sizes)):
            rng = np.random.default_rng(seed * 1_000_003 + S)
            st = np.empty((self.n, S), np.uint8)
            st[:k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
            for j, p in enumerate(cref.encode([st[i] for i in range(k)], k, m)):
                st[k + j] = p
            assert cref.verify(list(st), k, m)
            self.proto[S] = st
        # the expected image, replicated on the device; missing shards start as garbage
        self.want = torch.full_like(self.raw, SENTINEL)
        by_size = {}
        for b, S in enumerate(self.sizes):
            by_size.setdefault(S, []).append(b)
        miss = []
        for S, bs in by_size.items():
            col = torch.arange(S, device=dev)
            src = torch.from_numpy(self.proto[S]).to(dev)
            o = torch.from_numpy(self.offs[bs] + self.lead).to(dev)
            lost = torch.tensor([[not self.masks[b][i] for i in range(self.n)] for b in bs],
                                device=dev)
            for i in range(self.n):
                idx = o[:, i, None] + col[None, :]
                self.want[idx] = src[i][None, :].expand(len(bs), S)
                if bool(lost[:, i].any()):
                    miss.append(idx[lost[:, i]].reshape(-1))
        self.miss = torch.cat(miss) if miss else None
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        self.garbage = (torch.randint(0, 256, (self.miss.numel(),), dtype=torch.uint8, device=dev,
                                      generator=g) if miss else None)
        base = self.raw.data_ptr() + self.lead
        ptrs = [base + int(o) for o in self.offs.reshape(-1)]
        rows = [list(mk) for mk in self.masks]
        if kind == "uniform":
            assert len(set(self.masks)) == 1 and len(by_size) == 1
            self.plan = Plan(k, m, self.sizes[0], self.batch, ptrs, present=rows[0])
        elif kind == "mixed":
            assert len(by_size) == 1
            self.plan = Plan(k, m, self.sizes[0], self.batch, ptrs, present=rows)
        else:
            self.plan = Plan.ragged(k, m, self.sizes, ptrs, present=rows)
        self.groups = len(self.plan.forms())
        self.forms = None
        self.verdicts, self.whole = {}, set()
        self.launches = 0
        self.reset()

    def reset(self):
        """The consistent batch, garbage in every missing shard's buffer."""
        self.raw.copy_(self.want)
        if self.miss is not None:
            self.raw[self.miss] = self.garbage

    # -- probes: (stripe, shard or None, position, XOR value, index in raw) ------------------
    def probe(self, b, i, pos):
        assert 0 <= pos < self.sizes[b] and self.masks[b][i]
        return (b, i, pos, xor_of(pos), self.lead + int(self.offs[b, i]) + pos)

    def gap(self, b, i):
        """Bytes after shard i of stripe b that belong to no shard."""
        end = int(self.offs[b, i]) + self.sizes[b]
        nxt = int(self._starts[np.searchsorted(self._starts, end, side="left")])
        return nxt - end

    def pad_probe(self, b, i, j):
        end = int(self.offs[b, i]) + self.sizes[b]
        assert j < self.gap(b, i)
        return (b, None, self.sizes[b] + j, xor_of(j), self.lead + end + j)

    def guard_probes(self, count=16):
        """Flips just before the first and just after the last shard of the batch."""
        out = []
        for t in range(count):
            out.append((None, None, -1 - t, xor_of(t), self.lead + self.first - 1 - t))
            out.append((None, None, t, xor_of(t), self.lead + self.last + t))
        return out

    # -- the oracle ----------------------------------------------------------------------------
    def _ask(self, b, flips, lo, hi):
        """Is stripe b, with `flips` (shard, position, xor) applied to its host copy, corrupt in
        the oracle's eyes over the columns [lo, hi)? Reconstruct, then Verify."""
        mask, st = self.masks[b], self.proto[self.sizes[b]]
        sh = [st[i, lo:hi].copy() if mask[i] else None for i in range(self.n)]
        for i, pos, x in flips:
            sh[i][pos - lo] ^= x
        if not all(mask):
            sh = cref.reconstruct(sh, list(mask), self.k, self.m)
        return not cref.verify(sh, self.k, self.m)

    def oracle_corrupt(self, b, i, pos, x, whole=False):
        """The oracle's verdict on stripe b with one flipped bit. The code works column by column
        (byte position by byte position), and the clean stripe verified in full when it was
        made, so a stripe with one flipped byte is corrupt iff the columns around that byte are:
        the oracle is asked about the WINDOW columns that hold the probe. `whole` asks it about
        the whole stripe (done for the first probe of every launch, and the two must agree)."""
        if i is None:  # no byte of the host copy changes
            key = (self.sizes[b], self.masks[b], None) if b is not None else None
            if key is None:
                return False
            if key not in self.verdicts:
                self.verdicts[key] = self._ask(b, [], 0, self.sizes[b])
            return self.verdicts[key]
        S = self.sizes[b]
        key = (S, self.masks[b], i, pos, x)
        if key not in self.verdicts:
            lo = pos // WINDOW * WINDOW
            self.verdicts[key] = self._ask(b, [(i, pos, x)], lo, min(S, lo + WINDOW))
        if whole and key not in self.whole:
            self.whole.add(key)
            assert self._ask(b, [(i, pos, x)], 0, S) == self.verdicts[key]
        return self.verdicts[key]

    def expected(self, probes):
        """The set of stripes the oracle calls corrupt, and the condition the sweep rests on: it
        flags every probe inside a compared or an input shard of a stripe that has compared
        rows (the code is MDS: every coefficient of a compared row over the k inputs is
        nonzero), and no probe outside a shard."""
        want = set()
        seen = set()
        for n_, (b, i, pos, x, a) in enumerate(probes):
            if b is not None:
                assert b not in seen, "one probe per stripe"
                seen.add(b)
            bad = self.oracle_corrupt(b, i, pos, x, whole=(n_ == 0))
            inside = i is not None
            assert bad == (inside and len(self.roles[b][1]) > 0), (b, i, pos, x, bad)
            if bad:
                want.add(b)
        return sorted(want)

    # -- launches ------------------------------------------------------------------------------
    def pin(self, orders):
        """orders: None for the rule, else one order name per launch group ("none" = rule)."""
        self.plan.set_orders(orders if orders is not None else ["none"] * self.groups)
        forms = self.plan.forms()
        if orders is not None:
            assert all(o in ("none", f) for o, f in zip(orders, forms)), (orders, forms)
        self.forms = forms

    def launch(self, probes, what):
        torch = self.torch
        want = self.expected(probes)  # on the CPU, before the launch
        idx = torch.tensor([p[4] for p in probes], dtype=torch.int64, device=self.raw.device)
        val = torch.tensor([p[3] for p in probes], dtype=torch.uint8, device=self.raw.device)
        assert len(set(p[4] for p in probes)) == len(probes)
        if probes:
            self.raw[idx] = self.raw[idx] ^ val
        self.plan.launch()
        got = self.plan.corrupt_stripes()
        self.launches += 1
        if probes:
            self.raw[idx] = self.raw[idx] ^ val
        assert self.plan.forms() == self.forms, (what, self.forms, self.plan.forms())
        if got != want:
            at = {p[0]: p for p in probes}
            missed = [at[b][:4] for b in want if b not in got]
            spurious = [at.get(b, (b, "clean"))[:4] for b in got if b not in want]
            pytest.fail("%s, forms %s: missed (stripe, shard, position, xor) %s; spurious %s"
                        % (what, self.forms, missed[:12], spurious[:12]))

    def finish(self, what):
        """After the last launch of a case: one more clean launch flags nothing, and every byte
        of the allocation equals the expected image, sentinels included."""
        self.launch([], what + " clean")
        if not self.torch.equal(self.raw, self.want):
            d = (self.raw != self.want).nonzero().reshape(-1)[:8].tolist()
            pytest.fail("%s, forms %s: the allocation differs from the expected image at %s "
                        "(the batch starts at %d)" % (what, self.forms, d, self.lead))

    def close(self):
        self.plan.close()


def each_form(sw):
    """The rule, then every order each launch group offers, pinned one group at a time (an order
    the group's kernel does not offer is refused with RS_E_ARG)."""
    from callfs_amd import _native as N
    sw.pin(None)
    yield "rule"
    for g in range(sw.groups):
        for name in ALL_ORDER_NAMES:
            orders = ["none"] * sw.groups
            orders[g] = name
            try:
                sw.pin(orders)
            except N.NativeError as e:
                assert e.code == N.RS_E_ARG
                continue
            assert sw.forms[g] == name
            yield "%s@%d" % (name, g)
    sw.pin(None)


def uniform_probes(sw, shard, pos_list):
    pb = probed_stripes(sw.batch)
    assert len(pos_list) <= len(pb)
    return [sw.probe(b, shard(b), pos) for b, pos in zip(pb, pos_list)]


def sweep_uniform(k, m, missing, S, layout, seen=None, want_forms=None):
    """One uniform plan under the rule and every offered order: one launch per compared shard
    with all positions at once, one that flips an input shard (inputs[b % k]) at the same
    positions, one of negative probes (pitch padding of a compared shard, the guard bytes on
    both sides of the batch, and the missing shards' buffers refilled with garbage just before
    it, as before the first launch of every form), then the clean launch and the image check."""
    pos = positions(S)
    batch = stripes_for(len(pos))
    mask = [i not in missing for i in range(k + m)]
    sw = Sweep(k, m, [S] * batch, [mask] * batch, layout)
    inputs, compared, _ = sw.roles[0]
    assert compared, "a case without compared rows sweeps nothing"
    taken = []
    for form in each_form(sw):
        taken.append(form)
        sw.reset()
        for c in compared:
            sw.launch(uniform_probes(sw, lambda b: c, pos), "%s shard %d" % (form, c))
        sw.launch(uniform_probes(sw, lambda b: inputs[b % k], pos), form + " input shards")
        neg = sw.guard_probes()
        pb = probed_stripes(batch)
        for j, b in enumerate(pb):
            c = compared[j % len(compared)]
            if sw.gap(b, c):
                neg.append(sw.pad_probe(b, c, j % sw.gap(b, c)))
        sw.reset()
        sw.launch(neg, form + " outside every shard")
        sw.finish(form)
    print("RS(%d,%d) lost %s S=%d, %d stripes, %d launches: %s"
          % (k, m, list(missing), S, batch, sw.launches, " ".join(taken)))
    if seen is not None:
        seen.update(f for f in taken)
    if want_forms is not None:
        got = {f.split("@")[0] for f in taken}
        assert want_forms <= got, (sorted(want_forms), sorted(got))
    sw.close()
    return taken


@pytest.fixture(autouse=True)
def _rule_forms(native_lib):
    """The form called `rule` is the rule's: forget what other tests' tuners recorded."""
    native_lib.lib.rs_tune_table_reset(None)
    yield
    native_lib.lib.rs_tune_table_reset(None)


ALIGNED = [(10, 4, (5,)), (10, 4, ()), (6, 3, (2,)), (12, 8, (1,)), (10, 8, ()), (3, 2, (0,)),
           (3, 2, ()), (2, 4, ()), (10, 16, (0,)), (20, 16, ()), (20, 20, (3,))]


def _case_id(c):
    return "rs%d_%d-lost%s" % (c[0], c[1], "_".join(map(str, c[2])) or "none")


@pytest.mark.parametrize("layout", ["pitch", "planar"])
@pytest.mark.parametrize("S", VECTOR_SIZES + BYTE_SIZES)
@pytest.mark.parametrize("case", ALIGNED, ids=_case_id)
def test_aligned_plans(native_lib, case, S, layout):
    """Aligned shards (the pitch and the planar layout): every compared row x every position
    class x the rule and every order the plan offers; RS(20,20) {3} has two launch groups with
    compared rows in both. S < 16 runs the byte kernel with every position probed."""
    k, m, missing = case
    taken = sweep_uniform(k, m, missing, S, lay_pitch if layout == "pitch" else lay_planar)
    if S >= 16:
        assert len(taken) > 1, taken  # the rule and at least one pinned order
    if (k, m) == (20, 20):
        assert any(f.endswith("@1") for f in taken) or S < 16, taken


@pytest.mark.parametrize("base", [1, 9])
@pytest.mark.parametrize("S", [S_TILES, S_IDLE])
@pytest.mark.parametrize("case", [(10, 4, (5,)), (10, 8, (1,)), (5, 3, ())], ids=_case_id)
def test_split_plans(native_lib, case, S, base):
    """Upstream Split's layout at odd S from base offsets 1 and 9: every shard at its own byte
    offset, neighbouring shards touch, the guard bytes touch the first and the last shard. The
    realigning forms compare rows at unaligned addresses with 62 lanes of a wave active."""
    k, m, missing = case
    want = {"realign", "realign-x32", "realign-tri", "realign-tri-x32", "consecutive", "x32"}
    if not missing:  # read-only: the bit-sliced kernel on misaligned inputs
        want = {"bs-x32"}
    taken = sweep_uniform(k, m, missing, S, lay_split(base), want_forms=want)
    assert len(taken) > 1


@pytest.mark.parametrize("S", [S_TILES, S_IDLE])
@pytest.mark.parametrize("case", [(10, 4, (1,)), (10, 8, (1,))], ids=_case_id)
def test_readall_decode_into_fresh_buffers(native_lib, case, S):
    """io.ReadAll bodies: the surviving data shards at odd offsets, parity 64-B aligned, the lost
    shard rebuilt into a fresh aligned buffer; the place it had in the body is no shard and
    keeps its sentinel."""
    k, m, missing = case
    taken = sweep_uniform(k, m, missing, S, lay_readall(missing))
    assert len(taken) > 1


# ---- mixed and ragged plans: every stripe its own compared rows ---------------------------------

def patterns(k, m):
    """Seven presence masks (coprime with the probed / clean period of 4): nothing lost, one
    data shard, one parity shard, m shards lost (no compared row), and mixtures."""
    n = k + m
    lost = [(), (1,), (n - 1,), tuple(range(m)), (0, k), (k - 1, k + 1)[:m],
            tuple(range(k, k + m - 1))]
    return [tuple(i not in ls for i in range(n)) for ls in lost]


def sweep_per_stripe(sw, what):
    """Mixed and ragged plans: stripe b's probe sits at its own position in one of its own
    compared shards, chosen round-robin within its pattern; one launch per rotation, so that
    every (pattern, compared row) pair is probed at every position its stripes hold. Then the
    input shards, the negative probes and the clean launch."""
    pb = [b for b in probed_stripes(sw.batch) if sw.at[b] is not None]
    count, rank = {}, {}
    for b in pb:
        key = (sw.sizes[b], sw.masks[b])
        rank[b] = count.get(key, 0)
        count[key] = rank[b] + 1
    rounds = max(len(sw.roles[b][1]) for b in pb)
    pairs = set()
    for r in range(rounds):
        probes = []
        for b in pb:
            comp = sw.roles[b][1]
            if comp:
                c = comp[(rank[b] + r) % len(comp)]
                probes.append(sw.probe(b, c, sw.at[b]))
                pairs.add((sw.masks[b], c))
        sw.launch(probes, "%s rotation %d" % (what, r))
    assert pairs == {(mk, c) for mk in set(sw.masks) for c in roles(mk, sw.k)[1]}
    sw.launch([sw.probe(b, sw.roles[b][0][b % sw.k], sw.at[b]) for b in pb], what + " input shards")
    neg = sw.guard_probes()
    for j, b in enumerate(pb):
        comp = sw.roles[b][1]
        if comp and sw.gap(b, comp[j % len(comp)]):
            c = comp[j % len(comp)]
            neg.append(sw.pad_probe(b, c, j % sw.gap(b, c)))
    sw.reset()  # garbage in the missing shards' buffers again
    sw.launch(neg, what + " outside every shard")
    sw.finish(what)


def assign(sw, per_stripe_positions):
    """sw.at[b]: the position probed in stripe b (None: a clean stripe)."""
    sw.at = [None] * sw.batch
    for b, pos in per_stripe_positions.items():
        assert b % 4 != 3
        sw.at[b] = pos


@pytest.mark.parametrize("S", VECTOR_SIZES + BYTE_SIZES)
@pytest.mark.parametrize("k,m", [(10, 4), (10, 8), (10, 16)])
def test_mixed_plans(native_lib, k, m, S):
    """Plan.for_batch(sb, present=masks): seven patterns cycling through the batch, so
    neighbouring blocks compare different row sets; S < 16 is rs_apply_mixed_bytes."""
    pos = positions(S)
    batch = max(stripes_for(len(pos)), 4 * 7 * 3)
    pats = patterns(k, m)
    sw = Sweep(k, m, [S] * batch, [pats[b % 7] for b in range(batch)], lay_pitch, kind="mixed")
    pb = probed_stripes(batch)
    assign(sw, {b: pos[j % len(pos)] for j, b in enumerate(pb)})
    sw.pin(None)
    assert sw.forms == ["mixed"] * ((m + 15) // 16), sw.forms
    sweep_per_stripe(sw, "mixed RS(%d,%d) S=%d" % (k, m, S))
    sw.close()


def ragged_batch(repeat=1):
    """Sizes drawn from the sweep's list, mixed in one batch: per probed stripe (size, position),
    positions relative to the stripe's own size; neighbouring stripes differ in size."""
    per_size = {S: positions(S) for S in VECTOR_SIZES + BYTE_SIZES}
    todo = [(S, p) for S, ps in per_size.items() for p in ps] * repeat
    # interleave the sizes: sort by position rank within the size
    order = {}
    keyed = []
    for S, p in todo:
        order[S] = order.get(S, 0) + 1
        keyed.append((order[S], S, p))
    keyed.sort()
    batch = stripes_for(len(keyed))
    sizes, at = [], {}
    it = iter(keyed)
    for b in range(batch):
        if b % 4 != 3:
            nxt = next(it, None)
            if nxt is not None:
                sizes.append(nxt[1])
                at[b] = nxt[2]
                continue
        sizes.append((VECTOR_SIZES + BYTE_SIZES)[b % 6])
    return sizes, at


@pytest.mark.parametrize("packed", [False, True], ids=["aligned", "packed"])
@pytest.mark.parametrize("k,m", [(10, 4), (10, 8)])
def test_ragged_plans(native_lib, k, m, packed):
    """Plan.for_ragged: every stripe its own size and pattern in one launch. packed: shards back
    to back from an odd address, so heads are misaligned and neighbours touch."""
    sizes, at = ragged_batch()
    pats = patterns(k, m)
    sw = Sweep(k, m, sizes, [pats[b % 7] for b in range(len(sizes))], lay_ragged(packed),
               kind="ragged")
    assign(sw, at)
    sw.pin(None)
    assert sw.forms == ["ragged"] * ((m + 15) // 16), sw.forms
    sweep_per_stripe(sw, "ragged RS(%d,%d) %s" % (k, m, "packed" if packed else "aligned"))
    sw.close()


# ---- host calls ---------------------------------------------------------------------------------

def _host_stripe(k, m, S, seed):
    rng = np.random.default_rng(seed)
    d = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
    st = d + cref.encode(d, k, m)
    assert cref.verify(st, k, m)
    return st


def _oracle_status(N, st, mask, k, m, flips, shards=None):
    """RS_OK or RS_E_CORRUPT as Codec.Decode finds it: Reconstruct, then Verify. shards: a list
    that receives the stripe as the oracle leaves it."""
    sh = [st[i].copy() if mask[i] else None for i in range(k + m)]
    for i, pos, x in flips:
        sh[i][pos] ^= x
    if not all(mask):
        sh = cref.reconstruct(sh, list(mask), k, m)
    if shards is not None:
        shards[:] = sh
    return N.RS_OK if cref.verify(sh, k, m) else N.RS_E_CORRUPT


def _vp(arrs):
    return (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


def host_batch_sweep(N, k, m, sizes, lost, clean=4):
    """rs_reconstruct_batch over stripes of `sizes`: per call every probed stripe carries one flip
    (every byte of its last vector, byte 0, one middle byte, in each compared shard and in an
    input shard in turn); status[b] and the return code are the oracle's. Every `clean`-th
    stripe carries no flip."""
    n, B = k + m, len(sizes)
    ctx = N.default_context().handle
    mask = [i not in lost for i in range(n)]
    inputs, compared, _ = roles(mask, k)
    full = [_host_stripe(k, m, S, 1000 + S) for S in sizes]
    plist = [sorted(set(range(S // 16 * 16 if S % 16 else max(0, S - 16), S)) | {0, S // 2})
             for S in sizes]
    calls = 0
    for shard_of in [lambda b, c=c: c for c in compared] + [lambda b: inputs[b % k]]:
        for t in range(max(len(p) for p in plist) + 1):  # the last call is clean
            sh = [[x.copy() for x in f] for f in full]
            lens = (ctypes.c_size_t * (B * n))(*[S for S in sizes for _ in range(n)])
            want, rebuilt = [], []
            for b in range(B):
                for i in lost:
                    sh[b][i][:] = 0x5A
                    lens[b * n + i] = 0
                flips = []
                if b % clean != clean - 1 and t < len(plist[b]):
                    pos = plist[b][t]
                    flips = [(shard_of(b), pos, xor_of(pos))]
                    sh[b][flips[0][0]][pos] ^= flips[0][2]
                rebuilt.append([])
                want.append(_oracle_status(N, full[b], mask, k, m, flips, rebuilt[-1]))
                assert (want[-1] == N.RS_E_CORRUPT) == bool(flips)
            status = (ctypes.c_int * B)(*[77] * B)
            rc = N.lib.rs_reconstruct_batch(ctx, k, m, B, _vp([x for s in sh for x in s]), lens, 1,
                                            status)
            calls += 1
            assert list(status) == want, (k, m, t, [b for b in range(B) if status[b] != want[b]])
            assert rc == next((s for s in want if s), N.RS_OK)
            for b in range(B):
                for i in lost:  # what the oracle rebuilds from the same (flipped) inputs
                    assert np.array_equal(sh[b][i], rebuilt[b][i]), (b, i)
    return calls


@pytest.mark.parametrize("k,m,lost", [(10, 4, (1,)), (16, 4, ()), (3, 2, (0,))])
def test_host_reconstruct_batch(native_lib, k, m, lost):
    """The small in-place transport (rs_apply_small_ragged, its last-vector byte mask and its own
    status merge): sizes 1 + 97 b, so every residue of S % 16 and stripes below one vector."""
    sizes = [1 + 97 * b for b in range(24)]
    assert host_batch_sweep(native_lib, k, m, sizes, lost) > 0


def host_object_sweep(N, k, m, S, L, lost, plist, decode):
    """One rs_verify or rs_codec_decode call per probe: each position of plist in every compared
    shard; the return code (and rs_verify's flag) is the oracle's."""
    n = k + m
    ctx = N.default_context().handle
    full = _host_stripe(k, m, S, 31 + S)
    mask = [i not in lost for i in range(n)]
    _, compared, _ = roles(mask, k)
    calls = 0
    for c in compared:
        for pos in plist + [None]:
            flips = [(c, pos, xor_of(pos))] if pos is not None else []
            sh = [x.copy() for x in full]
            lens = (ctypes.c_size_t * n)(*[S] * n)
            for i in lost:
                sh[i][:] = 0x5A
                lens[i] = 0
            for i, p, x in flips:
                sh[i][p] ^= x
            want = _oracle_status(N, full, mask, k, m, flips)
            assert (want == N.RS_E_CORRUPT) == bool(flips)
            if decode:
                obj = np.full(L, 0xC3, np.uint8)
                rc = N.lib.rs_codec_decode(ctx, k, m, _vp(sh), lens, obj.ctypes.data, L)
                assert rc == want, (c, pos, rc)
                for i in lost:
                    assert np.array_equal(sh[i], full[i])
            else:
                ok = ctypes.c_int(-1)
                rc = N.lib.rs_verify(ctx, k, m, _vp(sh), lens, ctypes.byref(ok))
                assert rc == N.RS_OK and ok.value == int(want == N.RS_OK), (c, pos, rc, ok.value)
            calls += 1
    return calls


def test_host_verify_and_decode(native_lib):
    """rs_verify (four compared shards) and rs_codec_decode ({1} lost: three) of a 10,007-byte
    RS(10,4) object: every byte of the last vector of every compared shard, one call each."""
    L = 10_007
    S = -(-L // 10)
    last = list(range(S // 16 * 16, S))
    assert host_object_sweep(native_lib, 10, 4, S, L, (), last, decode=False) < 50
    assert host_object_sweep(native_lib, 10, 4, S, L, (1,), last, decode=True) < 50


# ---- child processes: settings read once per process -------------------------------------------

def child_nibble():
    """CALLFS_RS_BITSLICE=0: the nibble kernels behind the bit-sliced rule. The wide ring at R
    9..16, read-only launches at R <= 8 (the all-compared triples, kLdsVerify, the v_perm
    kernel) and R 5..8 rings with compared rows, under the rule and every order offered."""
    seen = set()
    cases = [(10, 16, (0,)), (20, 16, ()), (10, 12, ()), (10, 9, (0,)),   # the wide ring
             (10, 4, ()), (10, 8, ()), (6, 3, ()), (3, 2, ()),            # read-only, R <= 8
             (12, 8, (1,)), (10, 8, (1,)), (10, 6, (2,))]                 # R 5..8, compared rows
    for k, m, missing in cases:
        for S in (S_TILES, S_IDLE):
            taken = sweep_uniform(k, m, missing, S, lay_planar, seen=seen)
            assert not any(f.startswith("bs") for f in taken), taken
            print("ok RS(%d,%d) lost %s S=%d: %s" % (k, m, list(missing), S, " ".join(taken)),
                  flush=True)
    for k, m, missing, base in ((10, 8, (), 1), (10, 4, (), 9)):  # what bs-x32 took over in Split
        taken = sweep_uniform(k, m, missing, S_TILES, lay_split(base), seen=seen)
        assert not any(f.startswith("bs") for f in taken), taken
        print("ok RS(%d,%d) split S=%d: %s" % (k, m, S_TILES, " ".join(taken)), flush=True)
    return len(cases) * 2 + 2


def slice_cuts(grid, lim):
    """The first tile of every slice but the first, as launch_util.hpp launch_slices cuts a grid
    of `grid` tiles under a limit of `lim`: equal consecutive slices, one slice when the grid is
    no more than twice the limit."""
    nsl = -(-grid // lim) if grid // 2 > lim else 1
    per = -(-grid // nsl)
    return list(range(per, grid, per))


def child_sliced():
    """CALLFS_RS_MAX_TILES_PER_LAUNCH=1024: a ragged grid cut into slices (rs_mixed.hip
    launch_ragged always slices). The batch opens with 684 stripes of three tiles each, then the
    mixed sizes: 3,088 tiles, cut into four slices of 772. The first cut falls inside stripe
    257, between its first and its second tile, the second inside stripe 514, between its second
    and its third. Every stripe that holds a cut is probed at the cut's byte - 1 and at the
    cut's byte in a pattern that compares every parity row; its neighbours (where they are not
    clean stripes), and the stripes on both sides of a cut that falls between two stripes, at
    their last and their first byte."""
    k, m = 4, 2
    sizes, at = ragged_batch()
    lead = 684
    sizes = [S_TILES] * lead + sizes
    tiles = [max(1, -(-(S // 16) // 512)) for S in sizes]  # ragged_tables.hpp ragged_tiles
    tile0 = np.concatenate([[0], np.cumsum(tiles)])
    cuts = slice_cuts(int(tile0[-1]), 1024)
    assert int(tile0[-1]) == 3088 and cuts == [772, 1544, 2316], (int(tile0[-1]), cuts)
    pats = patterns(k, m)
    masks = [pats[b % 7] for b in range(len(sizes))]
    pos = positions(S_TILES)
    head = {b: pos[j % len(pos)] for j, b in enumerate(probed_stripes(lead))}
    head.update({b + lead: p for b, p in at.items()})
    inside, between = [], []   # (stripe, byte at the cut); stripes whose first tile opens a slice
    for t in cuts:
        b = int(np.searchsorted(tile0, t, side="right")) - 1
        if t > tile0[b]:
            inside.append((b, int(t - tile0[b]) * 8192))
        else:
            between.append(b)
    assert inside[:2] == [(257, 8192), (514, 16384)], inside

    def force(b, where):
        if b % 4 != 3 and 0 <= b < len(sizes):  # every fourth stripe stays clean
            head[b] = where if where >= 0 else sizes[b] + where
            masks[b] = pats[0]
            return True
        return False

    for b, _ in inside:
        force(b - 1, -1), force(b + 1, 0)
    for b in between:
        force(b - 1, -1), force(b, 0)
    for b, _ in inside:
        force(b, 0)
    sw = Sweep(k, m, sizes, masks, lay_ragged(False), kind="ragged")
    cases = 0
    for side in (-1, 0):
        probed = [(b, B + side) for b, B in inside if force(b, B + side)]
        assert probed[:2] == [(257, 8192 + side), (514, 16384 + side)]
        assign(sw, head)
        for b, where in probed + [(256, S_TILES - 1), (258, 0), (513, S_TILES - 1)]:  # 515 is clean
            assert sw.at[b] == where and len(sw.roles[b][1]) == m, (b, where)
        sw.pin(None)
        assert sw.forms == ["ragged"], sw.forms
        sw.reset()
        sweep_per_stripe(sw, "sliced ragged, cuts at tiles %s, probes %s" % (cuts, probed))
        cases += 1
        print("ok sliced ragged: slices start at tiles %s; (stripe, byte) probed %s"
              % (cuts, probed), flush=True)
    sw.close()
    return cases


def _host_counts(N):
    c = N.HostCounters()
    N.check(N.lib.rs_host_counters_read(N.default_context().handle, ctypes.byref(c)))
    return c.calls, c.chunks


def child_chunked():
    """CALLFS_RS_CHUNK_BYTES=65536 CALLFS_RS_SMALL_MAX_BYTES=0: the chunk pipeline. An RS(10,4)
    object of 5 column chunks of 4,096 and a 7-byte one (host_path.hpp chunk_geometry: 65,536 /
    14 shards, rounded down to 4 KiB): probes at each column cut -1 and +0 and at every byte of
    the last chunk. Then batches of 40 stripes: 1,000-byte shards move four stripes per chunk
    (65,536 / (14 x 1,024)), ten chunks per call; every third stripe is clean, so over the
    batch each place in a chunk, the last included, holds probed and clean stripes. Two sizes
    in one batch take the ragged pipeline, whose chunks are packed by bytes: clean periods 3
    and 4. The chunk counts are asserted per kind of call."""
    from callfs_amd import _native as N
    k, m, cw = 10, 4, 4096
    S = 5 * cw + 7
    cuts = [c * cw + d for c in range(1, 6) for d in (-1, 0)]
    plist = sorted(set(cuts) | set(range(5 * cw, S)) | {0})
    L = k * S - 3
    c0, h0 = _host_counts(N)
    calls = host_object_sweep(N, k, m, S, L, (1,), plist, decode=True)
    calls += host_object_sweep(N, k, m, S, L, (), plist, decode=False)
    c1, h1 = _host_counts(N)
    assert (c1 - c0, h1 - h0) == (calls, 6 * calls), (calls, c1 - c0, h1 - h0)
    print("ok chunked object: %d calls, %d chunks" % (calls, h1 - h0), flush=True)
    calls = host_batch_sweep(N, k, m, [1000] * 40, (1,), clean=3)
    c2, h2 = _host_counts(N)
    assert (c2 - c1, h2 - h1) == (calls, 10 * calls), (calls, c2 - c1, h2 - h1)
    print("ok chunked uniform batches: %d calls, %d chunks" % (calls, h2 - h1), flush=True)
    two = [1000 + (b & 1) for b in range(40)]
    calls = host_batch_sweep(N, k, m, two, (0, 13), clean=3)
    calls += host_batch_sweep(N, k, m, two, (0, 13), clean=4)
    c3, h3 = _host_counts(N)
    assert c3 - c2 == calls and h3 - h2 >= 4 * calls, (calls, c3 - c2, h3 - h2)
    print("ok chunked two-size batches: %d calls, %d chunks" % (calls, h3 - h2), flush=True)
    return 3


CHILDREN = {
    "nibble": (child_nibble, {"CALLFS_RS_BITSLICE": "0"}),
    "sliced": (child_sliced, {"CALLFS_RS_MAX_TILES_PER_LAUNCH": "1024"}),
    "chunked": (child_chunked, {"CALLFS_RS_CHUNK_BYTES": "65536", "CALLFS_RS_SMALL_MAX_BYTES": "0"}),
}


def _child_main(group):
    from callfs_amd import _native as N
    N.lib.rs_tune_table_reset(None)
    done = CHILDREN[group][0]()
    print("verify sweep %s: %d ok" % (group, done), flush=True)


@pytest.mark.parametrize("group", list(CHILDREN))
def test_in_a_fresh_process(native_lib, group):
    """Settings the library reads once per process: each group runs the same harness in a fresh
    child, started the way tests/test_gpu_nibble_fallback.py starts its children. A failed
    assertion, a fault or the time limit in the child fails the test with its output."""
    path = os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p])
    env = dict(os.environ, PYTHONPATH=path, **CHILDREN[group][1])
    for name in ("CALLFS_RS_INPLACE_PIPELINE", "CALLFS_RS_SLOTS"):
        env.pop(name, None)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", group], cwd=ROOT,
                           env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.fail("the %s child ran into its time limit\n%s\n%s" % (group, e.stdout, e.stderr))
    out = r.stdout[-6000:] + r.stderr[-6000:]
    assert r.returncode == 0, out
    lines = r.stdout.splitlines()
    print("\n".join(lines[-3:]))
    assert lines and lines[-1].startswith("verify sweep %s: " % group), out


if __name__ == "__main__" and sys.argv[1:2] == ["child"]:
    _child_main(sys.argv[2])
    sys.exit(0)
