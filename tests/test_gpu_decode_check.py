"""Decode-check device plans (rs_plan_create_decode_check): progressive Verify on
device memory. Beside a decode-idx plan's wanted rows every compared shard j has a check row, a
syndrome accumulator that receives C[j][delivered expected] * inputs and shard j itself when it
arrives; a final launch writes no check row, tests the value it would have received and flags the
stripe. Expected bytes come from the C oracle alone: the implied shards are cref.reconstruct with
present = expect over the shards as they are (damage included), a syndrome is implied ^ actual,
and a partial feed's terms are cref.apply(C[:, delivered], inputs) with C = cref.reconstruct of
the k unit vectors. Every byte of a sentinel-filled allocation -- inputs, accumulators, unused
shards, the gaps between all buffers, the guards, stripes in no launch -- is compared after every
launch with what the rule gives."""
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
SIZES = (1, 15, 16, 17, 1023, 8192, 8193, 2 * 8192 + 83)


def _expected_set(k, m, kind):
    """k of the k+m indices: 0 the first k, 1 the last k, 2 a set that mixes data and parity."""
    n = k + m
    if kind % 3 == 0:
        return tuple(range(k))
    if kind % 3 == 1:
        return tuple(range(n - k, n))
    return tuple(sorted(set(range(n)) - set(range(1, 1 + m))))


def _sets(k, m, batch, ncmp=(2, 1, 0, 1, 2, 2, 0, 1), nwant=(None, 1, 0)):
    """Per stripe its own expected set, compared set (ncmp[b] of the other indices, from the top)
    and wanted set (all the rest, one, none)."""
    expect, wanted, compared = [], [], []
    for b in range(batch):
        e = _expected_set(k, m, b)
        rest = [i for i in range(k + m) if i not in e]
        c = rest[len(rest) - min(ncmp[b % len(ncmp)], len(rest)):] if ncmp[b % len(ncmp)] else []
        free = [i for i in rest if i not in c]
        nw = nwant[b % len(nwant)]
        expect.append(e)
        compared.append(tuple(c))
        wanted.append(tuple(free if nw is None else free[:nw]))
    return tuple(expect), tuple(wanted), tuple(compared)


@functools.lru_cache(maxsize=None)
def _coef(k, m, expect):
    """C as an (n, k) array: row w, column j = the coefficient of expected shard V[j] in shard w.
    cref.reconstruct of the k unit vectors."""
    n = k + m
    shards = [None] * n
    for j, v in enumerate(expect):
        shards[v] = np.zeros(k, dtype=np.uint8)
        shards[v][j] = 1
    C = np.stack(cref.reconstruct(shards, [i in expect for i in range(n)], k, m))
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def _reference(k, m, sizes, expect, damage, seed):
    """Per stripe (actual [n][S], implied [n][S], C). actual: a codeword of random data with the
    stripe's damage, a tuple of (shard, offset, xor value), applied; implied: what the k expected
    shards of `actual` imply, cref.reconstruct with present = expect."""
    rng = np.random.default_rng(seed)
    n = k + m
    out = []
    for b, (S, e) in enumerate(zip(sizes, expect)):
        data = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)]
        actual = np.stack(data + cref.encode(data, k, m))
        for shard, off, val in damage[b]:
            assert val & 0xFF
            actual[shard, off] ^= val
        shards = [actual[i] if i in e else None for i in range(n)]
        implied = np.stack(cref.reconstruct(shards, [i in e for i in range(n)], k, m))
        for v in e:
            assert np.array_equal(implied[v], actual[v])
        actual.setflags(write=False)
        implied.setflags(write=False)
        out.append((actual, implied, _coef(k, m, e)))
    return out


class _Arena:
    """A sentinel-filled allocation holding all k+m shards of every stripe and one accumulator per
    compared shard, with sentinel gaps between all buffers. aligned: every buffer on a 256-B
    boundary; packed: every buffer at its own odd offset. Expected and compared shards hold the
    (possibly damaged) shards; wanted shards, unused shards and accumulators start as `start`
    says: "zero" or "junk" (random)."""

    def __init__(self, k, m, sizes, expect, wanted, compared, damage=None, layout="aligned", seed=1,
                 start="zero", guard=4096):
        import torch
        dev = torch.device("cuda:0")
        self.k, self.m, self.n, self.sizes = k, m, k + m, list(sizes)
        self.B = len(sizes)
        self.expect, self.wanted, self.compared = expect, wanted, compared
        damage = tuple(damage) if damage is not None else ((),) * self.B
        self.ref = _reference(k, m, tuple(sizes), tuple(expect), damage, seed)
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
        self.acc = [{j: take(S) for j in compared[b]} for b, S in enumerate(sizes)]
        self.nbytes = off + 16
        img = np.full(self.nbytes, SENTINEL, dtype=np.uint8)
        for b, (actual, implied, C) in enumerate(self.ref):
            S = sizes[b]
            for i in range(self.n):
                o = self.off[b][i]
                if i in expect[b] or i in compared[b]:
                    img[o:o + S] = actual[i]
                else:
                    img[o:o + S] = 0 if start == "zero" else rng.integers(0, 256, S, dtype=np.uint8)
            for o in self.acc[b].values():
                img[o:o + S] = 0 if start == "zero" else rng.integers(0, 256, S, dtype=np.uint8)
        self.raw = torch.full((self.nbytes + 2 * guard + 256,), SENTINEL, dtype=torch.uint8, device=dev)
        self.lead = guard + (-(self.raw.data_ptr() + guard) % 256)
        self.raw[self.lead:self.lead + self.nbytes].copy_(torch.from_numpy(img))
        torch.cuda.synchronize()
        self.start_img = self.raw.cpu().numpy()
        self.base = self.raw.data_ptr() + self.lead

    # a delivery: per stripe the set of shard indices delivered with a launch
    def deliver(self, positions=(), compared=()):
        """Positions of V and positions of the stripe's compared list (those it has)."""
        return [{self.expect[b][j] for j in positions} |
                {self.compared[b][c] for c in compared if c < len(self.compared[b])} for b in range(self.B)]

    def everything(self):
        return self.deliver(range(self.k), range(self.n))

    def pointers(self, deliver, compared=None):
        compared = self.compared if compared is None else compared
        inp, dst, chk, flags = [], [], [], []
        for b in range(self.B):
            for i in range(self.n):
                inp.append(self.base + self.off[b][i] if i in deliver[b] else 0)
                dst.append(self.base + self.off[b][i] if i in self.wanted[b] else 0)
                chk.append(self.base + self.acc[b][i] if i in compared[b] else 0)
            flags.append([i in self.expect[b] for i in range(self.n)])
        return flags, inp, dst, chk

    def plan(self, deliver, store=False, final=False, compared=None):
        from callfs_amd.device import Plan
        flags, inp, dst, chk = self.pointers(deliver, compared)
        return Plan.decode_check(self.k, self.m, self.sizes, flags, inp, dst, chk, store=store, final=final)

    def in_launch(self, b, deliver, final, compared=None):
        cmp_b = (self.compared if compared is None else compared)[b]
        return bool((deliver[b] and (self.wanted[b] or cmp_b)) or (final and cmp_b))

    def terms(self, b, deliver, compared=None):
        """{row: the value the rule computes for the row} of stripe b, from the oracle."""
        actual, implied, C = self.ref[b]
        cmp_b = (self.compared if compared is None else compared)[b]
        S = self.sizes[b]
        rows = sorted(set(self.wanted[b]) | set(cmp_b))
        pos = [j for j, v in enumerate(self.expect[b]) if v in deliver[b]]
        if pos and rows:
            t = cref.apply(C[rows][:, pos], [actual[self.expect[b][j]] for j in pos])
        else:
            t = [np.zeros(S, dtype=np.uint8) for _ in rows]
        out = dict(zip(rows, t))
        for j in cmp_b:
            if j in deliver[b]:
                out[j] = out[j] ^ actual[j]
        return out

    def after(self, image, deliver, store=False, final=False, compared=None):
        """(`image` after a launch of plan(deliver, store, final, compared), the stripes it flags),
        by the rule and the oracle's terms."""
        out = image.copy()
        flagged = []
        for b, S in enumerate(self.sizes):
            if not self.in_launch(b, deliver, final, compared):
                continue
            bad = False
            for row, t in self.terms(b, deliver, compared).items():
                o = self.lead + (self.off[b][row] if row in self.wanted[b] else self.acc[b][row])
                new = t if store else out[o:o + S] ^ t
                if final and row not in self.wanted[b]:
                    bad |= bool(new.any())
                else:
                    out[o:o + S] = new
            if bad:
                flagged.append(b)
        return out, flagged

    def damaged(self):
        """The stripes in which some compared shard differs from what the expected shards imply."""
        return [b for b in range(self.B)
                if any(not np.array_equal(self.ref[b][0][j], self.ref[b][1][j]) for j in self.compared[b])]

    def complete(self, image):
        """`image` with every wanted shard holding cref.reconstruct's bytes."""
        out = image.copy()
        for b, S in enumerate(self.sizes):
            for w in self.wanted[b]:
                o = self.lead + self.off[b][w]
                out[o:o + S] = self.ref[b][1][w]
        return out

    def syndromes(self, image):
        """`image` with every accumulator holding implied ^ actual."""
        out = image.copy()
        for b, S in enumerate(self.sizes):
            for j, o in self.acc[b].items():
                out[self.lead + o:self.lead + o + S] = self.ref[b][0][j] ^ self.ref[b][1][j]
        return out

    def wrong(self, image):
        import torch
        torch.cuda.synchronize()
        return np.flatnonzero(self.raw.cpu().numpy() != image)[:8].tolist()

    def bytes(self, deliver, store, final, compared=None):
        total = 0
        for b, S in enumerate(self.sizes):
            if not self.in_launch(b, deliver, final, compared):
                continue
            nc = len((self.compared if compared is None else compared)[b])
            per_check = (0 if store else 1) if final else (1 if store else 2)
            total += S * (len(deliver[b]) + (1 if store else 2) * len(self.wanted[b]) + per_check * nc)
        return total


def _run(ar, launches, groups=None):
    """Launches (deliver, store, final) in order, checking the whole image and the flags after
    each against the rule; returns the image and the stripes the last launch flagged."""
    img = ar.start_img
    flagged = []
    for q, (deliver, store, final) in enumerate(launches):
        want, flagged = ar.after(img, deliver, store, final)
        plan = ar.plan(deliver, store, final)
        if groups is not None and any(ar.in_launch(b, deliver, final) for b in range(ar.B)):
            assert plan.forms() == ["decode-check" if final else "decode-idx"] * groups
        assert plan.bytes == ar.bytes(deliver, store, final)
        plan.launch()
        assert ar.wrong(want) == [], (q, store, final)
        assert plan.corrupt_stripes() == flagged, (q, store, final)
        assert plan.corrupt_stripes() == []  # reported once, then cleared
        plan.close()
        img = want
    return img, flagged


def _damage(ar_sets, sizes, which):
    """Per stripe: b % 4 == 1 a flipped byte in its last compared shard (the last byte), b % 4 ==
    0 one in an expected shard (the middle byte), else none; nothing when not `which`."""
    expect, wanted, compared = ar_sets
    out = []
    for b, S in enumerate(sizes):
        if which and b % 4 == 1 and compared[b]:
            out.append(((compared[b][-1], S - 1, 0x01),))
        elif which and b % 4 == 0:
            out.append(((expect[b][3 % len(expect[b])], S // 2, 0x80),))
        else:
            out.append(())
    return tuple(out)


def _feed_launches(ar, feed, store_first, seed):
    k = ar.k
    perm = [int(i) for i in np.random.default_rng(seed).permutation(k)]
    if feed == "all":  # the one-shot decode plus Verify
        return [(ar.everything(), True, True)]
    if feed == "singles":
        items = [("e", j) for j in perm] + [("c", 0), ("c", 1)]
        order = [int(i) for i in np.random.default_rng(seed + 1).permutation(len(items))]
        items = [items[i] for i in order]
        first = next(i for i, it in enumerate(items) if it[0] == "e")  # a store must reach every stripe
        items.insert(0, items.pop(first))
        assert [it for it in items if it[0] == "e"] != [("e", j) for j in range(k)]
        assert any(t == "c" for t, _ in items[:-2])  # a compared shard arrives before the last expected ones
        ds = [ar.deliver([j], []) if t == "e" else ar.deliver([], [j]) for t, j in items]
    else:
        assert feed == "3+7+compared"
        ds = [ar.deliver(sorted(perm[:3]), []), ar.deliver(sorted(perm[3:]), []), ar.deliver([], range(ar.n))]
    return [(d, store_first and q == 0, q == len(ds) - 1) for q, d in enumerate(ds)]


@pytest.mark.parametrize("damage", [False, True], ids=["clean", "damaged"])
@pytest.mark.parametrize("start", ["merge-from-zero", "store-first-over-junk"])
@pytest.mark.parametrize("feed", ["all", "singles", "3+7+compared"])
@pytest.mark.parametrize("layout", ["aligned", "packed"])
def test_sizes_sets_and_feeds(native_lib, layout, feed, start, damage):
    """RS(10,4) over the tail-only stripe, one vector, vector plus tail, both sides of the tile
    edge and a tail behind full tiles; every stripe its own expected set (first k, last k, one that
    mixes data and parity), wanted set and compared set (two, one or none of the rest). After every
    non-final launch the check rows are the oracle's partial syndromes; after the final launch
    the wanted rows are cref.reconstruct's, the check rows what they were, and the flagged stripes
    exactly the damaged ones."""
    k, m = 10, 4
    sets = _sets(k, m, len(SIZES))
    expect, wanted, compared = sets
    assert {len(c) for c in compared} == {0, 1, 2} and {len(w) for w in wanted} >= {0, 1, 2}
    store_first = start.startswith("store")
    ar = _Arena(k, m, SIZES, expect, wanted, compared, _damage(sets, SIZES, damage), layout, seed=5,
                start="junk" if store_first or feed == "all" else "zero")
    hit = ar.damaged()
    assert hit == ([b for b in range(len(SIZES)) if compared[b] and b % 4 in (0, 1)] if damage else [])
    if damage:
        assert hit and len(hit) < sum(1 for c in compared if c)
    launches = _feed_launches(ar, feed, store_first, seed=11)
    # on the CPU, before any launch: the rule's chain ends in the oracle's syndromes
    img = ar.start_img
    for d, store, final in launches[:-1]:
        img, none = ar.after(img, d, store, False)
        assert none == []
    d, store, final = launches[-1]
    assert final
    full, none = ar.after(img, d, store, False)
    if feed != "all":
        assert np.array_equal(full, ar.syndromes(ar.complete(ar.start_img)))
    got, flagged = _run(ar, launches, groups=1)
    assert flagged == hit
    # wanted rows complete, check rows byte for byte what they were before the final launch
    assert np.array_equal(got, ar.complete(img))
    assert ar.wrong(ar.complete(img)) == []


@pytest.mark.parametrize("mode", ["store", "merge"])
@pytest.mark.parametrize("k,m,nwant", [(10, 4, 2), (10, 8, 4), (20, 12, 6)], ids=["rt4", "rt8", "rt16"])
def test_detection_sweep(native_lib, k, m, nwant, mode):
    """One damaged byte per stripe at the first byte, in wave 1, in wave 3, on both sides of the
    tile edges and in the tail, once in a compared shard and once in an expected shard, with clean
    stripes between them: each flip flags its stripe alone. store: one FINAL|STORE launch; merge:
    all expected shards but one merged from zero, then the last and the compared shards FINAL."""
    S = 2 * 8192 + 5
    offsets = (0, 16 * 64 + 3, 16 * 200, 8191, 8192, 16383, S - 1)
    n = k + m
    e = _expected_set(k, m, 2)
    rest = [i for i in range(n) if i not in e]
    cmp_ = tuple(rest[nwant:])
    want = tuple(rest[:nwant])
    assert len(cmp_) == m - nwant and max(len(want) + len(cmp_), 1) == m
    damage = []
    for q, off in enumerate(offsets):
        damage += [((cmp_[q % len(cmp_)], off, 1 + q),), (), ((e[(3 * q) % k], off, 0x10 + q),)]
    B = len(damage)
    hit = [b for b in range(B) if damage[b]]
    ar = _Arena(k, m, [S] * B, (e,) * B, (want,) * B, (cmp_,) * B, tuple(damage), "packed", seed=100 * k + m,
                start="junk" if mode == "store" else "zero")
    # every C entry is nonzero, so an expected-shard error reaches every check row
    assert _coef(k, m, e)[rest].all()
    for b in hit:
        actual, implied, C = ar.ref[b]
        shard, off, val = damage[b][0]
        synd = [int(actual[j][off] ^ implied[j][off]) for j in cmp_]
        assert all(synd) if shard in e else [bool(s) for s in synd] == [j == shard for j in cmp_]
    assert ar.damaged() == hit
    if mode == "store":
        launches = [(ar.everything(), True, True)]
    else:
        launches = [(ar.deliver(range(k - 1), []), False, False), (ar.deliver([k - 1], range(n)), False, True)]
    img, flagged = _run(ar, launches, groups=1)
    assert flagged == hit
    assert np.array_equal(img, ar.complete(img))


def test_equivalence_with_a_ragged_compare(native_lib):
    """A FINAL|STORE plan's flags and rebuilt bytes are those of Plan.ragged(present = expected and
    compared, required = wanted) over the same buffers, on clean and on damaged stripes. The
    ragged plan rebuilds from the first k present shards, so the expected set here is the first k
    of expected and compared: the two then read the same (damaged) shards."""
    import torch
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    S = 2 * 8192 + 5
    offsets = (0, 16 * 64 + 3, 16 * 200, 8191, 8192, 16383, S - 1)
    e = (0, 1, 2, 4, 5, 6, 7, 8, 9, 10)
    want, cmp_ = (3,), (11, 13)
    damage = [()]
    for q, off in enumerate(offsets):
        damage += [((cmp_[q % 2], off, 1 + q),), ((e[q], off, 0x10 + q),), ()]
    B = len(damage)
    ar = _Arena(k, m, [S] * B, (e,) * B, (want,) * B, (cmp_,) * B, tuple(damage), "packed", seed=77, start="junk")
    present = [[i in e or i in cmp_ for i in range(n)] for _ in range(B)]
    assert all(tuple(i for i in range(n) if p[i])[:k] == e for p in present)
    plan = ar.plan(ar.everything(), store=True, final=True)
    plan.launch()
    flags = plan.corrupt_stripes()
    mine = ar.raw.cpu().numpy()
    plan.close()
    assert flags == ar.damaged() == [b for b in range(B) if damage[b]]
    assert np.array_equal(mine, ar.complete(ar.start_img))
    ar.raw.copy_(torch.from_numpy(ar.start_img).to(ar.raw.device))  # junk in the wanted rows again
    ptrs = [ar.base + ar.off[b][i] if present[b][i] or i in want else 0 for b in range(B) for i in range(n)]
    rp = Plan.ragged(k, m, [S] * B, ptrs, present=present, required=[[i in want for i in range(n)]] * B)
    rp.launch()
    assert rp.corrupt_stripes() == flags
    assert ar.wrong(mine) == []
    rp.close()


def test_final_scan_with_nothing_delivered(native_lib):
    """After a complete non-final feed a final plan with no input only scans the accumulators: it
    flags the damaged stripes, writes nothing, twice (idempotent); a non-final plan with no input
    has no launch group. A compared shard left out of the final plan (check = NULL) is not
    tested."""
    k, m = 10, 4
    sizes = SIZES[1:]
    sets = _sets(k, m, len(sizes))
    expect, wanted, compared = sets
    ar = _Arena(k, m, sizes, expect, wanted, compared, _damage(sets, sizes, True), "packed", seed=9, start="junk")
    img, none = _run(ar, [(ar.deliver(range(4), [1]), True, False), (ar.deliver(range(4, k), [0]), False, False)])
    assert none == [] and np.array_equal(img, ar.syndromes(ar.complete(ar.start_img)))
    nothing = ar.deliver()
    idle = ar.plan(nothing)
    assert idle.forms() == [] and idle.bytes == 0
    idle.launch()
    assert ar.wrong(img) == [] and not idle.corrupt()
    idle.close()
    plan = ar.plan(nothing, final=True)
    assert plan.forms() == ["decode-check"]
    assert plan.bytes == ar.bytes(nothing, False, True) > 0
    for _ in range(2):
        plan.launch()
        assert ar.wrong(img) == []
        assert plan.corrupt_stripes() == ar.damaged() != []
    plan.close()
    # without the damaged compared shards: nothing to flag
    hit = ar.damaged()
    kept = tuple(tuple(j for j in c if np.array_equal(ar.ref[b][0][j], ar.ref[b][1][j])) for b, c in enumerate(compared))
    assert any(len(kept[b]) < len(compared[b]) for b in hit) and any(kept[b] for b in hit)
    want, flagged = ar.after(img, nothing, False, True, compared=kept)
    assert flagged == []  # (an expected-shard error reaches every check row: those stripes keep none)
    plan = ar.plan(nothing, final=True, compared=kept)
    plan.launch()
    assert ar.wrong(want) == [] and np.array_equal(want, img)
    assert plan.corrupt_stripes() == flagged
    plan.close()


@pytest.mark.parametrize("k,m", [(1, 3), (3, 2), (4, 2), (16, 4)])
def test_profiles(native_lib, k, m):
    """Small and wide profiles: the first half of the expected shards stored over junk, the second
    half merged, then the compared shards with the final launch."""
    sizes = [17, 8193] * 3
    sets = _sets(k, m, len(sizes))
    expect, wanted, compared = sets
    ar = _Arena(k, m, sizes, expect, wanted, compared, _damage(sets, sizes, True), "packed", seed=100 * k + m,
                start="junk")
    halves = [list(range(max(1, k // 2))), list(range(max(1, k // 2), k))]
    launches = [(ar.deliver(halves[0], []), True, False)]
    if halves[1]:
        launches.append((ar.deliver(halves[1], []), False, False))
    launches.append((ar.deliver([], range(ar.n)), False, True))
    img, flagged = _run(ar, launches, groups=1)
    assert flagged == ar.damaged() != []
    assert np.array_equal(img, ar.complete(img))


def test_two_launch_groups(native_lib):
    """RS(10,20) with 12 wanted and 8 compared rows: 16 + 4 rows, with check rows in both launch
    groups, beside a stripe with fewer than 17 rows, which the second launch leaves alone."""
    k, m, n = 10, 20, 30
    sizes = [8193, 17, 4000]
    e = _expected_set(k, m, 2)
    rest = [i for i in range(n) if i not in e]
    cmp_ = tuple(rest[3:5] + rest[13:19])  # rows on both sides of the 16-row boundary
    want = tuple(i for i in rest if i not in cmp_)
    assert len(want) == 12 and len(cmp_) == 8
    rows = sorted(want + cmp_)
    assert rows.index(cmp_[4]) < 16 <= rows.index(cmp_[5])
    expect = (e, e, _expected_set(k, m, 0))
    wanted = (want, want, (12, 13))
    compared = (cmp_, cmp_, (29,))
    damage = (((cmp_[7], 8192, 3),), (), ((29, 5, 1),))
    for mode in ("store", "merge"):
        ar = _Arena(k, m, sizes, expect, wanted, compared, damage, "aligned", seed=3, start="junk")
        if mode == "store":
            launches = [(ar.everything(), True, True)]
        else:
            launches = [(ar.deliver(range(k), [0, 1, 2]), True, False), (ar.deliver([], range(3, n)), False, True)]
        img, flagged = _run(ar, launches, groups=2)
        assert flagged == ar.damaged() == [0, 2]
        assert np.array_equal(img, ar.complete(img))


def test_wide_lds(native_lib):
    """RS(200,16) with 130 delivered shards and 3 compared ones: 133 * 512 B of tables, past 64 KiB
    of LDS, in a final merge launch; and the one-shot form with all 203."""
    k, m = 200, 16
    sizes = [40, 40]
    expect = (tuple(range(k)), tuple(range(16, k + 16)))
    wanted = (tuple(range(k, k + 13)), (0, 7))
    compared = (tuple(range(k + 13, k + 16)), (1, 2, 15))
    damage = ((), ((15, 39, 0x40),))
    ar = _Arena(k, m, sizes, expect, wanted, compared, damage, "aligned", seed=9, start="junk")
    first = list(range(130, 200))
    assert (130 + 3) * 512 > 64 << 10
    img, flagged = _run(ar, [(ar.deliver(first, []), True, False), (ar.deliver(range(130), range(3)), False, True)],
                        groups=1)
    assert flagged == ar.damaged() == [1]
    assert np.array_equal(img, ar.complete(img))
    ar = _Arena(k, m, sizes, expect, wanted, compared, damage, "aligned", seed=9, start="junk")
    img, flagged = _run(ar, [(ar.everything(), True, True)], groups=1)
    assert flagged == [1] and np.array_equal(img, ar.complete(ar.start_img))


def test_graph_capture(native_lib):
    """A captured final launch without wanted rows, replayed twice: it writes nothing and flags
    the damaged stripes after each replay."""
    import torch
    k, m = 10, 4
    sizes = [65_541, 9, 8192, 3 * 8192 + 17, 100, 40_000]
    expect, _, compared = _sets(k, m, len(sizes))
    wanted = ((),) * len(sizes)
    sets = (expect, wanted, compared)
    ar = _Arena(k, m, sizes, expect, wanted, compared, _damage(sets, sizes, True), "aligned", seed=41, start="zero")
    img, none = _run(ar, [(ar.deliver(range(k - 1), [0]), False, False)])
    last = ar.deliver([k - 1], [1])
    want, flagged = ar.after(img, last, False, True)
    assert np.array_equal(want, img) and flagged == ar.damaged() != []
    plan = ar.plan(last, final=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        plan.launch(s)
    torch.cuda.synchronize()
    assert plan.corrupt_stripes(s) == flagged
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch(s)
    assert ar.wrong(img) == [] and plan.corrupt_stripes(s) == []  # capture runs nothing
    for _ in range(2):
        g.replay()
        assert ar.wrong(img) == []
        assert plan.corrupt_stripes(s) == flagged
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
bufs, flags, inp, chk, hit = [], [], [], [], []
for b, S in enumerate(sizes):
    e = [(0, 1), (1, 2), (0, 2)][b % 3]
    c = [i for i in range(n) if i not in e][0]
    shards = [rng.integers(1, 256, S, dtype=np.uint8) if i in e else None for i in range(n)]
    full = np.stack(cref.reconstruct(shards, [i in e for i in range(n)], k, m))
    if b % 5 == 2:   # one byte, in the stripe's last tile or its tail
        full[c if b % 2 else e[0], S - 1 - (b % 3) * 16] ^= 1 + b
        hit.append(b)
    t = torch.from_numpy(full).to(dev)
    bufs.append(t)
    flags.append([i in e for i in range(n)])
    inp += [t[i].data_ptr() for i in range(n)]
    chk += [t[i].data_ptr() if i == c else 0 for i in range(n)]   # FINAL|STORE: the pointer only marks the index
plan = Plan.decode_check(k, m, sizes, flags, inp, [0] * len(inp), chk, store=True, final=True)
assert plan.forms() == ["decode-check"], plan.forms()
plan.launch()
got = plan.corrupt_stripes()
plan.close()
print("sliced decode-check child:", "ok" if got == hit and hit else "flagged %r, damaged %r" % (got, hit))
sys.exit(0 if got == hit and hit else 1)
"""


def test_sliced_grid(native_lib):
    """CALLFS_RS_MAX_TILES_PER_LAUNCH is read once per process: a fresh child runs an RS(2,1)
    batch of at least 2,100 tiles in slices of at most 1,024, with slice boundaries inside
    stripes; the damaged stripes, and they alone, are flagged."""
    env = dict(os.environ)
    env["CALLFS_RS_MAX_TILES_PER_LAUNCH"] = "1024"
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _SLICED_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sliced decode-check child: ok" in r.stdout


def test_api_edges(native_lib):
    """The error order the header states, with nothing created; forms, groups and bytes in the four
    flag combinations; tuning, pinning and ceilings."""
    import torch
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [8192 + 16 * 3 + 5, 11, 4000, 16]
    B = len(sizes)
    sets = _sets(k, m, B)
    expect, wanted, compared = sets
    ar = _Arena(k, m, sizes, expect, wanted, compared, None, "aligned", seed=33, start="junk")
    L = N.lib
    ctx = N.default_context()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    deliver = ar.deliver([2, 5], [0])
    flags0, inp0, dst0, chk0 = ar.pointers(deliver)
    vp = lambda p: (ctypes.c_void_p * len(p))(*[x or None for x in p])  # noqa: E731
    fl = lambda rows: (ctypes.c_uint8 * (B * n))(*[1 if f else 0 for r in rows for f in r])  # noqa: E731
    sz = lambda v: (ctypes.c_size_t * B)(*v)  # noqa: E731

    def create(kk=k, mm=m, sizes_=sizes, flags=flags0, inp=inp0, dst=dst0, chk=chk0, bits=0, null=()):
        h = ctypes.c_void_p(0xdead)
        args = {"sizes": sz(sizes_), "expect": fl(flags), "input": vp(inp), "dst": vp(dst), "check": vp(chk)}
        for name in null:
            args[name] = None
        rc = L.rs_plan_create_decode_check(ctx.handle, 0, kk, mm, B, args["sizes"], args["expect"], args["input"],
                                           args["dst"], args["check"], bits, ctypes.byref(h))
        if rc != 0:
            assert h.value in (None, 0xdead)  # nothing created
        else:
            L.rs_plan_destroy(h)
        return rc

    zero = list(sizes)
    zero[0] = 0
    few = [list(r) for r in flags0]
    few[1][expect[1][0]] = False
    many = [list(r) for r in flags0]
    many[3][[i for i in range(n) if i not in expect[3]][0]] = True
    assert wanted[1] and compared[0] and compared[1] and not compared[2]
    in_unexpected = list(inp0)
    in_unexpected[1 * n + wanted[1][0]] = ar.base  # an input at a wanted index: neither expected nor compared
    chk_expected = list(chk0)
    chk_expected[2 * n + expect[2][0]] = ar.base
    dst_expected = list(dst0)
    dst_expected[0 * n + expect[0][3]] = ar.base
    chk_and_dst = list(dst0)
    chk_and_dst[1 * n + compared[1][0]] = ar.base
    # 1. the profile, before anything else
    assert create(kk=0, null=("sizes", "input"), bits=4) == N.RS_E_INVALID_PROFILE
    assert create(kk=250, mm=10, flags=few) == N.RS_E_UNSUPPORTED
    # 2. NULL arrays, counts and flag bits, before the expect count
    for name in ("sizes", "expect", "input", "dst", "check"):
        assert create(flags=few, null=(name,)) == N.RS_E_ARG, name
    assert L.rs_plan_create_decode_check(ctx.handle, 0, k, m, B, sz(sizes), fl(flags0), vp(inp0), vp(dst0),
                                         vp(chk0), 0, None) == N.RS_E_ARG
    for bits in (4, 7, 1 << 31):
        assert create(flags=few, bits=bits) == N.RS_E_ARG
    # 3. the expect count, before misplaced pointers and sizes
    assert create(flags=few, inp=in_unexpected, sizes_=zero) == N.RS_E_TOO_FEW_SHARDS
    assert create(flags=many, sizes_=zero) == N.RS_E_ARG
    # 4. misplaced pointers, before a zero size
    for bits in (0, 1, 2, 3):
        assert create(inp=in_unexpected, sizes_=zero, bits=bits) == N.RS_E_ARG
        assert create(chk=chk_expected, sizes_=zero, bits=bits) == N.RS_E_ARG
        assert create(dst=dst_expected, sizes_=zero, bits=bits) == N.RS_E_ARG
        assert create(dst=chk_and_dst, sizes_=zero, bits=bits) == N.RS_E_ARG
        # 5. a zero size on a stripe in the launch
        assert create(sizes_=zero, bits=bits) == N.RS_E_NO_DATA
        assert create(bits=bits) == N.RS_OK
    noin = [0 if i < n else p for i, p in enumerate(inp0)]  # stripe 0 delivered nothing
    assert create(sizes_=zero, inp=noin) == N.RS_OK  # not in a non-final launch
    assert create(sizes_=zero, inp=noin, bits=2) == N.RS_E_NO_DATA  # its check rows are in a final one
    with pytest.raises(ValueError):
        Plan.decode_check(k, m, sizes, flags0[:3], inp0, dst0, chk0)
    with pytest.raises(ValueError):
        Plan.decode_check(k, m, sizes, flags0, inp0, dst0, chk0[:-1])
    # a decode-idx plan still refuses the new bit
    h = ctypes.c_void_p()
    assert L.rs_plan_create_decode_idx(ctx.handle, 0, k, m, B, sz(sizes), fl(flags0), vp([0] * (B * n)), vp(dst0), 2,
                                       ctypes.byref(h)) == N.RS_E_ARG

    # forms, groups, bytes
    seen = set()
    for store in (False, True):
        for final in (False, True):
            plan = ar.plan(deliver, store, final)
            assert int(L.rs_plan_groups(plan.handle)) == 1
            forms = (ctypes.c_int * 1)()
            assert L.rs_plan_forms(plan.handle, forms, 1) == 1
            assert forms[0] == (N.RS_ORDER_DECODE_CHECK if final else 32768)  # + RS_ORDER_CONSECUTIVE (0)
            assert plan.forms() == ["decode-check" if final else "decode-idx"]
            assert plan.bytes == ar.bytes(deliver, store, final)
            seen.add(plan.bytes)
            assert plan.tune() == ["none"]  # the tuner times nothing: no byte is touched
            with pytest.raises(N.NativeError) as ei:
                plan.set_orders(["consecutive"])
            assert ei.value.code == N.RS_E_ARG
            plan.set_orders(["none"])
            for mode in (1, 2):
                assert L.rs_plan_launch_ceiling(plan.handle, s, mode) == N.RS_E_ARG
            assert ar.wrong(ar.start_img) == [] and not plan.corrupt()
            plan.close()
    assert len(seen) == 4
    assert L.rs_tune_table_entries() == 0
    # timed launches bracket the final kernel
    plan = ar.plan(ar.everything(), store=True, final=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    plan.launch(events=(e0, e1))
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) > 0
    assert ar.wrong(ar.complete(ar.start_img)) == [] and not plan.corrupt()
    plan.close()
