"""Decode-repair device plans (rs_plan_create_decode_repair): the final launch of
a progressive decode names the corrupt shard of a mismatching byte column from the finished check
rows, repairs the wanted rows and XORs the error values into the fix buffers. Expected bytes come
from the C oracle alone, as in test_gpu_decode_check.py, whose arena and rule model the non-final
launches here run through: a true codeword from cref.encode, chosen bytes of the delivered shards
damaged, the implied shards from cref.reconstruct over the damaged inputs. A column in which one
expected or compared shard is damaged (and three check rows or more confirm it) ends with the
true shards' bytes in the wanted rows, damaged ^ true in a zeroed fix buffer and the true shard in
a fix buffer that held the shard as delivered; any other damaged column is unexplained, its wanted
bytes cref.reconstruct's over the damaged inputs. Every byte of the sentinel-filled allocations --
shards, accumulators, fix buffers, gaps, guards -- is compared after every launch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_decode_check as DC

pytestmark = pytest.mark.gpu

ROOT = DC.ROOT
SENTINEL = DC.SENTINEL
SIZES = (1, 15, 16, 17, 1023, 8192, 8193, 2 * 8192 + 83)
EDGE_S = 2 * 8192 + 5
EDGE_OFFSETS = (0, 16 * 64 + 3, 16 * 200, 8191, 8192, 16383, EDGE_S - 1)  # the wave edge, the tile edge, the tail


class _Fix:
    """The fix side of a decode-repair plan over a DC._Arena. mode "null": no fix pointer;
    "alias": fix[i] is shard i where it lies in the arena; "zero" / "delivered": a sentinel-filled
    allocation of its own with one buffer per expected and compared shard, zeroed or holding the
    shard as delivered, aligned or each at its own odd offset."""

    def __init__(self, ar, mode, layout="aligned", guard=4096):
        import torch
        self.ar, self.mode = ar, mode
        self.off = [{} for _ in range(ar.B)]
        self.raw = None
        if mode not in ("zero", "delivered"):
            return
        off = 0
        for b, S in enumerate(ar.sizes):
            for q, i in enumerate(sorted(set(ar.expect[b]) | set(ar.compared[b]))):
                off += 16
                off = (off + 255) // 256 * 256 if layout == "aligned" else (off + 2 * ((q + b) % 7)) | 1
                self.off[b][i] = off
                off += S
        self.nbytes = off + 16
        img = np.full(self.nbytes, SENTINEL, dtype=np.uint8)
        for b, S in enumerate(ar.sizes):
            for i, o in self.off[b].items():
                img[o:o + S] = 0 if mode == "zero" else ar.ref[b][0][i]
        self.raw = torch.full((self.nbytes + 2 * guard + 256,), SENTINEL, dtype=torch.uint8, device=ar.raw.device)
        self.lead = guard + (-(self.raw.data_ptr() + guard) % 256)
        self.raw[self.lead:self.lead + self.nbytes].copy_(torch.from_numpy(img))
        torch.cuda.synchronize()
        self.start_img = self.raw.cpu().numpy()
        self.base = self.raw.data_ptr() + self.lead

    def pointers(self):
        ar = self.ar
        out = []
        for b in range(ar.B):
            for i in range(ar.n):
                given = i in ar.expect[b] or i in ar.compared[b]
                if self.mode == "alias":
                    out.append(ar.base + ar.off[b][i] if given else 0)
                elif self.raw is not None:
                    out.append(self.base + self.off[b][i] if given else 0)
                else:
                    out.append(0)
        return out

    def wrong(self, image):
        import torch
        if self.raw is None:
            return []
        torch.cuda.synchronize()
        return np.flatnonzero(self.raw.cpu().numpy() != image)[:8].tolist()


def _verdicts(ar, damage, b):
    """By construction: ({offset: shard} for the columns of stripe b in which exactly one expected
    or compared shard is damaged and at least three check rows stand, the offsets of every other
    damaged column)."""
    cols = {}
    for shard, off, _ in damage[b]:
        assert shard in ar.expect[b] or shard in ar.compared[b]
        cols.setdefault(off, set()).add(shard)
    blamed = {off: next(iter(s)) for off, s in cols.items() if len(s) == 1 and len(ar.compared[b]) >= 3}
    for off, s in cols.items():  # what the rule leaves alone for certain: 2..r'-1 errors, or r' < 3
        assert off in blamed or len(ar.compared[b]) < 3 or 2 <= len(s) < len(ar.compared[b])
    return blamed, sorted(set(cols) - set(blamed))


def _truth(ar, damage, b):
    t = ar.ref[b][0].copy()
    for shard, off, val in damage[b]:
        t[shard, off] ^= val
    return t


def _expected(ar, fx, damage, img, fix_img, deliver, store):
    """(arena image, fix image, flagged stripes, counts) after the repair launch of `deliver`: the
    final decode-check launch by DC's rule model, then the repair by construction."""
    want, flagged = ar.after(img, deliver, store, True)
    fix_want = None if fix_img is None else fix_img.copy()
    counts = np.zeros((ar.B, ar.n + 1), dtype=np.uint64)
    hit = []
    for b, S in enumerate(ar.sizes):
        if not ar.in_launch(b, deliver, True):
            continue
        blamed, unexplained = _verdicts(ar, damage, b)
        if blamed or unexplained:
            hit.append(b)
        truth = _truth(ar, damage, b)
        actual, implied, _ = ar.ref[b]
        for w in ar.wanted[b]:
            o = ar.lead + ar.off[b][w]
            row = truth[w].copy()
            row[unexplained] = implied[w][unexplained]
            if not (blamed or unexplained):
                assert np.array_equal(want[o:o + S], row)  # a clean stripe: the check plan's bytes
            want[o:o + S] = row
        counts[b, ar.n] = len(unexplained)
        for off, shard in blamed.items():
            counts[b, shard] += 1
            e = actual[shard][off] ^ truth[shard][off]
            if fx.mode == "alias":
                want[ar.lead + ar.off[b][shard] + off] ^= e
            elif fix_want is not None:
                fix_want[fx.lead + fx.off[b][shard] + off] ^= e
    assert flagged == hit
    return want, fix_want, flagged, counts


def _repair(ar, fx, damage, img, deliver, store, launches=1):
    """Creates the repair plan of `deliver`, launches it and checks every byte, the flags and the
    counts; returns the plan (open) and the arena image."""
    from callfs_amd.device import Plan
    flags, inp, dst, chk = ar.pointers(deliver)
    plan = Plan.decode_repair(ar.k, ar.m, ar.sizes, flags, inp, dst, chk, fx.pointers(), store=store)
    if any(ar.in_launch(b, deliver, True) for b in range(ar.B)):
        assert plan.forms() == ["decode-repair"]
    assert plan.bytes == ar.bytes(deliver, store, True)
    fix_img = None if fx.raw is None else fx.start_img
    want, fix_want, flagged, counts = _expected(ar, fx, damage, img, fix_img, deliver, store)
    for _ in range(launches):
        plan.launch()
    assert ar.wrong(want) == [], (store, fx.mode)
    assert fx.wrong(fix_want) == [], (store, fx.mode)
    assert plan.corrupt_stripes() == flagged
    assert plan.corrupt_stripes() == []  # reported once, then cleared
    got = plan.blame()
    assert np.array_equal(got, counts * np.uint64(launches)), (got.nonzero(), counts.nonzero())
    assert not plan.blame().any()  # read once, then cleared
    return plan, want


def _sets(k, m, batch, ncmp, nwant):
    """Per stripe its own expected set (first k, last k, mixed), and of the other indices ncmp
    compared and nwant wanted ones, which ones rotating with the stripe."""
    expect, wanted, compared = [], [], []
    for b in range(batch):
        e = DC._expected_set(k, m, b)
        rest = [i for i in range(k + m) if i not in e]
        rest = rest[b % len(rest):] + rest[:b % len(rest)]
        expect.append(e)
        compared.append(tuple(sorted(rest[:ncmp])))
        wanted.append(tuple(sorted(rest[ncmp:ncmp + nwant])))
    return tuple(expect), tuple(wanted), tuple(compared)


def _mixed_damage(sets, sizes):
    """Every fourth stripe clean; the others in turn: a byte of an expected shard, a byte of a
    compared shard, two shards in different columns where the stripe has two bytes."""
    expect, wanted, compared = sets
    out = []
    for b, S in enumerate(sizes):
        e, c = expect[b], compared[b]
        if b % 4 == 3:
            out.append(())
        elif b % 4 == 0:
            out.append(((e[(3 + b) % len(e)], S // 2, 0x80 + b),))
        elif b % 4 == 1:
            out.append(((c[b % len(c)], S - 1, 1 + b),))
        else:
            out.append(((e[b % len(e)], 0, 0x11),) + (((c[0], S - 1, 0xfe),) if S > 1 else ()))
    return tuple(out)


@pytest.mark.parametrize("fix", ["null", "zero", "alias"])
@pytest.mark.parametrize("feed", ["store", "singles", "corrupt-first", "corrupt-last"])
@pytest.mark.parametrize("layout", ["aligned", "packed"])
def test_sizes_sets_and_feeds(native_lib, layout, feed, fix):
    """RS(10,4) with three compared rows and one wanted row over the tail-only stripe, one vector,
    vector plus tail, both sides of the tile edge and a tail behind full tiles; every stripe its
    own expected, compared and wanted sets. store: one STORE launch. singles: single-shard
    decode-check merge launches in a shuffled order, the repair plan delivering the last shard.
    corrupt-first / corrupt-last: the damaged shards in the first launch (a decode-check store
    over junk), or in the repair launch itself."""
    k, m = 10, 4
    sets = _sets(k, m, len(SIZES), 3, 1)
    expect, wanted, compared = sets
    damage = _mixed_damage(sets, SIZES)
    ar = DC._Arena(k, m, SIZES, expect, wanted, compared, damage, layout, seed=17,
                   start="zero" if feed == "singles" else "junk")
    fx = _Fix(ar, fix, layout)
    img = ar.start_img
    if feed == "store":
        last, store = ar.everything(), True
    else:
        store = False
        bad = [{s for s, _, _ in damage[b]} for b in range(ar.B)]
        every = ar.everything()
        if feed == "singles":
            items = [("e", j) for j in range(k)] + [("c", j) for j in range(3)]
            order = [int(i) for i in np.random.default_rng(5).permutation(len(items))]
            ds = [ar.deliver([j], []) if t == "e" else ar.deliver([], [j]) for t, j in (items[i] for i in order)]
            launches = [(d, False, False) for d in ds[:-1]]
            last = ds[-1]
        else:
            first = [bad[b] if feed == "corrupt-first" else every[b] - bad[b] for b in range(ar.B)]
            # a clean stripe (and a store over junk needs every stripe): half of its shards
            first = [f if f and f != every[b] else set(sorted(every[b])[::2]) for b, f in enumerate(first)]
            launches = [(first, True, False)]
            last = [every[b] - first[b] for b in range(ar.B)]
        img, none = DC._run(ar, launches)
        assert none == []
    plan, img = _repair(ar, fx, damage, img, last, store)
    plan.close()
    # the clean stripes flagged nothing and counted nothing (checked above); the damaged ones end
    # with the true shard in every wanted row
    for b, S in enumerate(SIZES):
        for w in wanted[b]:
            o = ar.lead + ar.off[b][w]
            assert np.array_equal(img[o:o + S], _truth(ar, damage, b)[w])


@pytest.mark.parametrize("fix", ["null", "zero", "delivered", "alias"])
@pytest.mark.parametrize("where", ["expected", "compared"])
@pytest.mark.parametrize("mode", ["store", "merge"])
def test_one_byte_at_every_edge(native_lib, mode, where, fix):
    """One damaged byte per stripe at the first byte, in wave 1, in wave 3, on both sides of the
    tile edges and in the tail, in an expected or in a compared shard, every fourth stripe clean:
    the wanted row is the true shard, the shard is named, the count is 1."""
    k, m = 10, 4
    B = 10
    sets = _sets(k, m, B, 3, 1)
    expect, wanted, compared = sets
    offs = iter(EDGE_OFFSETS)
    damage = []
    for b in range(B):
        if b % 4 == 3 or b >= 9:
            damage.append(())
            continue
        off = next(offs)
        shard = expect[b][(3 * b) % k] if where == "expected" else compared[b][b % 3]
        damage.append(((shard, off, 0x10 + b),))
    assert next(offs, None) is None
    ar = DC._Arena(k, m, [EDGE_S] * B, expect, wanted, compared, tuple(damage), "packed", seed=23,
                   start="junk" if mode == "store" else "zero")
    fx = _Fix(ar, fix, "packed")
    img = ar.start_img
    if mode == "store":
        last = ar.everything()
    else:
        img, none = DC._run(ar, [(ar.deliver(range(k - 1), [0]), False, False)])
        last = ar.deliver([k - 1], [1, 2])
    plan, img = _repair(ar, fx, tuple(damage), img, last, mode == "store")
    plan.close()


def _edge_case(k, m, nchk, nwant, damage_of, B=4, S=8192 + 16 * 3 + 5, seed=3):
    sets = _sets(k, m, B, nchk, nwant)
    damage = tuple(damage_of(b, sets, S) for b in range(B))
    return sets, damage, S


@pytest.mark.parametrize("mode", ["store", "merge"])
def test_whole_shard_four_shards_and_a_shared_column(native_lib, mode):
    """A wholly corrupt survivor (every byte, vectors and tail); one bad byte on each of four
    different shards in different columns, all four repaired; two shards damaged in the same
    column, unexplained: flagged, counted, the wanted bytes cref.reconstruct's over the damaged
    inputs; and a clean stripe."""
    k, m = 10, 4
    S = 8192 + 16 * 3 + 5
    sets = _sets(k, m, 4, 3, 1)
    expect, wanted, compared = sets
    rng = np.random.default_rng(8)
    whole = tuple((expect[0][4], off, int(v)) for off, v in enumerate(rng.integers(1, 256, S)))
    four = ((expect[1][0], 5, 1), (expect[1][9], 16 * 100 + 15, 2), (compared[1][1], 8192, 3), (compared[1][2], S - 1, 4))
    shared = ((expect[2][2], 777, 0x21), (compared[2][0], 777, 0x42), (expect[2][5], S - 2, 7))
    damage = (whole, four, shared, ())
    ar = DC._Arena(k, m, [S] * 4, expect, wanted, compared, damage, "packed", seed=31,
                   start="junk" if mode == "store" else "zero")
    fx = _Fix(ar, "zero", "packed")
    blamed, unexplained = _verdicts(ar, damage, 2)
    assert unexplained == [777] and len(blamed) == 1
    img = ar.start_img
    if mode == "store":
        last = ar.everything()
    else:
        img, none = DC._run(ar, [(ar.deliver(range(0, k, 2), [1]), False, False)])
        last = ar.deliver(range(1, k, 2), [0, 2])
    plan, img = _repair(ar, fx, damage, img, last, mode == "store")
    plan.close()
    # the unexplained column holds what a reconstruct from the damaged inputs gives, not the truth
    o = ar.lead + ar.off[2][wanted[2][0]] + 777
    assert img[o] == ar.ref[2][1][wanted[2][0]][777] != _truth(ar, damage, 2)[wanted[2][0]][777]


@pytest.mark.parametrize("mode", ["store", "merge"])
@pytest.mark.parametrize("k,m,nchk,nwant", [(10, 8, 4, 4), (20, 12, 3, 9), (10, 20, 8, 8)],
                         ids=["rt8-4+4", "rt16-3+9", "rt16-8+8"])
def test_wider_instances(native_lib, k, m, nchk, nwant, mode):
    """The 8- and 16-row instances: a byte of an expected shard, a byte of a compared shard, a
    whole expected shard, 2 shards in one column (unexplained with four rows or more) and a clean
    stripe; every wanted row repaired."""
    S = 8192 + 16 * 2 + 7
    B = 5
    sets = _sets(k, m, B, nchk, nwant)
    expect, wanted, compared = sets
    rng = np.random.default_rng(k + m)
    whole = tuple((expect[2][k - 1], off, int(v)) for off, v in enumerate(rng.integers(1, 256, S)))
    pair = ((expect[3][1], 8200, 9), (compared[3][0], 8200, 9)) if nchk >= 4 else ((compared[3][1], 8200, 9),)
    damage = (((expect[0][0], 8191, 0x33),), ((compared[1][nchk - 1], S - 1, 0x44),), whole, pair, ())
    ar = DC._Arena(k, m, [S] * B, expect, wanted, compared, damage, "packed", seed=k * m,
                   start="junk" if mode == "store" else "zero")
    fx = _Fix(ar, "zero", "aligned")
    img = ar.start_img
    if mode == "store":
        last = ar.everything()
    else:
        img, none = DC._run(ar, [(ar.deliver(range(k // 2), [0]), False, False)])
        last = ar.deliver(range(k // 2, k), range(1, nchk))
    plan, img = _repair(ar, fx, damage, img, last, mode == "store")
    plan.close()


def test_gate_and_row_limit(native_lib):
    """Two check rows: a damaged stripe is flagged, every damaged column counted as unexplained
    and nothing written beyond the unrepaired wanted rows (fix buffers untouched). 17 rows are
    refused with RS_E_UNSUPPORTED, 16 accepted."""
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    k, m = 10, 4
    S = 8192 + 21
    sets = _sets(k, m, 4, 2, 2)
    expect, wanted, compared = sets
    damage = (((expect[0][1], 100, 5),), ((compared[1][0], S - 1, 6),), (), ((expect[3][2], 16, 1), (expect[3][3], 17, 2)))
    for mode in ("store", "merge"):
        ar = DC._Arena(k, m, [S] * 4, expect, wanted, compared, damage, "aligned", seed=2,
                       start="junk" if mode == "store" else "zero")
        fx = _Fix(ar, "zero", "aligned")
        assert all(not _verdicts(ar, damage, b)[0] for b in range(4))
        img = ar.start_img
        if mode == "merge":
            img, none = DC._run(ar, [(ar.deliver(range(3, k), []), False, False)])
        last = ar.everything() if mode == "store" else ar.deliver(range(3), [0, 1])
        plan, img = _repair(ar, fx, damage, img, last, mode == "store")
        plan.close()
    k, m, n = 10, 20, 30
    e = tuple(range(k))
    ar = DC._Arena(k, m, [64], (e,), (tuple(range(10, 19)),), (tuple(range(19, 27)),), None, "aligned", seed=1)
    flags, inp, dst, chk = ar.pointers(ar.everything())
    with pytest.raises(N.NativeError) as ei:
        Plan.decode_repair(k, m, [64], flags, inp, dst, chk)
    assert ei.value.code == N.RS_E_UNSUPPORTED
    dst[18] = 0  # 8 + 8 rows
    Plan.decode_repair(k, m, [64], flags, inp, dst, chk).close()
    assert ar.wrong(ar.start_img) == []


@pytest.mark.parametrize("k,m", [(1, 3), (3, 2), (4, 2)])
def test_small_profiles(native_lib, k, m):
    """RS(1,3) has three check rows over one expected shard and repairs; RS(3,2) and RS(4,2) have
    at most two and only flag. The first half of the expected shards stored over junk by a
    decode-check plan, the rest and the compared shards with the repair launch."""
    sizes = [17, 8193, 40, 16]
    nchk = min(m, 3)
    sets = _sets(k, m, len(sizes), nchk, m - nchk)
    expect, wanted, compared = sets
    damage = tuple(() if b % 4 == 3 else ((expect[b][b % k], S - 1, 3 + b),) if b % 2 == 0 else
                   ((compared[b][0], 0, 0x80),) for b, S in enumerate(sizes))
    ar = DC._Arena(k, m, sizes, expect, wanted, compared, damage, "packed", seed=100 * k + m, start="junk")
    fx = _Fix(ar, "delivered", "packed")
    half = list(range(max(1, k // 2)))
    img, none = DC._run(ar, [(ar.deliver(half, []), True, False)])
    plan, img = _repair(ar, fx, damage, img, ar.deliver(range(len(half), k), range(nchk)), False)
    plan.close()
    assert any(_verdicts(ar, damage, b)[0] for b in range(len(sizes))) == (nchk >= 3)


def test_wide_lds(native_lib):
    """RS(200,16) with 130 delivered expected shards and 3 compared ones in the repair launch:
    133 * 512 B of tables, past 64 KiB of LDS, 13 wanted rows repaired."""
    k, m = 200, 16
    sizes = [40, 40, 40]
    expect = (tuple(range(k)), tuple(range(16, k + 16)), tuple(range(k)))
    wanted = (tuple(range(k, k + 13)), tuple(range(3, 16)), tuple(range(k, k + 13)))
    compared = (tuple(range(k + 13, k + 16)), (0, 1, 2), tuple(range(k + 13, k + 16)))
    damage = (((150, 39, 0x40),), ((2, 16, 0x07), (100, 3, 0x70)), ())
    ar = DC._Arena(k, m, sizes, expect, wanted, compared, damage, "aligned", seed=9, start="junk")
    fx = _Fix(ar, "zero", "aligned")
    assert (130 + 3) * 512 > 64 << 10
    img, none = DC._run(ar, [(ar.deliver(range(130, 200), []), True, False)])
    plan, img = _repair(ar, fx, damage, img, ar.deliver(range(130), range(3)), False)
    plan.close()


def test_blame_clears_and_doubles(native_lib):
    """A plan with no wanted and no fix rows is idempotent: launched twice before a read, every
    count is doubled, the flags are the same, no byte moves; a read clears."""
    k, m = 10, 4
    sizes = [8192 + 37, 9, 4000, 16]
    expect, _, compared = _sets(k, m, len(sizes), 4, 0)
    wanted = ((),) * len(sizes)
    damage = (((expect[0][0], 8192, 1), (compared[0][3], 36, 2)), ((compared[1][0], 8, 3),), ((expect[2][9], 3999, 4),), ())
    ar = DC._Arena(k, m, sizes, expect, wanted, compared, damage, "packed", seed=12, start="zero")
    fx = _Fix(ar, "null")
    img, none = DC._run(ar, [(ar.deliver(range(k), []), False, False)])
    plan, got = _repair(ar, fx, damage, img, ar.deliver([], range(4)), False, launches=2)
    assert np.array_equal(got, img)
    plan.close()


def test_graph_capture(native_lib):
    """A captured repair launch (no wanted rows, zeroed fix buffers) replayed twice: the second
    replay XORs the error values out again, the counts double."""
    import torch
    from callfs_amd.device import Plan
    k, m = 10, 4
    sizes = [65_541, 9, 8192, 3 * 8192 + 17]
    expect, _, compared = _sets(k, m, len(sizes), 3, 0)
    wanted = ((),) * len(sizes)
    damage = (((expect[0][2], 65_540, 9), (compared[0][1], 8191, 1)), ((expect[1][0], 8, 2),), (), ((compared[3][2], 0, 5),))
    ar = DC._Arena(k, m, sizes, expect, wanted, compared, damage, "aligned", seed=41, start="zero")
    fx = _Fix(ar, "zero", "aligned")
    img, none = DC._run(ar, [(ar.deliver(range(k - 1), [0]), False, False)])
    last = ar.deliver([k - 1], [1, 2])
    want, fix_want, flagged, counts = _expected(ar, fx, damage, img, fx.start_img, last, False)
    assert np.array_equal(want, img) and flagged == [0, 1, 3]
    flags, inp, dst, chk = ar.pointers(last)
    plan = Plan.decode_repair(k, m, sizes, flags, inp, dst, chk, fx.pointers())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside capture
        plan.launch(s)
    torch.cuda.synchronize()
    assert ar.wrong(img) == [] and fx.wrong(fix_want) == []
    assert plan.corrupt_stripes(s) == flagged and np.array_equal(plan.blame(s), counts)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.launch(s)
    assert ar.wrong(img) == [] and fx.wrong(fix_want) == [] and plan.corrupt_stripes(s) == []  # capture runs nothing
    assert not plan.blame(s).any()
    g.replay()
    assert ar.wrong(img) == [] and fx.wrong(fx.start_img) == []  # XOR in place, twice: the error values are out again
    g.replay()
    assert ar.wrong(img) == [] and fx.wrong(fix_want) == []
    assert plan.corrupt_stripes(s) == flagged
    assert np.array_equal(plan.blame(s), counts * np.uint64(2))
    plan.close()


_SLICED_CHILD = r"""
import sys
import numpy as np
import torch
from oracle import cref
from callfs_amd.device import Plan

k, m, n = 2, 4, 6
sizes = [35 * 8192 + b % 17 for b in range(60)] + [8192, 5, 8193, 16]
tiles = sum(max(1, -(-(S // 16) // 512)) for S in sizes)
assert tiles >= 2100 and (tiles // 3) % 35 != 0, tiles   # 3 slices, cut inside stripes
per = -(-tiles // 3)
first = np.cumsum([0] + [max(1, -(-(S // 16) // 512)) for S in sizes])
cuts = {}   # stripe -> the tile of it a slice starts with
for t in (per, 2 * per):
    b = int(np.searchsorted(first, t, side="right")) - 1
    cuts[b] = t - int(first[b])
assert len(cuts) == 2 and all(0 < c < 35 for c in cuts.values()), cuts
rng = np.random.default_rng(3)
dev = torch.device("cuda:0")
keep, ws, flags, inp, dst, chk, want, hit = [], [], [], [], [], [], [], {}
for b, S in enumerate(sizes):
    e = [(0, 1), (1, 5), (0, 4)][b % 3]
    rest = [i for i in range(n) if i not in e]
    w, c = rest[0], rest[1:]
    data = [rng.integers(1, 256, S, dtype=np.uint8) for _ in range(k)]
    full = np.stack(data + cref.encode(data, k, m))
    want.append(full[w].copy())
    if b % 5 == 0 or b in cuts:   # the last byte of one slice and the first of the next, or a byte near the stripe's end
        shard = c[b % 3] if b % 2 else e[0]
        offs = [cuts[b] * 8192 - 1, cuts[b] * 8192] if b in cuts else [S - 1 - (b % 3) * 16]
        for off in offs:
            full[shard, off] ^= 1 + b
        hit[b] = (shard, len(offs))
    t = torch.from_numpy(full).to(dev)
    t[w].fill_(0x5a)
    keep.append(t)
    ws.append(w)
    flags.append([i in e for i in range(n)])
    inp += [t[i].data_ptr() if i != w else 0 for i in range(n)]
    dst += [t[i].data_ptr() if i == w else 0 for i in range(n)]
    chk += [t[i].data_ptr() if i in c else 0 for i in range(n)]   # STORE: the pointer only marks the index
assert all(b in hit for b in cuts)
plan = Plan.decode_repair(k, m, sizes, flags, inp, dst, chk, store=True)
assert plan.forms() == ["decode-repair"], plan.forms()
plan.launch()
got = plan.corrupt_stripes()
counts = plan.blame()
plan.close()
ok = got == sorted(hit) and bool(hit)
for b in range(len(sizes)):
    ok = ok and np.array_equal(keep[b][ws[b]].cpu().numpy(), want[b])
    exp = np.zeros(n + 1, dtype=np.uint64)
    if b in hit:
        exp[hit[b][0]] = hit[b][1]
    ok = ok and np.array_equal(counts[b], exp)
print("sliced decode-repair child:", "ok" if ok else "flagged %r, damaged %r" % (got, hit))
sys.exit(0 if ok else 1)
"""


def test_sliced_grid(native_lib):
    """CALLFS_RS_MAX_TILES_PER_LAUNCH is read once per process: a fresh child runs an RS(2,4)
    batch of at least 2,100 tiles in slices of at most 1,024, with a slice boundary inside a
    damaged stripe; the damaged stripes alone are flagged, blamed on the right shard, and every
    wanted shard is the true one."""
    env = dict(os.environ)
    env["CALLFS_RS_MAX_TILES_PER_LAUNCH"] = "1024"
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    r = subprocess.run([sys.executable, "-c", _SLICED_CHILD], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "sliced decode-repair child: ok" in r.stdout


def test_equivalence_with_a_final_decode_check(native_lib):
    """On clean input the flags (none) and the wanted bytes are those of
    rs_plan_create_decode_check with FINAL over the same buffers, store and merge."""
    import torch
    k, m = 10, 4
    sets = _sets(k, m, len(SIZES), 3, 1)
    expect, wanted, compared = sets
    for store in (True, False):
        ar = DC._Arena(k, m, SIZES, expect, wanted, compared, None, "packed", seed=71, start="junk" if store else "zero")
        img = ar.start_img
        if not store:
            img, none = DC._run(ar, [(ar.deliver(range(1, k), [0, 2]), False, False)])
        last = ar.everything() if store else ar.deliver([0], [1])
        cp = ar.plan(last, store=store, final=True)
        cp.launch()
        assert cp.corrupt_stripes() == []
        theirs = ar.raw.cpu().numpy()
        cp.close()
        assert np.array_equal(theirs, ar.complete(img))
        ar.raw.copy_(torch.from_numpy(img).to(ar.raw.device))
        plan, mine = _repair(ar, _Fix(ar, "null"), ((),) * ar.B, img, last, store)
        plan.close()
        assert np.array_equal(mine, theirs) and ar.wrong(theirs) == []


def test_api_edges(native_lib):
    """The error order the header states, with nothing created; forms, groups, bytes, tuning,
    pinning and ceilings; blame on other plans; the Python mirror's own errors."""
    import torch
    from callfs_amd import _native as N
    from callfs_amd.device import Plan
    k, m, n = 10, 4, 14
    sizes = [8192 + 16 * 3 + 5, 11, 4000, 16]
    B = len(sizes)
    sets = _sets(k, m, B, 3, 1)
    expect, wanted, compared = sets
    ar = DC._Arena(k, m, sizes, expect, wanted, compared, None, "aligned", seed=33, start="junk")
    fx = _Fix(ar, "zero")
    L = N.lib
    ctx = N.default_context()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    deliver = ar.deliver([2, 5], [0])
    flags0, inp0, dst0, chk0 = ar.pointers(deliver)
    fix0 = fx.pointers()
    vp = lambda p: (ctypes.c_void_p * len(p))(*[x or None for x in p])  # noqa: E731
    fl = lambda rows: (ctypes.c_uint8 * (B * n))(*[1 if f else 0 for r in rows for f in r])  # noqa: E731
    sz = lambda v: (ctypes.c_size_t * B)(*v)  # noqa: E731

    def create(kk=k, mm=m, sizes_=sizes, flags=flags0, inp=inp0, dst=dst0, chk=chk0, fix=fix0, bits=0, null=()):
        h = ctypes.c_void_p(0xdead)
        args = {"sizes": sz(sizes_), "expect": fl(flags), "input": vp(inp), "dst": vp(dst), "check": vp(chk),
                "fix": vp(fix)}
        for name in null:
            args[name] = None
        rc = L.rs_plan_create_decode_repair(ctx.handle, 0, kk, mm, B, args["sizes"], args["expect"], args["input"],
                                            args["dst"], args["check"], args["fix"], bits, ctypes.byref(h))
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
    many[3][wanted[3][0]] = True
    in_wanted = list(inp0)
    in_wanted[1 * n + wanted[1][0]] = ar.base
    chk_expected = list(chk0)
    chk_expected[2 * n + expect[2][0]] = ar.base
    fix_wanted = list(fix0)
    fix_wanted[1 * n + wanted[1][0]] = ar.base
    assert create(kk=0, null=("sizes", "input"), bits=4) == N.RS_E_INVALID_PROFILE
    assert create(kk=250, mm=10, flags=few) == N.RS_E_UNSUPPORTED
    for name in ("sizes", "expect", "input", "dst", "check", "fix"):
        assert create(flags=few, null=(name,)) == N.RS_E_ARG, name
    for bits in (2, 3, 4, 1 << 31):  # FINAL is not a flag of this call: the plan is always final
        assert create(flags=few, bits=bits) == N.RS_E_ARG
    assert create(flags=few, inp=in_wanted, sizes_=zero) == N.RS_E_TOO_FEW_SHARDS
    assert create(flags=many, sizes_=zero) == N.RS_E_ARG
    for bits in (0, 1):
        assert create(inp=in_wanted, sizes_=zero, bits=bits) == N.RS_E_ARG
        assert create(chk=chk_expected, sizes_=zero, bits=bits) == N.RS_E_ARG
        assert create(fix=fix_wanted, sizes_=zero, bits=bits) == N.RS_E_ARG
        assert create(sizes_=zero, bits=bits) == N.RS_E_NO_DATA
        assert create(bits=bits) == N.RS_OK
    with pytest.raises(ValueError):
        Plan.decode_repair(k, m, sizes, flags0[:3], inp0, dst0, chk0)
    with pytest.raises(ValueError):
        Plan.decode_repair(k, m, sizes, flags0, inp0, dst0, chk0, fix0[:-1])
    # the other constructors refuse what they refused
    h = ctypes.c_void_p()
    assert L.rs_plan_create_decode_check(ctx.handle, 0, k, m, B, sz(sizes), fl(flags0), vp(inp0), vp(dst0), vp(chk0), 4,
                                         ctypes.byref(h)) == N.RS_E_ARG
    assert L.rs_plan_create_decode_idx(ctx.handle, 0, k, m, B, sz(sizes), fl(flags0), vp([0] * (B * n)), vp(dst0), 2,
                                       ctypes.byref(h)) == N.RS_E_ARG
    seen = set()
    for store in (False, True):
        plan = Plan.decode_repair(k, m, sizes, flags0, inp0, dst0, chk0, fix0, store=store)
        assert int(L.rs_plan_groups(plan.handle)) == 1
        forms = (ctypes.c_int * 1)()
        assert L.rs_plan_forms(plan.handle, forms, 1) == 1
        assert forms[0] == N.RS_ORDER_DECODE_REPAIR == 131072 and plan.forms() == ["decode-repair"]
        assert plan.bytes == ar.bytes(deliver, store, True)
        seen.add(plan.bytes)
        assert plan.tune() == ["none"]
        with pytest.raises(N.NativeError) as ei:
            plan.set_orders(["consecutive"])
        assert ei.value.code == N.RS_E_ARG
        plan.set_orders(["none"])
        for mode in (1, 2):
            assert L.rs_plan_launch_ceiling(plan.handle, s, mode) == N.RS_E_ARG
        assert ar.wrong(ar.start_img) == [] and not plan.corrupt() and not plan.blame().any()
        plan.close()
    assert len(seen) == 2
    # rs_plan_blame still refuses a plan without counts
    cp = ar.plan(deliver, final=True)
    with pytest.raises(N.NativeError) as ei:
        cp.blame()
    assert ei.value.code == N.RS_E_ARG
    cp.close()
    # a timed launch brackets the kernel
    plan = Plan.decode_repair(k, m, sizes, *ar.pointers(ar.everything())[:4], fix0, store=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    plan.launch(events=(e0, e1))
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) > 0
    assert ar.wrong(ar.complete(ar.start_img)) == [] and fx.wrong(fx.start_img) == [] and not plan.corrupt()
    plan.close()
