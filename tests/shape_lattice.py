"""Helpers of tests/test_gpu_shape_lattice.py (a plain module, imported by the test module and by
the child process of its wide-LDS cases): one sentinel-guarded arena and one runner per plan kind
of the tile-map kernels. A runner builds the buffers of one plan in the packed (odd-offset) layout,
computes the image the launch must leave with oracle.cref alone, asserts on the CPU that every
written row's expected bytes differ from its starting bytes, asserts the plan's kernel forms and
launch groups, launches and compares the whole allocation -- guards and gaps included -- with the
expected image. Nothing here has a tolerance."""
import functools

import numpy as np

from oracle import cref

SENTINEL = 0x5A
GUARD = 4096
# per stripe: tail only; one vector and no tail; two vectors and 8 tail bytes; one full 512-vector
# tile, one lane of a second tile and 3 tail bytes
SIZES = (5, 16, 40, 8211)


def cycle_sizes(batch, first=0):
    return [SIZES[(first + b) % len(SIZES)] for b in range(batch)]


def two_cols(S):
    """Two byte columns of a shard of S bytes: one in the vector body and one in the S % 16 tail
    where the size has both, for 8211 the vector in the second tile."""
    return {5: (1, 3), 16: (2, 9), 40: (17, 35), 8211: (8192 + 3, 8209)}[S]


def third_col(S, b):
    """A column two_cols(S) does not use; in the tail for odd b where the size has one."""
    return {5: (4, 0), 16: (13, 6), 40: (3, 38), 8211: (4000, 8210)}[S][b % 2]


class Arena:
    """A sentinel-filled device allocation: buffers at odd offsets with sentinel gaps between them
    (take), 4 KiB guards before and behind. `start` is the host image of the body; upload() puts an
    image on the device, wrong() lists the first offsets at which the whole allocation differs from
    the guards around an expected body."""

    def __init__(self):
        self.spans = []
        self._off = 0

    def take(self, S):
        self._off += 16
        self._off = (self._off + 2 * (len(self.spans) % 7)) | 1
        o = self._off
        self.spans.append((o, S))
        self._off += S
        return o

    def seal(self):
        import torch
        assert all(o % 2 == 1 for o, _ in self.spans)
        self.nbytes = self._off + 16
        self.start = np.full(self.nbytes, SENTINEL, dtype=np.uint8)
        self.raw = torch.full((self.nbytes + 2 * GUARD + 256,), SENTINEL, dtype=torch.uint8,
                              device=torch.device("cuda:0"))
        self.lead = GUARD + (-(self.raw.data_ptr() + GUARD) % 256)
        self.base = self.raw.data_ptr() + self.lead

    def ptr(self, o):
        return 0 if o is None else self.base + o

    def upload(self, body):
        import torch
        assert body.shape == (self.nbytes,) and body.dtype == np.uint8
        self.raw[self.lead:self.lead + self.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(body)))
        torch.cuda.synchronize()

    def wrong(self, body):
        import torch
        torch.cuda.synchronize()
        got = self.raw.cpu().numpy()
        want = np.full(got.size, SENTINEL, dtype=np.uint8)
        want[self.lead:self.lead + self.nbytes] = body
        return (np.flatnonzero(got != want)[:8] - self.lead).tolist()


def put(img, o, row):
    img[o:o + len(row)] = row


def get(img, o, S):
    return img[o:o + S]


def check_plan(plan, form, rows):
    """The plan runs `form` in ceil(rows / 16) launch groups."""
    from callfs_amd import _native as N
    groups = (rows + 15) // 16
    assert int(N.lib.rs_plan_groups(plan.handle)) == groups, (int(N.lib.rs_plan_groups(plan.handle)), groups)
    assert plan.forms() == [form] * groups, (plan.forms(), form, groups)


def codeword(k, m, S, rng):
    """[k + m][S]: random data and the oracle's parity."""
    st = np.empty((k + m, S), dtype=np.uint8)
    st[:k] = rng.integers(0, 256, (k, S), dtype=np.uint8)
    par = cref.encode([st[i] for i in range(k)], k, m)
    for j in range(m):
        st[k + j] = par[j]
    return st


@functools.lru_cache(maxsize=None)
def coef(k, m, expect):
    """C as an (n, k) array: row w, column j = the coefficient of expected shard expect[j] in shard
    w; cref.reconstruct of the k unit vectors."""
    n = k + m
    shards = [None] * n
    for j, v in enumerate(expect):
        shards[v] = np.zeros(k, dtype=np.uint8)
        shards[v][j] = 1
    C = np.stack(cref.reconstruct(shards, [i in expect for i in range(n)], k, m))
    C.setflags(write=False)
    return C


def apply_rows(C, rows, pos, inputs, S):
    """cref.apply(C[rows][:, pos], inputs) as a {row: bytes} dict; zeros when there is no input."""
    if not rows:
        return {}
    if not pos:
        return {r: np.zeros(S, dtype=np.uint8) for r in rows}
    return dict(zip(rows, cref.apply(C[list(rows)][:, list(pos)], inputs)))


def mask_of(n, lost):
    lost = set(lost)
    return [i not in lost for i in range(n)]


# ---- mixed, ragged, required -----------------------------------------------------------------

def run_rebuild(kind, k, m, sizes, masks, wanted=None, seed=1):
    """kind "mixed" (one size), "ragged" or "required" (wanted: per stripe the lost shards to
    rebuild). The lost shards start as the sentinel. One clean launch: the written shards hold
    cref.reconstruct's bytes, everything else is what it was, nothing is flagged. Then, when a
    stripe compares a shard, one launch per flipped byte (one in the vector body, one in the tail,
    in different stripes where there are two) over the starting image: exactly that stripe is
    flagged and the image is the clean launch's but for the flipped byte."""
    from callfs_amd.device import Plan
    n, B = k + m, len(sizes)
    assert (kind == "required") == (wanted is not None) and len(masks) == B
    assert kind != "mixed" or len(set(sizes)) == 1
    rng = np.random.default_rng(seed)
    ar = Arena()
    off = [[ar.take(S) for _ in range(n)] for S in sizes]
    ar.seal()
    start = ar.start
    written, compared = [], []
    for b, (S, mask) in enumerate(zip(sizes, masks)):
        st = codeword(k, m, S, rng)
        present = [i for i in range(n) if mask[i]]
        assert len(present) >= k
        for i in present:
            put(start, off[b][i], st[i])
        written.append([i for i in range(n) if not mask[i] and (wanted is None or wanted[b][i])])
        compared.append(present[k:])
    want = start.copy()
    for b, (S, mask) in enumerate(zip(sizes, masks)):
        if not written[b]:
            continue
        full = cref.reconstruct([get(start, off[b][i], S).copy() if mask[i] else None for i in range(n)],
                                mask, k, m)
        for i in written[b]:
            assert not np.array_equal(np.asarray(full[i]), get(start, off[b][i], S)), (b, i)
            put(want, off[b][i], np.asarray(full[i]))
    rows = max(len(w) + len(c) for w, c in zip(written, compared))
    assert kind == "required" or rows == m
    ptrs = [ar.ptr(o) for row in off for o in row]
    if kind == "mixed":
        plan = Plan(k, m, sizes[0], B, ptrs, present=masks)
    else:
        plan = Plan.ragged(k, m, sizes, ptrs, present=masks, required=wanted)
    check_plan(plan, kind, rows)
    ar.upload(start)
    plan.launch()
    assert ar.wrong(want) == [], (kind, k, m, "clean")
    assert plan.corrupt_stripes() == []
    # one flipped byte of one compared shard
    cands = [b for b in range(B) if compared[b]]
    flips = [(b, compared[b][(seed + which) % len(compared[b])], two_cols(sizes[b])[which])
             for which, b in enumerate((cands[0], cands[-1]) if cands else ())]
    for b, i, col in flips:
        s2, w2 = start.copy(), want.copy()
        s2[off[b][i] + col] ^= 0x40
        w2[off[b][i] + col] ^= 0x40
        ar.upload(s2)
        plan.launch()
        assert plan.corrupt_stripes() == [b], (kind, k, m, b, i, col)
        assert ar.wrong(w2) == [], (kind, k, m, "flipped", b, i, col)
    plan.close()
    return len(flips)


def lattice_masks(k, m, batch, seed):
    """Per stripe its own mask: stripe 0 an encode (every parity shard lost, nothing compared), then
    1, 2, m // 2 and no shards lost, seeded."""
    n = k + m
    rng = np.random.default_rng(seed)
    masks = [mask_of(n, range(k, n))]
    for b in range(1, batch):
        lose = (m, 1, min(2, m), max(1, m // 2), 0)[b % 5]
        masks.append(mask_of(n, (int(i) for i in rng.choice(n, size=lose, replace=False))))
    return masks


def required_sets(k, m, seed, narrow=()):
    """Masks and wanted sets of a required plan whose widest stripe has m rows: stripe 0 loses every
    parity shard and wants them all; stripe 1 loses m shards and wants one; stripe 2 loses m // 2
    and wants none (compared rows alone); stripe 3 loses one and wants it (m rows); then one stripe
    per entry of `narrow` that loses m shards and wants that many."""
    n = k + m
    rng = np.random.default_rng(seed)

    def lose(c):
        return sorted(int(i) for i in rng.choice(n, size=c, replace=False))

    sets = [(list(range(k, n)), m), (lose(m), 1), (lose(max(1, m // 2)), 0), (lose(1), 1)]
    sets += [(lose(m), w) for w in narrow if w <= m]
    masks = [mask_of(n, lost) for lost, _ in sets]
    wanted = [[i in lost[:w] for i in range(n)] for lost, w in sets]
    return masks, wanted


# ---- update ----------------------------------------------------------------------------------

def run_update(k, m, sizes, changed, pair, seed=1):
    """Update (pair) or EncodeIdx (single) plans: parity ^= P[:, changed] * (old ^ new). The
    expected parity is cref.encode of the new data (pair), or the random starting parity XOR
    cref.apply(P[:, changed], new shards). A second launch restores the starting image."""
    from callfs_amd.device import Plan
    B = len(sizes)
    rng = np.random.default_rng(seed)
    E = cref.encode_matrix(k, m)
    ar = Arena()
    old_off = [[ar.take(S) if pair and i in ch else None for i in range(k)] for S, ch in zip(sizes, changed)]
    new_off = [[ar.take(S) if i in ch else None for i in range(k)] for S, ch in zip(sizes, changed)]
    par_off = [[ar.take(S) for _ in range(m)] for S in sizes]
    ar.seal()
    start = ar.start
    exp = []
    for b, (S, ch) in enumerate(zip(sizes, changed)):
        ch = sorted(ch)
        old = rng.integers(0, 256, (k, S), dtype=np.uint8)
        new = old.copy()
        for i in ch:
            new[i] = rng.integers(0, 256, S, dtype=np.uint8)
            new[i][0] = old[i][0] ^ 0x80
            put(start, new_off[b][i], new[i])
            if pair:
                put(start, old_off[b][i], old[i])
        if pair:
            par0 = np.stack(cref.encode(list(old), k, m))
            after = np.stack(cref.encode(list(new), k, m)) if ch else par0
        else:
            par0 = rng.integers(0, 256, (m, S), dtype=np.uint8)
            after = par0 ^ np.stack(cref.apply(E[k:, ch], [new[i] for i in ch])) if ch else par0
        for j in range(m):
            put(start, par_off[b][j], par0[j])
            assert not ch or not np.array_equal(after[j], par0[j]), (b, j)
        exp.append(after)
    want = start.copy()
    for b in range(B):
        for j in range(m):
            put(want, par_off[b][j], exp[b][j])
    flags = [[i in ch for i in range(k)] for ch in changed]
    old_ptrs = [ar.ptr(o) for row in old_off for o in row] if pair else None
    plan = Plan.update(k, m, sizes, flags, old_ptrs, [ar.ptr(o) for row in new_off for o in row],
                       [ar.ptr(o) for row in par_off for o in row])
    check_plan(plan, "update", m if any(changed) else 0)
    ar.upload(start)
    plan.launch()
    assert ar.wrong(want) == [], ("update", pair, k, m)
    assert not plan.corrupt()
    plan.launch()
    assert ar.wrong(start) == [], ("update twice", pair, k, m)
    plan.close()


def pick_sets(k, counts, seed):
    """Per count c a seeded sorted c-subset of range(k)."""
    rng = np.random.default_rng(seed)
    return [tuple(sorted(int(i) for i in rng.choice(k, size=c, replace=False))) for c in counts]


# ---- decode-idx ------------------------------------------------------------------------------

def expected_set(k, m, kind):
    """k of the k+m indices: the first k, the last k, or a set that mixes data and parity."""
    n = k + m
    if kind % 3 == 0:
        return tuple(range(k))
    if kind % 3 == 1:
        return tuple(range(n - k, n))
    return tuple(sorted(set(range(n)) - set(range(1, 1 + m))))


def run_decode_idx(k, m, sizes, expect, wanted, feeds, store, seed=1):
    """feeds[b]: the positions in expect[b] delivered. Wanted rows start as random bytes; a launch
    leaves start ^ terms there (merge) or the terms (store), terms = cref.apply(C[wanted][:, feed],
    inputs)."""
    from callfs_amd.device import Plan
    n, B = k + m, len(sizes)
    rng = np.random.default_rng(seed)
    ar = Arena()
    off = [[ar.take(S) for _ in range(n)] for S in sizes]
    ar.seal()
    start = ar.start
    terms = []
    for b, S in enumerate(sizes):
        data = rng.integers(0, 256, (k, S), dtype=np.uint8)
        for i in range(n):
            put(start, off[b][i], data[expect[b].index(i)] if i in expect[b]
                else rng.integers(0, 256, S, dtype=np.uint8))
        terms.append(apply_rows(coef(k, m, expect[b]), list(wanted[b]), list(feeds[b]),
                                [data[j] for j in feeds[b]], S))
    want = start.copy()
    rows = 0
    for b, S in enumerate(sizes):
        if not feeds[b] or not wanted[b]:
            continue
        rows = max(rows, len(wanted[b]))
        for w in wanted[b]:
            new = terms[b][w] if store else get(start, off[b][w], S) ^ terms[b][w]
            assert not np.array_equal(new, get(start, off[b][w], S)), (b, w)
            put(want, off[b][w], new)
    inp, dst, flags = [], [], []
    for b in range(B):
        deliver = {expect[b][j] for j in feeds[b]}
        inp += [ar.ptr(off[b][i]) if i in deliver else 0 for i in range(n)]
        dst += [ar.ptr(off[b][i]) if i in wanted[b] else 0 for i in range(n)]
        flags.append([i in expect[b] for i in range(n)])
    plan = Plan.decode_idx(k, m, sizes, flags, inp, dst, store=store)
    check_plan(plan, "decode-idx", rows)
    ar.upload(start)
    plan.launch()
    assert ar.wrong(want) == [], ("decode-idx", store, k, m)
    assert not plan.corrupt()
    plan.close()


# ---- final decode-check ----------------------------------------------------------------------

def run_decode_check(k, m, sizes, expect, wanted, compared, feeds, store, damage=None, seed=1, scan_only=()):
    """A final decode-check launch. feeds[b]: the positions in expect[b] delivered with it.
    merge: the compared shards are not delivered and every accumulator starts as the oracle's
    C[j][feed] * inputs, so a clean stripe's check value is zero everywhere; wanted rows start as
    random bytes and become start ^ terms. store: the compared shards are delivered too (the source
    count is len(feeds[b]) + len(compared[b])) and hold the oracle's C[j][feed] * inputs, so again
    a clean stripe's value is zero; the accumulators hold junk that is never read; wanted rows become
    the terms. scan_only: stripes that are delivered nothing at all, compared shards included (their
    accumulators, under store not even those, are all the launch looks at). damage[b]: None, or 0 / 1 for one flipped byte in the vector body / in the tail
    (two_cols) of a check row's accumulator (merge) or compared shard (store). The flagged stripes,
    by the rule over the buffers as they are, must be the damaged ones; the image changes in the
    wanted rows alone."""
    from callfs_amd.device import Plan
    n, B = k + m, len(sizes)
    damage = damage if damage is not None else [None] * B
    rng = np.random.default_rng(seed)
    ar = Arena()
    off = [[ar.take(S) for _ in range(n)] for S in sizes]
    acc = [{j: ar.take(S) for j in compared[b]} for b, S in enumerate(sizes)]
    ar.seal()
    start = ar.start
    datas = []
    for b, S in enumerate(sizes):
        assert not set(wanted[b]) & set(compared[b]) and not (set(wanted[b]) | set(compared[b])) & set(expect[b])
        data = rng.integers(0, 256, (k, S), dtype=np.uint8)
        datas.append(data)
        for i in range(n):
            put(start, off[b][i], data[expect[b].index(i)] if i in expect[b]
                else rng.integers(0, 256, S, dtype=np.uint8))
        part = apply_rows(coef(k, m, expect[b]), list(compared[b]), list(feeds[b]),
                          [data[j] for j in feeds[b]], S)
        for j in compared[b]:
            put(start, acc[b][j], rng.integers(0, 256, S, dtype=np.uint8) if store else part[j])
            if store and b not in scan_only:
                put(start, off[b][j], part[j])
        if damage[b] is not None:
            assert not (store and b in scan_only)
            j = compared[b][(seed + b) % len(compared[b])]
            start[(off[b][j] if store else acc[b][j]) + two_cols(S)[damage[b]]] ^= 0x21
    # the rule, over the buffers as they are
    want = start.copy()
    flagged, rows = [], 0
    for b, S in enumerate(sizes):
        if not compared[b] and not (feeds[b] and wanted[b]):
            continue  # not in the launch
        rows = max(rows, len(wanted[b]) + len(compared[b]))
        C = coef(k, m, expect[b])
        ins = [get(start, off[b][expect[b][j]], S) for j in feeds[b]]
        t = apply_rows(C, sorted(set(wanted[b]) | set(compared[b])), list(feeds[b]), ins, S)
        for w in wanted[b]:
            new = t[w] if store else get(start, off[b][w], S) ^ t[w]
            assert not np.array_equal(new, get(start, off[b][w], S)), (b, w)
            put(want, off[b][w], new)
        bad = False
        for j in compared[b]:
            value = t[j]
            if not store:
                value = value ^ get(start, acc[b][j], S)
            elif b not in scan_only:
                value = value ^ get(start, off[b][j], S)
            bad |= bool(value.any())
        if bad:
            flagged.append(b)
    assert flagged == [b for b in range(B) if damage[b] is not None], (flagged, damage)
    inp, dst, chk, flags = [], [], [], []
    for b in range(B):
        assert b not in scan_only or not feeds[b]
        deliver = {expect[b][j] for j in feeds[b]} | (set(compared[b]) if store and b not in scan_only else set())
        inp += [ar.ptr(off[b][i]) if i in deliver else 0 for i in range(n)]
        dst += [ar.ptr(off[b][i]) if i in wanted[b] else 0 for i in range(n)]
        chk += [ar.ptr(acc[b][i]) if i in compared[b] else 0 for i in range(n)]
        flags.append([i in expect[b] for i in range(n)])
    plan = Plan.decode_check(k, m, sizes, flags, inp, dst, chk, store=store, final=True)
    check_plan(plan, "decode-check", rows)
    ar.upload(start)
    plan.launch()
    assert ar.wrong(want) == [], ("decode-check", store, k, m)
    assert plan.corrupt_stripes() == flagged, ("decode-check", store, k, m)
    assert plan.corrupt_stripes() == []
    plan.close()


# ---- locate, locate2, correct ----------------------------------------------------------------

def examined(k, mask):
    """(valid, cmp): the first k present shards and the next min(present - k, 16)."""
    present = [i for i, p in enumerate(mask) if p]
    return present[:k], present[k:k + 16]


def stripe_hits(kind, k, mask, S, b, rng):
    """The shared hit setup of one stripe: {shard: [column, ...]}. One column on a valid shard (found
    through the ratio table) and one on a compared shard (the nz == 1 path), one of them in the
    vector body and one in the tail where the size has both; for locate2, where r' >= 3, a third
    column hit in a valid and a compared shard at once."""
    valid, cmp_ = examined(k, mask)
    if not cmp_:
        return {}
    cols = two_cols(S)
    d = valid[int(rng.integers(0, len(valid)))]
    c = cmp_[int(rng.integers(0, len(cmp_)))]
    hits = {d: [cols[b % 2]], c: [cols[1 - b % 2]]}
    if kind == "locate2" and len(cmp_) >= 3:
        d2 = valid[int(rng.integers(0, len(valid)))]
        c2 = cmp_[int(rng.integers(0, len(cmp_)))]
        for i in (d2, c2):
            hits.setdefault(i, []).append(third_col(S, b))
    return hits


def locate_expected(kind, k, n, mask, hits):
    """(counts [n + 1], the (shard, column) bytes a correct plan restores) from the hits alone."""
    valid, cmp_ = examined(k, mask)
    exp = np.zeros(n + 1, dtype=np.uint64)
    restored = []
    r = len(cmp_)
    per_col = {}
    for i, cols in hits.items():
        if i in valid + cmp_:
            for c in cols:
                per_col.setdefault(c, []).append(i)
    for c, shards in per_col.items():
        e = len(shards)
        if kind == "correct":
            assert e == 1
            if r >= 3:
                exp[shards[0]] += 1
                restored.append((shards[0], c))
            else:
                exp[n] += 1
        elif r == 1:
            exp[n] += 1
        elif e == 1:
            exp[shards[0]] += 1
        elif e == 2 and r >= 4 and kind == "locate2":
            exp[shards[0]] += 1
            exp[shards[1]] += 1
        else:
            assert e <= (r - 2 if r >= 4 and kind == "locate2" else r - 1), "the rule promises nothing here"
            exp[n] += 1
    return exp, restored


def run_locate(kind, k, m, sizes, masks, hits, rows, seed=1):
    """kind "locate", "locate2" or "correct"; hits[b] = {shard: columns}, each hit byte XORed with
    a nonzero value. Counts and flagged stripes are derived from the hits alone; locate plans leave
    the whole allocation as it was, a correct plan leaves the pristine bytes where it repairs and
    the damaged ones elsewhere. `rows`: the widest stripe's compared shards (at most 16)."""
    from callfs_amd.device import Plan
    n, B = k + m, len(sizes)
    rng = np.random.default_rng(seed)
    ar = Arena()
    off = [[ar.take(S) for _ in range(n)] for S in sizes]
    ar.seal()
    clean = ar.start
    for b, S in enumerate(sizes):
        st = codeword(k, m, S, rng)
        for i in range(n):
            put(clean, off[b][i], st[i] if masks[b][i] else rng.integers(0, 256, S, dtype=np.uint8))
    damaged = clean.copy()
    exp = np.zeros((B, n + 1), dtype=np.uint64)
    fixes = []
    for b in range(B):
        for i, cols in hits[b].items():
            assert masks[b][i] and len(set(cols)) == len(cols)
            for c in cols:
                assert 0 <= c < sizes[b]
                damaged[off[b][i] + c] ^= int(rng.integers(1, 256))
        exp[b], restored = locate_expected(kind, k, n, masks[b], hits[b])
        fixes += [(b, i, c) for i, c in restored]
    want = damaged.copy()
    for b, i, c in fixes:
        want[off[b][i] + c] = clean[off[b][i] + c]
    assert kind != "correct" or not fixes or not np.array_equal(want, damaged)
    assert max(len(examined(k, mk)[1]) for mk in masks) == rows
    ptrs = [ar.ptr(o) for row in off for o in row]
    if kind == "correct":
        plan = Plan.correct(k, m, sizes, ptrs, present=masks)
    else:
        plan = Plan.locate(k, m, sizes, ptrs, present=masks, max_errors=2 if kind == "locate2" else 1)
    check_plan(plan, "correct" if kind == "correct" else "locate", min(rows, 16))
    ar.upload(damaged)
    plan.launch()
    flagged = plan.corrupt_stripes()
    counts = plan.blame()
    assert ar.wrong(want) == [], (kind, k, m)
    bad = np.argwhere(counts != exp)[:6].tolist()
    assert not bad, (kind, k, m, [(b, i, int(counts[b, i]), int(exp[b, i])) for b, i in bad])
    assert flagged == [b for b in range(B) if exp[b].any()], (kind, k, m, flagged)
    plan.close()
    return exp


def locate_masks(k, m, rprimes):
    """Per r' a stripe that keeps every data shard and r' parity shards: the last r' for odd r',
    the first r' for even, so compared shard x is not always shard k + x."""
    n = k + m
    masks = []
    for r in rprimes:
        assert 1 <= r <= m
        lost = range(k, k + m - r) if r % 2 else range(k + r, n)
        masks.append(mask_of(n, lost))
    return masks


def run_locate_profile(kind, k, m, seed=1, extra_clean=True):
    """One plan of RS(k, m): a stripe per r' in {1, 2, 3, 4, 5, 8, 9, 16} that m allows, m itself
    first, each with the shared hit setup, and a clean stripe that nothing may flag."""
    top = min(m, 16)
    rps = [top] + [r for r in (1, 2, 3, 4, 5, 8, 9, 16) if r < top]
    masks = locate_masks(k, m, [min(r, m) for r in rps])
    if m > 16:
        masks[0] = mask_of(k + m, ())  # everything present: 16 of the m compared shards examined
    if extra_clean:
        masks.append(list(masks[0]))
    sizes = cycle_sizes(len(masks), first=seed)
    rng = np.random.default_rng(seed + 77)
    hits = [stripe_hits(kind, k, mk, S, b, rng) for b, (mk, S) in enumerate(zip(masks, sizes))]
    if extra_clean:
        hits[-1] = {}
    return run_locate(kind, k, m, sizes, masks, hits, top, seed)


# ---- the wide-LDS child ----------------------------------------------------------------------

WIDE_PROFILES = ((20, 16), (128, 16), (129, 9), (240, 16), (20, 16))
WIDE_KINDS = ("mixed", "ragged", "required", "update-single", "locate", "locate2", "correct")
WIDE_SIZES = (40, 8211)
_WIDE_COLS = {40: (1, 17, 20, 33, 35, 38), 8211: (5, 100, 8190, 8195, 8209, 8210)}
_WIDE_PAIR_COL = {40: 25, 8211: 4000}


def run_wide(kind, k, m, seed):
    """One launch group of `kind` over RS(k, m) with 16-byte table entries (m > 8) and every one of
    the k inputs staged: k * 512 bytes of dynamic LDS, at sizes 40 and 8211."""
    n = k + m
    sizes = list(WIDE_SIZES)
    if kind in ("mixed", "ragged"):
        masks = [mask_of(n, range(k, n)), mask_of(n, (0, k - 1))]
        if kind == "ragged":
            run_rebuild("ragged", k, m, sizes, masks, seed=seed)
        else:
            for S in sizes:
                run_rebuild("mixed", k, m, [S, S], masks, seed=seed + S)
    elif kind == "required":
        masks = [mask_of(n, range(k, n)), mask_of(n, (0, k - 1))]
        wanted = [[i >= k for i in range(n)], [i == k - 1 for i in range(n)]]
        run_rebuild("required", k, m, sizes, masks, wanted, seed=seed)
    elif kind == "update-single":
        run_update(k, m, sizes, [tuple(range(k)), (k - 1,)], pair=False, seed=seed)
    else:
        masks = [mask_of(n, ())] * 2  # everything present: k + min(m, 16) examined shards
        top = min(m, 16)
        if kind == "correct":
            shards = [s for s in (255, 200) if s < k + top] or [k + top - 1, k // 2]
        else:
            shards = sorted({s for s in (0, 127, 128, 239, 240, 255, k - 1, k, k + top - 1) if s < k + top})[:6]
        hits = []
        for S in sizes:
            h = {s: [_WIDE_COLS[S][q]] for q, s in enumerate(shards)}
            if kind == "locate2":
                for s in ((239, 255) if k + top == 256 else (k - 1, k + top - 1)):
                    h.setdefault(s, []).append(_WIDE_PAIR_COL[S])
            hits.append(h)
        exp = run_locate(kind, k, m, sizes, masks, hits, top, seed)
        assert int(exp.sum()) == 2 * len(shards) + (4 if kind == "locate2" else 0)


def wide_child():
    """Every kind, one after the other, through WIDE_PROFILES in order (the opt-in is set once per
    process, device and kind: the order of launches is the test). Prints one JSON line: per kind the
    profiles that passed and the first failure. A failure that is no plain mismatch -- a HIP error
    among them -- ends the run: nothing further is launched."""
    import json
    import traceback
    from callfs_amd import _native as N
    N.lib.rs_tune_table_reset(None)
    out = {}
    fatal = False
    for kind in WIDE_KINDS:
        res = out[kind] = {"passed": [], "error": None}
        if fatal:
            res["error"] = "not run: an earlier launch failed"
            continue
        for step, (k, m) in enumerate(WIDE_PROFILES):
            try:
                run_wide(kind, k, m, seed=100 * step + k)
                res["passed"].append([k, m])
            except AssertionError:
                res["error"] = "RS(%d,%d) step %d: %s" % (k, m, step, traceback.format_exc()[-1500:])
                break
            except Exception:
                res["error"] = "RS(%d,%d) step %d (fatal): %s" % (k, m, step, traceback.format_exc()[-1500:])
                fatal = True
                break
    print("WIDE_LDS_RESULT " + json.dumps(out))
    return 1 if fatal else 0
