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

    def layout(self):
        """Closes the layout and makes the host image `start`; needs no device."""
        assert all(o % 2 == 1 for o, _ in self.spans)
        self.nbytes = self._off + 16
        self.start = np.full(self.nbytes, SENTINEL, dtype=np.uint8)

    def seal(self):
        """layout(), unless it was called already, and the device allocation."""
        import torch
        if not hasattr(self, "start"):
            self.layout()
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


# ---- decode-repair ---------------------------------------------------------------------------

def narrow_rows(m):
    """Row counts below m for the stripes that run in a wider instance than they need: 1 and 9
    beside 16, 5 beside 8."""
    return [w for w in (1, 9, 5, 13, 2, 7) if w < m]


def repair_stripe(S, expect, compared, wanted, feeds, cmp_fed=None, damage=(), fix=None):
    """One stripe of a decode-repair plan. feeds: the positions in `expect` delivered with the
    launch; cmp_fed: the compared shards delivered with it (None: all of them under store, none
    under merge); damage: (shard, column, value) triples on expected or compared shards; fix: a
    {shard: mode} dict, or one mode for every expected and compared shard: None (a null pointer),
    "zero" (a zeroed buffer of its own) or "alias" (the shard's own buffer)."""
    if not isinstance(fix, dict):
        fix = {i: fix for i in tuple(expect) + tuple(compared)}
    return dict(S=S, expect=tuple(expect), compared=tuple(compared), wanted=tuple(wanted),
                feeds=tuple(sorted(feeds)), cmp_fed=None if cmp_fed is None else tuple(cmp_fed),
                damage=tuple(damage), fix=fix)


class RepairModel:
    """What one decode-repair launch must do, from oracle.cref and the construction alone; needs no
    device. Per stripe a true codeword (cref.apply of the oracle's coefficients over random data;
    under store the data is zero at the positions that are not fed, so the launch is a complete
    decode), the shards as delivered (the damage XORed in), and the state earlier launches would
    have left: under merge the accumulators and wanted rows hold cref.apply of the not-fed expected
    shards as delivered, the accumulators also the compared shards that do not come with this
    launch; under store both hold junk. A damaged column is blamed (one damaged shard, three check
    rows or more) or unexplained (fewer than three check rows, or 2 <= damaged shards < r'); any
    other column is refused. The expected image: wanted rows are the true shards, in unexplained
    columns cref.apply over the damaged expected shards; a zeroed fix buffer ends as the error row
    of its shard's blamed columns, an aliased shard ends restored there; nothing else moves.

    start, want: the arena's images; counts [B][n + 1], flagged; rows: the widest stripe's row
    count; srcs[b], nrows[b], nchk[b]: stripe b's source, row and check-row counts; blamed[b]
    {column: shard}, unexplained[b] [column]; truth[b], implied[b]: {index: bytes}."""

    def __init__(self, k, m, stripes, store, seed=1):
        n = k + m
        self.k, self.m, self.n, self.store, self.stripes = k, m, n, store, stripes
        rng = np.random.default_rng(seed)
        ar = self.ar = Arena()
        self.off = [{i: ar.take(st["S"]) for i in sorted(set(st["expect"]) | set(st["compared"]) | set(st["wanted"]))}
                    for st in stripes]
        self.acc = [{j: ar.take(st["S"]) for j in st["compared"]} for st in stripes]
        self.fixo = [{i: ar.take(st["S"]) for i, mode in sorted(st["fix"].items()) if mode == "zero"}
                     for st in stripes]
        ar.layout()
        start = self.start = ar.start
        B = len(stripes)
        self.counts = np.zeros((B, n + 1), dtype=np.uint64)
        self.flagged, self.srcs, self.nrows, self.nchk, self.cmp_fed = [], [], [], [], []
        self.blamed, self.unexplained, self.truth, self.implied, self.delivered = [], [], [], [], []
        first = []
        for b, st in enumerate(stripes):
            S, V, J, Wd, feeds = st["S"], st["expect"], st["compared"], st["wanted"], list(st["feeds"])
            cmp_fed = st["cmp_fed"] if st["cmp_fed"] is not None else (J if store else ())
            assert len(V) == k and list(V) == sorted(set(V)) and J and len(J) + len(Wd) <= 16
            assert not set(Wd) & set(J) and not (set(Wd) | set(J)) & set(V)
            assert set(cmp_fed) <= set(J) and set(feeds) <= set(range(k))
            assert all(mode in (None, "zero", "alias") and i in V + J for i, mode in st["fix"].items())
            if store:  # a complete decode, or a stripe that is delivered nothing and only scans
                assert tuple(cmp_fed) == J or (not cmp_fed and not feeds and not Wd and not st["damage"])
            C = coef(k, m, V)
            X = rng.integers(0, 256, (k, S), dtype=np.uint8)
            notfed = [j for j in range(k) if j not in feeds]
            if store:
                X[notfed] = 0
            rows = sorted(J + Wd)
            truth = {V[j]: X[j] for j in range(k)}
            truth.update(apply_rows(C, rows, list(range(k)), list(X), S))
            D = {i: truth[i].copy() for i in V + J}
            cols = {}
            for shard, col, val in st["damage"]:
                assert shard in D and 0 <= col < S and 0 < val < 256, (b, shard, col, val)
                assert not store or shard in J or V.index(shard) in feeds, "nothing reads this shard"
                assert shard not in cols.get(col, ()), (b, shard, col)
                D[shard][col] ^= val
                cols.setdefault(col, []).append(shard)
            blamed = {c: s[0] for c, s in cols.items() if len(s) == 1 and len(J) >= 3}
            unexplained = sorted(set(cols) - set(blamed))
            for c in unexplained:
                assert (len(cols[c]) <= len(J) if len(J) < 3 else 2 <= len(cols[c]) < len(J)), \
                    "the rule promises nothing here"
            implied = apply_rows(C, list(Wd), list(range(k)), [D[V[j]] for j in range(k)], S)
            for c in unexplained:  # one damaged expected shard: G has no zero entry
                if sum(s in V for s in cols[c]) == 1:
                    assert all(implied[w][c] != truth[w][c] for w in Wd), (b, c)
            part = apply_rows(C, rows, notfed, [D[V[j]] for j in notfed], S)
            for i in V + J:
                put(start, self.off[b][i], D[i])
            for w in Wd:
                put(start, self.off[b][w], rng.integers(0, 256, S, dtype=np.uint8) if store else part[w])
            for j in J:
                put(start, self.acc[b][j], rng.integers(0, 256, S, dtype=np.uint8) if store
                    else part[j] if j in cmp_fed else part[j] ^ D[j])
            for o in self.fixo[b].values():
                start[o:o + S] = 0
            first.append((C, D, cols))
            self.blamed.append(blamed)
            self.unexplained.append(unexplained)
            self.truth.append(truth)
            self.implied.append(implied)
            self.delivered.append(D)
            self.cmp_fed.append(tuple(cmp_fed))
            self.srcs.append(len(feeds) + len(cmp_fed))
            self.nrows.append(len(rows))
            self.nchk.append(len(J))
            if cols:
                self.flagged.append(b)
        self.rows = max(self.nrows)
        want = self.want = start.copy()
        for b, st in enumerate(stripes):
            S, V, Wd = st["S"], st["expect"], st["wanted"]
            C, D, cols = first[b]
            truth, blamed, unexplained = self.truth[b], self.blamed[b], self.unexplained[b]
            # a wanted row is rewritten with other bytes when the launch stores it, adds a source's
            # terms to it or takes an expected shard's error out of it; otherwise it must stay
            moves = store or bool(st["feeds"]) or any(s in V for s in blamed.values())
            for w in Wd:
                row = truth[w].copy()
                row[unexplained] = self.implied[b][w][unexplained]
                assert np.array_equal(row, get(start, self.off[b][w], S)) != moves, (b, w)
                put(want, self.off[b][w], row)
            self.counts[b, n] = len(unexplained)
            for c, shard in blamed.items():
                self.counts[b, shard] += 1
                e = int(D[shard][c] ^ truth[shard][c])
                assert e != 0
                mode = st["fix"].get(shard)
                if mode == "zero":
                    want[self.fixo[b][shard] + c] ^= e
                elif mode == "alias":
                    want[self.off[b][shard] + c] ^= e
                    assert want[self.off[b][shard] + c] == truth[shard][c]

    def pointers(self, ptr):
        """(expect flags, input, dst, check, fix) of the plan; ptr maps an arena offset."""
        flags, inp, dst, chk, fix = [], [], [], [], []
        for b, st in enumerate(self.stripes):
            V, J, Wd = st["expect"], st["compared"], st["wanted"]
            fed = {V[j] for j in st["feeds"]} | set(self.cmp_fed[b])
            off = self.off[b]
            flags.append([i in V for i in range(self.n)])
            inp += [ptr(off[i]) if i in fed else 0 for i in range(self.n)]
            dst += [ptr(off[i]) if i in Wd else 0 for i in range(self.n)]
            chk += [ptr(self.acc[b][i]) if i in J else 0 for i in range(self.n)]
            for i in range(self.n):
                mode = st["fix"].get(i)
                fix.append(ptr(self.fixo[b][i]) if mode == "zero" else ptr(off[i]) if mode == "alias" else 0)
        return flags, inp, dst, chk, fix


def run_decode_repair(k, m, stripes, store, seed=1):
    """One decode-repair launch over RepairModel's starting image: the whole allocation, the
    flagged stripes and the counts -- per shard, and bin n for the unexplained columns -- are the
    model's, exactly. Returns the model."""
    from callfs_amd.device import Plan
    md = RepairModel(k, m, stripes, store, seed)
    ar = md.ar
    ar.seal()
    flags, inp, dst, chk, fix = md.pointers(ar.ptr)
    plan = Plan.decode_repair(k, m, [st["S"] for st in stripes], flags, inp, dst, chk, fix, store=store)
    check_plan(plan, "decode-repair", md.rows)
    ar.upload(md.start)
    plan.launch()
    flagged = plan.corrupt_stripes()
    counts = plan.blame()
    assert ar.wrong(md.want) == [], ("decode-repair", store, k, m)
    bad = np.argwhere(counts != md.counts)[:6].tolist()
    assert not bad, ("decode-repair", store, k, m, [(b, i, int(counts[b, i]), int(md.counts[b, i])) for b, i in bad])
    assert flagged == md.flagged, ("decode-repair", store, k, m, flagged, md.flagged)
    assert plan.corrupt_stripes() == [] and not plan.blame().any()
    plan.close()
    return md


def _fix_by_turns(b, shards):
    """Null and non-null fix pointers within one stripe."""
    return {i: ("zero", "alias", None)[(b + i) % 3] for i in shards}


def repair_counted(k, m, counts, store, seed):
    """The stripes of the input-axis plan: one per source count C, the most sources first, and a
    last one that is delivered nothing. Stripes 0 and 4 have m rows, the rest fewer (narrow_rows);
    the check rows are the front of the row list. Under store C counts the compared shards, all
    delivered, and the stripe that is delivered nothing has no wanted row; under merge an odd
    stripe delivers one compared shard among its C sources, and the source-less stripe keeps its
    wanted rows. Stripes 1, 4, 7, ... are damaged: in turn a compared shard's byte in the tail and
    an expected shard's byte in the vector body (two_cols); under merge also the source-less stripe,
    in an expected shard that is merged already, with three check rows."""
    counts = tuple(counts)[::-1] + (0,)
    B = len(counts)
    sizes = cycle_sizes(B, first=seed)
    widths = [m] + narrow_rows(m)
    rng = np.random.default_rng(seed)
    out = []
    for b, (C, S) in enumerate(zip(counts, sizes)):
        e = expected_set(k, m, b)
        rest = [i for i in range(k + m) if i not in e]
        w = m if b in (0, 4) else widths[b % len(widths)]
        rows = rest[:w] if b % 2 == 0 else rest[-w:]
        nchk = min((3, 3, 4, 3, 3, 5, 1, 8, 2, 3)[b % 10], w)
        if store and C:
            nchk = min(nchk, C)
        cmp_ = rows[:nchk]
        if store:
            cmp_fed = tuple(cmp_) if C else ()
        else:
            cmp_fed = tuple(cmp_[-1:]) if b % 2 and C >= 2 else ()
        nf = C - len(cmp_fed)
        assert 0 <= nf <= k
        feeds = sorted(int(j) for j in rng.choice(k, size=nf, replace=False))
        wanted = [i for i in rows if i not in cmp_] if C or not store else []
        last = not store and b == B - 1
        damage = ()
        if (b % 3 == 1 or last) and (C or not store):
            body, tail = two_cols(S)
            if (last or (b // 3) % 2 == 1) and (nf or not store):
                pos = feeds[(seed + b) % nf] if store else (seed + b) % k
                damage = ((e[pos], body, 0x21 + b),)
            else:
                damage = ((cmp_[(seed + b) % nchk], tail, 0x21 + b),)
        out.append(repair_stripe(S, e, cmp_, wanted, feeds, cmp_fed, damage, _fix_by_turns(b, tuple(e) + tuple(cmp_))))
    return out


REPAIR_ROWS = {"rt4": ((3, 0), (3, 1), (4, 0), (2, 2)),
               "rt8": ((3, 2), (4, 1), (5, 0), (5, 3), (6, 1), (7, 1), (8, 0), (3, 5)),
               "rt16": ((3, 6), (5, 4), (9, 0), (9, 7), (12, 1), (13, 3), (15, 1), (16, 0), (3, 13))}


def repair_row_stripes(k, nchk, nwant, store, seed):
    """RS(k, nchk + nwant): a clean stripe, one with a byte of an expected shard damaged in the
    vector body, one with a byte of the last check row's compared shard (syndrome byte r' - 1)
    damaged in the tail, one with a byte of the first check row's compared shard damaged. Store:
    everything is delivered; merge: k, 1, k - 1 and no expected shards and every other compared
    shard."""
    m = nchk + nwant
    sizes = (40, 8211, 40, 8211) if k == 3 else (8211, 40, 8211, 16)
    out = []
    for b, S in enumerate(sizes):
        e = expected_set(k, m, b + seed)
        rest = [i for i in range(k + m) if i not in e]
        cmp_ = rest[:nchk] if b % 2 == 0 else rest[-nchk:]
        wanted = [i for i in rest if i not in cmp_]
        feeds = range(k) if store else range((k, 1, k - 1, 0)[b])
        cmp_fed = None if store else cmp_[b % 2::2]
        body, tail = two_cols(S)
        damage = ((), ((e[(seed + 1) % k], body, 0x31),), ((cmp_[-1], tail, 0x32),),
                  ((cmp_[0], (body, tail)[nchk % 2], 0x33),))[b]
        out.append(repair_stripe(S, e, cmp_, wanted, feeds, cmp_fed, damage, _fix_by_turns(b, tuple(e) + tuple(cmp_))))
    return out


RUN_S = 8192 + 16 * 3 + 5  # a full tile, three vectors of a second, a 5-byte tail
RUN_SHAPES = ((3, 1), (4, 4), (7, 1), (13, 3))  # RT 4 (early loads), RT 8, RT 8, RT 16 (four words)
RUN_VECTORS = (0, 63, 64, 512, 514)  # the first; lanes 63 and 64 of tile 0; the first of tile 1; the last


def repair_run_stripes(nchk, nwant, store, fix):
    """RS(10, nchk + nwant) at RUN_S. A and B are expected shards, X a compared shard, L the last
    expected shard (position k - 1) and X0 compared shard 0 (position k); U is a column damaged in
    B and X, unexplained. The sequences, by column of one 16-byte vector:
      0 A, B          1 A, X, A at columns 2, 3, 4 (both sides of a word of the gathered vector)
      2 A, U, A       3 U at column 0, A at column 15
      4 A and B in turn over all 16 columns           5 L, X0 at columns 8, 9
    Stripe 0 has sequences 0..4 at RUN_VECTORS and 5 at vector 65, stripe 1 has 5, 4, 3, 2, 1 there
    and 0 at vector 300; stripe 2 has four neighbouring lanes of one wave with a change from A to B
    at column 3, one at column 7, a clean lane and a lane that is wholly A; stripe 3 is clean.
    fix "zero": every fix buffer zeroed; "mixed": A's pointer null, L aliased, the others zeroed."""
    k, m, S = 10, nchk + nwant, RUN_S
    assert S // 16 - 1 == RUN_VECTORS[-1] and S % 16
    e = expected_set(k, m, 2)
    rest = [i for i in range(k + m) if i not in e]
    cmp_, wanted = rest[:nchk], rest[nchk:]
    A, Bs, X, L, X0 = e[2], e[7], cmp_[nchk - 2], e[k - 1], cmp_[0]
    assert nchk >= 3 and len({A, Bs, X, L, X0}) == 5
    seqs = (((A, 0), (Bs, 1)),
            ((A, 2), (X, 3), (A, 4)),
            ((A, 5), (Bs, 6), (X, 6), (A, 7)),
            ((Bs, 0), (X, 0), (A, 15)),
            tuple(((A, Bs)[c % 2], c) for c in range(16)),
            ((L, 8), (X0, 9)))
    four = (tuple((A if c < 3 else Bs, c) for c in range(5)),
            tuple((A if c < 7 else Bs, c) for c in range(10)),
            (),
            tuple((A, c) for c in range(16)))
    places = (dict(zip(RUN_VECTORS + (65,), seqs)),
              dict(zip(RUN_VECTORS + (300,), (seqs[5], seqs[4], seqs[3], seqs[2], seqs[1], seqs[0]))),
              {2 * 64 + 10 + q: four[q] for q in range(4)},
              {})
    modes = {i: "zero" for i in tuple(e) + tuple(cmp_)}
    if fix == "mixed":
        modes[A], modes[L] = None, "alias"
    else:
        assert fix == "zero"
    out, nth = [], 0
    for b, place in enumerate(places):
        damage = []
        for vec, seq in sorted(place.items()):
            for shard, c in seq:
                nth += 1
                damage.append((shard, 16 * vec + c, 1 + (37 * nth) % 255))
        feeds = range(k) if store else (range(1, k, 2), range(k), range(5), (k - 1,))[b]
        cmp_fed = None if store else (cmp_[1:], (), cmp_, cmp_[:1])[b]
        out.append(repair_stripe(S, e, cmp_, wanted, feeds, cmp_fed, damage, dict(modes)))
    return out, dict(A=A, B=Bs, X=X, L=L, X0=X0)


def _wanted_rows_hold(md):
    """Every wanted row of the expected image is the true shard but in the unexplained columns,
    where it is what the damaged expected shards imply, and that is not the truth."""
    for b, st in enumerate(md.stripes):
        S, un = st["S"], md.unexplained[b]
        for w in st["wanted"]:
            row = get(md.want, md.off[b][w], S)
            keep = np.ones(S, dtype=bool)
            keep[un] = False
            assert np.array_equal(row[keep], md.truth[b][w][keep]), (b, w)
            assert np.array_equal(row[un], md.implied[b][w][un]), (b, w)


def check_repair_counted(md, k, m, counts, store):
    """The input-axis plan is the intended one: the source counts, m rows on stripe 0, a damaged and
    a clean stripe, null and non-null fix pointers within every stripe, a source-less last stripe
    that under merge keeps wanted rows and has an expected shard's error taken out of them, and, in
    the plans of ten stripes, a repair with wanted rows."""
    B = len(md.stripes)
    assert tuple(md.srcs) == tuple(counts)[::-1] + (0,), md.srcs
    assert md.nrows[0] == md.rows == m and all(r <= m for r in md.nrows)
    assert md.flagged and len(md.flagged) < B and 0 not in md.flagged
    for st in md.stripes:
        modes = set(st["fix"].values())
        assert None in modes and "zero" in modes
    last = md.stripes[-1]
    if store:
        assert not last["wanted"] and not last["damage"]
    else:
        assert B - 1 in md.flagged
        if B == 10 or (md.nchk[B - 1] >= 3 and last["wanted"]):
            assert last["wanted"] and md.blamed[B - 1] and set(md.blamed[B - 1].values()) <= set(last["expect"])
    if B == 10:
        assert md.nrows[4] == m and md.stripes[4]["wanted"] and md.nchk[4] == 3
        assert set(md.blamed[4].values()) <= set(md.stripes[4]["expect"]) and md.blamed[4]
    _wanted_rows_hold(md)


def check_repair_rows(md, nchk, nwant):
    """Four stripes of nchk + nwant rows: clean; an expected shard in the vector body; the last
    check row's compared shard in the tail; the first check row's compared shard."""
    assert md.nchk == [nchk] * 4 and md.nrows == [nchk + nwant] * 4 and md.flagged == [1, 2, 3]
    (s1, c1, _), = md.stripes[1]["damage"]
    (s2, c2, _), = md.stripes[2]["damage"]
    (s3, _, _), = md.stripes[3]["damage"]
    assert s1 in md.stripes[1]["expect"] and c1 < md.stripes[1]["S"] // 16 * 16
    assert s2 == max(md.stripes[2]["compared"]) and c2 >= md.stripes[2]["S"] // 16 * 16
    assert s3 == min(md.stripes[3]["compared"])
    for b, s in ((1, s1), (2, s2), (3, s3)):
        if nchk >= 3:
            assert md.counts[b, s] == 1 == md.counts[b].sum()
        else:
            assert md.counts[b, md.n] == 1 == md.counts[b].sum()
    _wanted_rows_hold(md)


def check_repair_runs(md, names, shape, fix):
    """The counts the sequences give, per shard and for the unexplained bin; the wanted rows; both
    of A's error bytes around X in A's fix row; A's null pointer and L's aliased buffer."""
    A, Bs, X, L, X0 = (names[q] for q in ("A", "B", "X", "L", "X0"))
    assert md.nrows == [sum(shape)] * 4 and md.nchk == [shape[0]] * 4 and md.flagged == [0, 1, 2]
    for b in (0, 1):
        exp = {A: 1 + 2 + 2 + 1 + 8, Bs: 1 + 8, X: 1, L: 1, X0: 1, md.n: 2}
        assert {i: int(c) for i, c in enumerate(md.counts[b]) if c} == exp, (b, md.counts[b].nonzero())
        assert len(md.unexplained[b]) == 2
    assert {i: int(c) for i, c in enumerate(md.counts[2]) if c} == {A: 3 + 7 + 16, Bs: 2 + 3}
    assert not md.counts[3].any()
    _wanted_rows_hold(md)
    col = 16 * RUN_VECTORS[1] + 2  # stripe 0: A, X, A in lane 63
    if fix == "zero":
        row = get(md.want, md.fixo[0][A], RUN_S)
        assert row[col] and not row[col + 1] and row[col + 2]
        assert get(md.want, md.fixo[0][X], RUN_S)[col + 1]
    else:
        assert A not in md.fixo[0] and md.stripes[0]["fix"][A] is None and md.stripes[0]["fix"][L] == "alias"
        assert np.array_equal(get(md.want, md.off[0][L], RUN_S), md.truth[0][L])
        assert not np.array_equal(get(md.start, md.off[0][L], RUN_S), md.truth[0][L])
        assert not np.array_equal(get(md.want, md.off[0][A], RUN_S), md.truth[0][A])  # A stays as delivered


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
WIDE_KINDS = ("mixed", "ragged", "required", "update-single", "locate", "locate2", "correct", "repair",
              "repair-store")
WIDE_SIZES = (40, 8211)
_WIDE_COLS = {40: (1, 17, 20, 33, 35, 38), 8211: (5, 100, 8190, 8195, 8209, 8210)}
_WIDE_PAIR_COL = {40: 25, 8211: 4000}


def repair_wide_stripes(k, m, store):
    """Three check rows (the last three of the other indices: 253..255 in RS(240,16), verdict 255
    and positions 240..242 of the fix table) and every remaining index wanted, 9 or 16 rows: 16-byte
    table entries. The source count is exactly k: under merge every expected shard, under store all
    but positions 1..3 and the three compared shards. Sizes 40 and 8211 with one byte each damaged
    in the expected shards at positions 0, 127, 128 and 239 (those below k, and k - 1) and in the last
    compared shard, in different columns; a third stripe is clean."""
    e = tuple(range(k))
    rest = list(range(k, k + m))
    cmp_, wanted = rest[-3:], rest[:-3]
    feeds = [j for j in range(k) if not (store and 1 <= j <= 3)]
    hit = [e[j] for j in sorted({j for j in (0, 127, 128, 239, k - 1) if j < k})][:4] + [cmp_[-1]]
    out = []
    for S in WIDE_SIZES + (40,):
        damage = [(s, _WIDE_COLS[S][q], 0x11 * (q + 1)) for q, s in enumerate(hit)] if len(out) < 2 else ()
        fix = {s: "zero" for s in hit}
        fix[hit[0]] = "alias"
        out.append(repair_stripe(S, e, cmp_, wanted, feeds, None, damage, fix))
    return out


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
    elif kind.startswith("repair"):
        md = run_decode_repair(k, m, repair_wide_stripes(k, m, kind == "repair-store"), kind == "repair-store", seed)
        assert md.rows == m > 8 and set(md.srcs) == {k}
        hits = 1 + len({j for j in (0, 127, 128, 239, k - 1) if j < k})
        assert hits == (5 if k == 240 else 3 if k < 129 else 4)
        assert md.flagged == [0, 1] and int(md.counts.sum()) == 2 * hits and not md.counts[:, n].any()
        assert k + m < 256 or md.counts[0, 255] == 1  # the verdict 255
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
