"""Feed objects (rs_feed_create / rs_feed_launch): one shard per launch into the
resident rows of one stripe. Every case runs in a sentinel-filled Arena (tests/shape_lattice.py)
with the sources and the rows at odd offsets and 4 KiB guards; the first launch stores over junk,
the later ones merge, and after every launch the whole allocation is compared with the image the
rule gives. Expected bytes come from the C oracle alone: a launch's terms are
cref.apply(C[rows][:, position], shard) with C = cref.reconstruct of the k unit vectors, and a
compared shard's term is the shard itself in its own row. Nothing here has a tolerance."""
import numpy as np
import pytest

from shape_lattice import Arena, apply_rows, codeword, coef, expected_set, get, put

pytestmark = pytest.mark.gpu

T = 4096  # bytes of the source, and of every row, per block
SIZES = (1, 5, 15, 16, 17, 40, 1023, T - 1, T, T + 1, T + 16, 2 * T + 83)


def _config(k, m, which):
    """(expected, wanted, compared) of RS(k, m): 0 = the first k expected, one wanted and the rest
    compared; 1 = the last k expected and every other shard wanted; 2 = an expected set that mixes
    data and parity, half of the rest wanted and half compared."""
    e = expected_set(k, m, which)
    rest = [i for i in range(k + m) if i not in e]
    nw = (1, len(rest), len(rest) // 2)[which]
    return e, tuple(rest[:nw]), tuple(rest[nw:])


class _Case:
    """One stripe: a codeword whose every shard is nonzero in its first byte, the compared shards
    damaged in their last byte, a source buffer per fed shard and a junk-filled row per wanted or
    compared shard."""

    def __init__(self, k, m, S, expect, wanted, compared, seed, first=None):
        from callfs_amd.device import Feed
        rng = np.random.default_rng(seed)
        self.k, self.m, self.S = k, m, S
        self.expect, self.wanted, self.compared = expect, wanted, compared
        self.rows = list(compared) + list(wanted)  # the feed object's order
        while True:
            st = codeword(k, m, S, rng)
            if (st[:, 0] != 0).all():
                break
        self.truth = st
        self.shard = st.copy()
        for j in compared:  # as delivered: damaged in the last byte, still nonzero in the first
            self.shard[j, S - 1] ^= 0x40 if S > 1 or self.shard[j, 0] != 0x40 else 0x80
        self.fed = list(expect) + list(compared)
        assert all(self.shard[i, 0] != 0 for i in self.fed)  # every fed shard is nonzero in its first byte
        self.C = coef(k, m, tuple(expect))
        ar = self.ar = Arena()
        self.src = {i: ar.take(S) for i in self.fed}
        self.row = {i: ar.take(S) for i in self.rows}
        ar.seal()
        for i in self.fed:
            put(ar.start, self.src[i], self.shard[i])
        self.order = [int(i) for i in rng.permutation(self.fed)]
        if first is not None:
            self.order = [first] + [i for i in self.order if i != first]
        # junk in every row; its first byte differs from what the first (store) launch leaves
        # there, so that launch changes every row whatever the rest of the junk is
        stored = self.terms(self.order[0])
        for i in self.rows:
            junk = rng.integers(0, 256, S, dtype=np.uint8)
            junk[0] = stored[i][0] ^ 0xFF
            put(ar.start, self.row[i], junk)
        n = k + m
        self.feed = Feed(k, m, S, [i in expect for i in range(n)],
                         [ar.ptr(self.row[i]) if i in wanted else 0 for i in range(n)],
                         [ar.ptr(self.row[i]) if i in compared else 0 for i in range(n)])

    def terms(self, idx):
        """{row: what feeding shard idx adds to the row}, from the oracle."""
        if idx in self.expect:
            assert all(self.C[r, self.expect.index(idx)] != 0 for r in self.rows)
            return apply_rows(self.C, self.rows, [self.expect.index(idx)], [self.shard[idx]], self.S)
        return {r: self.shard[idx] if r == idx else np.zeros(self.S, dtype=np.uint8) for r in self.rows}

    def after(self, img, idx, store):
        """The image after shard idx is fed; asserts on the CPU that the launch changes every row
        it must, and no other."""
        terms = self.terms(idx)
        out = img.copy()
        changed = set()
        for r in self.rows:
            old = get(img, self.row[r], self.S)
            new = terms[r] if store else old ^ terms[r]
            if not np.array_equal(new, old):
                changed.add(r)
            put(out, self.row[r], new)
        must = set(self.rows) if store or idx in self.expect else {idx}
        assert changed == must, (idx, store, sorted(changed), sorted(must))
        return out

    def launch_feed(self, idx, store, stream=None):
        self.feed.launch(idx, self.ar.ptr(self.src[idx]), store=store, stream=stream)

    def launch_plan(self, idx, store, stream=None):
        """The same delivery as a non-final decode-check plan with that one input."""
        from callfs_amd.device import Plan
        n = self.k + self.m
        plan = Plan.decode_check(self.k, self.m, [self.S], [[i in self.expect for i in range(n)]],
                                 [self.ar.ptr(self.src[i]) if i == idx else 0 for i in range(n)],
                                 [self.ar.ptr(self.row[i]) if i in self.wanted else 0 for i in range(n)],
                                 [self.ar.ptr(self.row[i]) if i in self.compared else 0 for i in range(n)],
                                 store=store)
        plan.launch()
        import torch
        torch.cuda.synchronize()
        plan.close()

    def drive(self, order, launch):
        """Feeds `order`, the first launch storing, and compares the whole allocation after every
        launch; returns the images."""
        ar = self.ar
        ar.upload(ar.start)
        img, images = ar.start, []
        for at, idx in enumerate(order):
            img = self.after(img, idx, at == 0)
            launch(idx, at == 0)
            assert ar.wrong(img) == [], (self.S, at, idx)
            images.append(img)
        return images

    def check_final(self, img):
        """After every shard: the wanted rows are the codeword's shards, a compared row is the
        shard as delivered XOR the shard the expected ones imply."""
        for w in self.wanted:
            assert np.array_equal(get(img, self.row[w], self.S), self.truth[w]), w
        for j in self.compared:
            assert np.array_equal(get(img, self.row[j], self.S), self.shard[j] ^ self.truth[j]), j
            assert get(img, self.row[j], self.S).any()


@pytest.mark.parametrize("which", (0, 1, 2))
@pytest.mark.parametrize("S", SIZES)
def test_every_shard_in_a_shuffled_order(S, which):
    c = _Case(10, 4, S, *_config(10, 4, which), seed=100 * which + S)
    images = c.drive(c.order, c.launch_feed)
    c.check_final(images[-1])
    c.feed.close()


@pytest.mark.parametrize("which", (0, 2))
@pytest.mark.parametrize("S", (5, 17, T + 1, 2 * T + 83))
def test_a_compared_shard_stored_first_zeroes_the_other_rows(S, which):
    e, wanted, compared = _config(10, 4, which)
    first = compared[-1]
    c = _Case(10, 4, S, e, wanted, compared, seed=7 * S + which, first=first)
    images = c.drive(c.order, c.launch_feed)
    for r in c.rows:  # junk before, zeros after: the store wrote every row and read none
        want = c.shard[first] if r == first else np.zeros(S, dtype=np.uint8)
        assert np.array_equal(get(images[0], c.row[r], S), want), r
    c.check_final(images[-1])
    c.feed.close()


@pytest.mark.parametrize("which", (0, 1, 2))
@pytest.mark.parametrize("S", (15, 40, T + 16, 2 * T + 83))
def test_bit_equal_to_non_final_decode_check_plans(S, which):
    c = _Case(10, 4, S, *_config(10, 4, which), seed=31 * S + which)
    by_feed = c.drive(c.order, c.launch_feed)
    by_plan = c.drive(c.order, c.launch_plan)
    assert all(np.array_equal(a, b) for a, b in zip(by_feed, by_plan))
    c.feed.close()


@pytest.mark.parametrize("S", (17, T + 1))
def test_a_second_merge_launch_restores_what_the_first_started_from(S):
    c = _Case(10, 4, S, *_config(10, 4, 2), seed=S)
    ar = c.ar
    ar.upload(ar.start)
    img = c.after(ar.start, c.order[0], True)
    c.launch_feed(c.order[0], True)
    for idx in c.order[1:4]:
        once = c.after(img, idx, False)
        c.launch_feed(idx, False)
        assert ar.wrong(once) == [], idx
        c.launch_feed(idx, False)
        assert ar.wrong(img) == [], idx
    c.launch_feed(c.order[0], True)  # a store launch is idempotent -- over the merged rows as well
    assert ar.wrong(img) == []
    c.feed.close()


def test_a_captured_graph_of_three_feeds():
    import torch
    S = 2 * T + 83
    c = _Case(10, 4, S, *_config(10, 4, 0), seed=5)
    ar = c.ar
    ar.upload(ar.start)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    img = c.after(ar.start, c.order[0], True)
    with torch.cuda.stream(s):  # outside capture: the store, and a merge launched twice
        c.launch_feed(c.order[0], True, s)
        c.launch_feed(c.order[1], False, s)
        c.launch_feed(c.order[1], False, s)
    torch.cuda.synchronize()
    assert ar.wrong(img) == []
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for idx in c.order[1:4]:
            c.launch_feed(idx, False, s)
    assert ar.wrong(img) == []  # capturing ran nothing
    for idx in c.order[1:4]:
        img = c.after(img, idx, False)
    g.replay()
    assert ar.wrong(img) == []
    for at, idx in enumerate(c.order[4:]):
        img = c.after(img, idx, False)
        c.launch_feed(idx, False)
        assert ar.wrong(img) == [], idx
    c.check_final(img)
    c.feed.close()


# the other profiles, every shard outside the expected set a row: RS(10,8) fills the 8-row
# instance, RS(20,12) with 12 rows runs in the 16-row one (its rows come from the device table)
@pytest.mark.parametrize("k,m,which", [(1, 3, 2), (3, 2, 2), (4, 2, 0), (16, 4, 2), (10, 8, 2), (10, 8, 0),
                                        (20, 12, 2), (20, 12, 1)])
@pytest.mark.parametrize("S", (15, 2 * T + 83))
def test_other_profiles(k, m, which, S):
    e, wanted, compared = _config(k, m, which)
    assert len(wanted) + len(compared) == m
    c = _Case(k, m, S, e, wanted, compared, seed=k * 100 + m + S)
    images = c.drive(c.order, c.launch_feed)
    c.check_final(images[-1])
    c.feed.close()


def test_a_source_in_pinned_host_memory():
    """The source may be host-coherent pinned memory, at an odd address."""
    import torch
    S = T + 21
    c = _Case(10, 4, S, *_config(10, 4, 0), seed=9)
    ar = c.ar
    ar.upload(ar.start)
    pinned = torch.empty(len(c.fed) * (S + 32) + 1, dtype=torch.uint8).pin_memory()
    host = pinned.numpy()
    at = {}
    for q, i in enumerate(c.fed):
        at[i] = (q * (S + 32)) | 1
        host[at[i]:at[i] + S] = c.shard[i]
    img = ar.start
    for q, idx in enumerate(c.order):
        img = c.after(img, idx, q == 0)
        c.feed.launch(idx, pinned.data_ptr() + at[idx], store=q == 0)
        assert ar.wrong(img) == [], (q, idx)
    c.check_final(img)
    c.feed.close()
