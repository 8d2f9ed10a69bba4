"""Absorb objects (rs_absorb_create / rs_absorb_launch): byte ranges of an
object's body into the object's resident parity rows. Every case runs in a sentinel-filled Arena
(tests/shape_lattice.py) with the body and the rows at odd offsets and 4 KiB guards; the rows start
zeroed, and after every launch the whole allocation is compared with the image the rule gives:
the rows are the C oracle's Encode of the body with every byte not yet fed set to zero
(tests/absorb_cases.py), everything else is what it was. Nothing here has a tolerance."""
import numpy as np
import pytest

from absorb_cases import (OTHER_PROFILES, PATTERNS, SIZES, T, Masked, body_len, parity_of, random_body,
                          ranges, shards_of)
from shape_lattice import Arena, get, put

pytestmark = pytest.mark.gpu


class _Case:
    """One object: its body in one buffer and a zeroed row per parity shard."""

    def __init__(self, k, m, S, L, seed, body=None):
        from callfs_amd.device import Absorb
        self.rng = np.random.default_rng(seed)
        self.k, self.m, self.S, self.L = k, m, S, L
        self.body = random_body(L, self.rng) if body is None else body
        ar = self.ar = Arena()
        self.src = ar.take(L)
        self.row = [ar.take(S) for _ in range(m)]
        ar.seal()
        put(ar.start, self.src, self.body)
        for o in self.row:
            ar.start[o:o + S] = 0
        self.absorb = Absorb(k, m, S, [ar.ptr(o) for o in self.row])
        self.masked = Masked(self.body, k, m, S)

    def after(self, img, off, n):
        """The image after [off, off + n) is fed: it differs from `img`, in the rows alone."""
        par = self.masked.feed(off, n)
        out = img.copy()
        for j, o in enumerate(self.row):
            put(out, o, par[j])
        assert not np.array_equal(out, img), (off, n)
        return out

    def launch(self, off, n, stream=None, src=None):
        self.absorb.launch(off, n, (self.ar.ptr(self.src) if src is None else src) + off, stream=stream)

    def drive(self, rs):
        ar = self.ar
        ar.upload(ar.start)
        img = ar.start
        for at, (off, n) in enumerate(rs):
            img = self.after(img, off, n)
            self.launch(off, n)
            assert ar.wrong(img) == [], (self.k, self.m, self.S, at, off, n)
        return img

    def check_final(self, img):
        want = parity_of(self.body, self.k, self.m, self.S)
        assert self.masked.fed.tobytes() == self.body.tobytes()
        for j, o in enumerate(self.row):
            assert np.array_equal(get(img, o, self.S), want[j]), j

    def close(self):
        self.absorb.close()


def _run(k, m, S, L, pattern, seed):
    c = _Case(k, m, S, L, seed)
    rs = ranges(pattern, S, L, c.rng)
    assert rs is not None and sum(n for _, n in rs) == L
    c.check_final(c.drive(rs))
    c.close()


def _patterns(S):
    return [p for p in PATTERNS if ranges(p, S, S * 10, np.random.default_rng(0)) is not None]


@pytest.mark.parametrize("S,pattern", [(S, p) for S in SIZES for p in _patterns(S)])
def test_rs_10_4_every_size_and_pattern(S, pattern):
    _run(10, 4, S, body_len(10, S), pattern, seed=1000 * PATTERNS.index(pattern) + S)


@pytest.mark.parametrize("S", (16, 40, T))
def test_rs_10_4_a_body_without_padding(S):
    for pattern in ("whole", "cycle", "three"):
        _run(10, 4, S, 10 * S, pattern, seed=S)


# RS(1,3), (3,2), (4,2), (16,4) run in the 4-row instance, (10,8) in the 8-row one, (20,12) and
# (64,16) in the 16-row one (its rows come from the device table)
@pytest.mark.parametrize("S,pattern", [(S, p) for S in (17, T + 16) for p in _patterns(S)])
@pytest.mark.parametrize("k,m", OTHER_PROFILES)
def test_other_profiles(k, m, S, pattern):
    _run(k, m, S, body_len(k, S), pattern, seed=k * 100 + m + S)


def test_hi_under_rs_4_2():
    """L = 2, S = 1: the known-answer parity bytes 19, 1e."""
    body = np.frombuffer(b"hi", dtype=np.uint8).copy()
    for rs in ([(0, 2)], [(1, 1), (0, 1)]):
        c = _Case(4, 2, 1, 2, seed=1, body=body)
        img = c.drive(rs)
        assert [int(get(img, o, 1)[0]) for o in c.row] == [0x19, 0x1E]
        c.check_final(img)
        c.close()


def test_a_source_in_pinned_host_memory():
    """The source may be host-coherent pinned memory, at an odd address."""
    import torch
    k, m, S = 10, 4, T + 21
    L = body_len(k, S)
    c = _Case(k, m, S, L, seed=9)
    pinned = torch.empty(L + 64, dtype=torch.uint8).pin_memory()
    pinned.numpy()[3:3 + L] = c.body
    ar = c.ar
    ar.upload(ar.start)
    img = ar.start
    for off, n in ranges("three", S, L, c.rng):
        img = c.after(img, off, n)
        c.launch(off, n, src=pinned.data_ptr() + 3)
        assert ar.wrong(img) == [], (off, n)
    c.check_final(img)
    c.close()


def test_a_captured_graph_of_three_launches():
    """A linear graph of three launches, replayed once."""
    import torch
    k, m, S = 10, 4, 2 * T + 83
    L = body_len(k, S)
    c = _Case(k, m, S, L, seed=5)
    rs = ranges("cycle", S, L, c.rng)
    ar = c.ar
    ar.upload(ar.start)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    img = c.after(ar.start, *rs[0])
    with torch.cuda.stream(s):
        c.launch(*rs[0], stream=s)
    torch.cuda.synchronize()
    assert ar.wrong(img) == []
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for off, n in rs[1:4]:
            c.launch(off, n, stream=s)
    assert ar.wrong(img) == []  # capturing ran nothing
    for off, n in rs[1:4]:
        img = c.after(img, off, n)
    g.replay()
    assert ar.wrong(img) == []
    for off, n in rs[4:]:
        img = c.after(img, off, n)
        c.launch(off, n)
    assert ar.wrong(img) == []
    c.check_final(img)
    c.close()


@pytest.mark.parametrize("k,m,S", [(10, 4, 40), (10, 4, 2 * T + 83), (10, 8, T + 16), (20, 12, T + 16)])
def test_one_whole_body_launch_equals_the_uniform_encode_plan(k, m, S):
    import torch
    from callfs_amd.device import Plan
    L = k * S
    c = _Case(k, m, S, L, seed=S + m)
    img = c.drive([(0, L)])
    mine = np.stack([get(img, o, S) for o in c.row])
    pitch = (S + 255) // 256 * 256
    buf = torch.zeros((k + m) * pitch, dtype=torch.uint8, device="cuda:0")
    sh = shards_of(c.body, k, S)
    for i in range(k):
        buf[i * pitch:i * pitch + S].copy_(torch.from_numpy(sh[i]))
    plan = Plan(k, m, S, 1, [buf.data_ptr() + i * pitch for i in range(k + m)])
    plan.launch()
    torch.cuda.synchronize()
    theirs = buf.cpu().numpy().reshape(k + m, pitch)[k:, :S]
    plan.close()
    assert np.array_equal(mine, theirs)
    c.close()


def test_launch_refusals():
    from callfs_amd import _native as N
    c = _Case(10, 4, 40, 393, seed=3)
    ar = c.ar
    ar.upload(ar.start)
    h, src = c.absorb.handle, ar.ptr(c.src)
    import ctypes
    vp = ctypes.c_void_p
    assert N.lib.rs_absorb_launch(h, 0, 0, vp(src), None) == N.RS_E_ARG
    assert N.lib.rs_absorb_launch(h, 400, 1, vp(src), None) == N.RS_E_ARG
    assert N.lib.rs_absorb_launch(h, 399, 2, vp(src), None) == N.RS_E_ARG
    assert N.lib.rs_absorb_launch(h, 0, 401, vp(src), None) == N.RS_E_ARG
    assert N.lib.rs_absorb_launch(h, 0, 10, None, None) == N.RS_E_ARG
    assert N.lib.rs_absorb_launch(None, 0, 10, vp(src), None) == N.RS_E_ARG
    assert ar.wrong(ar.start) == []  # nothing ran
    c.close()
