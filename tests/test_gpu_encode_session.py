"""Encode sessions (rs_encode_session_open / _feed / _peek / _finish): the body
fed from host memory as it arrives, the parity rows resident on the device. Expected bytes come
from the C oracle's Encode (tests/absorb_cases.py: after any set of feeds the rows are the parity
of the body with every byte not yet fed set to zero), and every finish is also compared, bit for
bit, with rs_codec_encode of the same body. The three feed routes are forced by
CALLFS_RS_SESSION_INPLACE_MAX and rs_host_alloc memory, slot cutting by a small
CALLFS_RS_ENCODE_SESSION_CHUNK; both are read at open. Nothing here has a tolerance."""
import concurrent.futures
import ctypes
import functools

import numpy as np
import pytest

from absorb_cases import Masked, cover, parity_of, random_body

pytestmark = pytest.mark.gpu

K, M = 10, 4
SIZES = (2, 397, 10 * 8211 - 7)
ROUTES = ("inplace", "direct", "staged")
GUARD = 64


@functools.lru_cache(maxsize=None)
def _body(L):
    b = random_body(L, np.random.default_rng(L))
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _parity(L, k=K, m=M):
    p = parity_of(_body(L), k, m, -(-L // k))
    p.setflags(write=False)
    return p


def _counters():
    from callfs_amd.erasure import host_counters
    c = host_counters()
    return np.array([c["calls"], c["launches"], c["copies"]], dtype=np.int64)


def _codec_encode(body, k, m):
    """rs_codec_encode of the whole body: [k + m][S]."""
    from callfs_amd import _native as N
    L = len(body)
    S = -(-L // k)
    out = np.zeros((k + m) * S, dtype=np.uint8)
    ss = ctypes.c_size_t(0)
    data = np.ascontiguousarray(body)
    N.check(N.lib.rs_codec_encode(N.default_context().handle, k, m, ctypes.c_void_p(data.ctypes.data), L,
                                  ctypes.c_void_p(out.ctypes.data), out.size, ctypes.byref(ss)), "rs_codec_encode")
    assert ss.value == S
    return out.reshape(k + m, S)


class _Source:
    """The body where the route wants it: plain memory, or at an odd offset inside an
    rs_host_alloc buffer (the direct route)."""

    def __init__(self, body, route):
        from callfs_amd import _native as N
        self.pinned = None
        if route == "direct":
            self.pinned = N.PinnedBuffer(len(body) + 64, N.default_context())
            self.view = self.pinned.array[5:5 + len(body)]
            self.view[:] = body
        else:
            self.view = body.copy()

    def piece(self, off, n):
        return self.view[off:off + n]

    def close(self):
        if self.pinned is not None:
            self.pinned.close()


def _set_route(monkeypatch, route, chunk=None):
    monkeypatch.setenv("CALLFS_RS_SESSION_INPLACE_MAX", "0" if route == "staged" else str(1 << 30))
    if chunk is None:
        monkeypatch.delenv("CALLFS_RS_ENCODE_SESSION_CHUNK", raising=False)
    else:
        monkeypatch.setenv("CALLFS_RS_ENCODE_SESSION_CHUNK", str(chunk))


def _pieces(n, slot):
    return -(-n // slot)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("L", SIZES)
def test_feeds_peeks_and_finish(L, route, monkeypatch):
    from callfs_amd.erasure import EncodeSession, ErrShortData
    S = -(-L // K)
    slot = max(1, min(L, 3001))  # a small chunk: the larger feeds are cut into slot-sized pieces
    _set_route(monkeypatch, route, slot)
    body, src = _body(L), _Source(_body(L), route)
    rng = np.random.default_rng(L + len(route))
    rs = cover(L, [7, 16, 100, S + 3, 2 * slot + slot // 2])
    rs = [rs[i] for i in rng.permutation(len(rs))]
    masked = Masked(body, K, M, S)
    with EncodeSession(K, M, L) as s:
        assert s.S == S
        for j in range(M):  # before the first feed the rows read zero
            assert not any(s.peek(j))
        # the first ones one by one (the last range is always left), every row peeked after each;
        # the counters move by one call and, per piece, one launch and the route's copies
        nhead = min(6, len(rs) - 1)
        head, left = rs[:nhead], rs[nhead:]
        for off, n in head:
            c0 = _counters()
            s.feed(off, src.piece(off, n))
            p = _pieces(n, slot)
            assert (_counters() - c0).tolist() == [1, p, p if route == "staged" else 0], (off, n, route)
            par = masked.feed(off, n)
            for j in range(M):
                assert bytes(s.peek(j)) == par[j].tobytes(), (off, n, j)
            assert bytes(s.peek(0, min(S, 7))) == par[0][:7].tobytes()
            with pytest.raises(ErrShortData):  # before coverage: the session stays usable
                s.finish()
        # the rest from eight threads over disjoint ranges
        c0 = _counters()
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
            list(ex.map(lambda r: s.feed(r[0], src.piece(*r)), left))
        launches = sum(_pieces(n, slot) for _, n in left)
        assert (_counters() - c0).tolist() == [len(left), launches, launches if route == "staged" else 0]
        for off, n in left:
            masked.feed(off, n)
        want = _parity(L)
        assert np.array_equal(masked.parity(), want)
        for j in range(M):
            assert bytes(s.peek(j)) == want[j].tobytes(), j
        c0 = _counters()
        parity = s.finish()
        assert (_counters() - c0).tolist() == [1, 0, 1]  # one D2H of the rows through staging
        ref = _codec_encode(body, K, M)
        for j in range(M):
            assert bytes(parity[j]) == want[j].tobytes() == ref[K + j].tobytes(), j
        again = s.finish()  # a finish may be repeated: it changes nothing
        assert [bytes(p) for p in again] == [bytes(p) for p in parity]
    src.close()


def test_hi_under_rs_4_2():
    from callfs_amd.erasure import EncodeSession
    with EncodeSession(4, 2, 2) as s:
        s.feed(1, b"i")
        s.feed(0, b"h")
        assert [bytes(p) for p in s.finish()] == [b"\x19", b"\x1e"]


def test_refusals(monkeypatch):
    from callfs_amd import erasure as E
    _set_route(monkeypatch, "inplace")
    L = 397
    body = _body(L)
    with pytest.raises(E.ErrInvalidProfile):
        E.EncodeSession(0, 4, L)
    with pytest.raises(E.ErrShortData):
        E.EncodeSession(K, M, 0)
    with pytest.raises(E.ErrUnsupportedProfile):
        E.EncodeSession(10, 17, L)
    with pytest.raises(E.ErrUnsupportedProfile):
        E.EncodeSession(200, 100, L)
    with E.EncodeSession(K, M, L) as s:
        s.feed(100, body[100:150])
        c0 = _counters()
        for off, n in ((99, 2), (149, 1), (120, 5), (90, 100), (100, 50), (396, 2), (397, 1), (0, 398)):
            with pytest.raises(E.ErrInvalidInput):
                s.feed(off, body[:n] if n <= L else bytes(n))
        with pytest.raises(E.ErrInvalidInput):
            s.feed(0, b"")
        with pytest.raises(E.ErrInvalidInput):
            s.peek(M)
        with pytest.raises(E.ErrInvalidInput):
            s.peek(-1)
        with pytest.raises(E.ErrInvalidInput):
            s.peek(0, s.S + 1)
        with pytest.raises(E.ErrShortData):
            s.finish()
        assert (_counters() - c0).tolist()[1:] == [0, 0]  # nothing was launched or copied
        s.feed(0, body[:100])
        s.feed(150, body[150:])
        want = _parity(L)
        assert [bytes(p) for p in s.finish()] == [w.tobytes() for w in want]
        with pytest.raises(E.ErrInvalidInput):  # feeds after a finish
            s.feed(0, body[:1])
        assert bytes(s.peek(1)) == want[1].tobytes()


@pytest.mark.parametrize("L", (397, 10 * 8211 - 7))
def test_parity_destinations_pinned_and_guarded(L, monkeypatch):
    """Two destinations inside an rs_host_alloc buffer (their D2H goes direct), two in guarded
    plain buffers (one D2H through staging)."""
    from callfs_amd import _native as N
    from callfs_amd.erasure import EncodeSession
    _set_route(monkeypatch, "inplace")
    S = -(-L // K)
    body = _body(L)
    pinned = N.PinnedBuffer(2 * (S + 2 * GUARD) + 8, N.default_context())
    pinned.array[:] = 0xA5
    plain = [np.full(S + 2 * GUARD, 0xA5, dtype=np.uint8) for _ in range(2)]
    at = [3 + GUARD, 3 + GUARD + S + 2 * GUARD]
    dst = [pinned.array[at[0]:at[0] + S], plain[0][GUARD:GUARD + S], pinned.array[at[1]:at[1] + S],
           plain[1][GUARD:GUARD + S]]
    with EncodeSession(K, M, L) as s:
        s.feed(0, body)
        c0 = _counters()
        s.finish(dst)
        assert (_counters() - c0).tolist() == [1, 0, 3]
    want = _parity(L)
    for j in range(M):
        assert dst[j].tobytes() == want[j].tobytes(), j
    # nothing outside the destinations moved
    img = pinned.array.copy()
    for a in at:
        img[a:a + S] = 0xA5
    assert (img == 0xA5).all()
    for p in plain:
        assert (p[:GUARD] == 0xA5).all() and (p[GUARD + S:] == 0xA5).all()
    pinned.close()


@pytest.mark.parametrize("k,m", [(1, 3), (3, 2), (16, 4), (10, 8), (20, 12), (64, 16)])
def test_other_profiles(k, m, monkeypatch):
    from callfs_amd.erasure import EncodeSession
    _set_route(monkeypatch, "inplace", 5000)
    S = 4096 + 16
    L = k * S - min(7, k - 1)
    body = _body(L)
    rs = cover(L, [S + 3, 12000, 7])
    rng = np.random.default_rng(k + m)
    with EncodeSession(k, m, L) as s:
        for i in rng.permutation(len(rs)):
            off, n = rs[i]
            s.feed(off, body[off:off + n])
        got = s.finish()
    want = parity_of(body, k, m, S)
    ref = _codec_encode(body, k, m)
    for j in range(m):
        assert bytes(got[j]) == want[j].tobytes() == ref[k + j].tobytes(), j


@pytest.mark.parametrize("L", (2, 10 * 8211 - 7))
def test_codec_encode_session_round_trip(L, monkeypatch):
    from callfs_amd.erasure import Codec, ErasureProfile
    _set_route(monkeypatch, "inplace")
    prof = ErasureProfile(K, M)
    codec = Codec()
    body = _body(L).tobytes()
    with codec.encode_session(prof, L) as s:
        half = L // 2
        s.feed(half, body[half:])
        s.feed(0, body[:half])
        shards = s.finish()
    ref = codec.encode(body, prof)
    assert [bytes(x) for x in shards] == [bytes(x) for x in ref]
    want = _parity(L)
    assert [bytes(x) for x in shards[K:]] == [w.tobytes() for w in want]
    got = [bytearray(x) for x in shards]
    got[0] = None
    got[K] = None
    assert bytes(codec.decode(got, prof, L)) == body


def test_codec_encode_session_10_mib_in_64_kib_writes():
    from callfs_amd.erasure import Codec, ErasureProfile
    L = 10 << 20
    prof = ErasureProfile(K, M)
    codec = Codec()
    body = np.random.default_rng(10).integers(0, 256, L, dtype=np.uint8).tobytes()
    with codec.encode_session(prof, L) as s:
        for at in range(0, L, 64 << 10):
            assert s.write(body[at:at + (64 << 10)]) == 64 << 10
        shards = s.finish()
    ref = codec.encode(body, prof)
    assert [bytes(x) for x in shards] == [bytes(x) for x in ref]
    S = L // K
    want = parity_of(np.frombuffer(body, dtype=np.uint8), K, M, S)
    assert [bytes(x) for x in shards[K:]] == [w.tobytes() for w in want]
    got = [bytearray(x) for x in shards]
    got[3] = None
    got[K + 1] = None
    assert bytes(codec.decode(got, prof, L)) == body
