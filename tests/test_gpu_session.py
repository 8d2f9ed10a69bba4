"""Decode sessions (rs_session_open / _feed / _peek / _finish): shards fed from
host memory as they land, the rows resident on the device. Expected bytes come from the C oracle
alone (tests/shape_lattice.py: codeword, coef, apply_rows; cref.reconstruct for what corrupted
survivors imply), and every finish is also compared, bit for bit, with the one-shot
rs_decode_check / rs_decode_repair call given the same shards at once. Both feed routes are
forced by CALLFS_RS_SESSION_INPLACE_MAX. Nothing here has a tolerance."""
import concurrent.futures
import functools

import numpy as np
import pytest

from oracle import cref
from shape_lattice import apply_rows, codeword, coef

pytestmark = pytest.mark.gpu

K, M, N_ = 10, 4, 14
EXPECT = (0, 5, 6, 7, 8, 9, 10, 11, 12, 13)  # data and parity mixed; 1..4 are the others
ROUTES = {"inplace": str(1 << 30), "staged": "0"}
SIZES = (40, 8211, (1 << 20) + 1)


@functools.lru_cache(maxsize=None)
def _stripe(S):
    st = codeword(K, M, S, np.random.default_rng(S))
    st.setflags(write=False)
    return st


def _flags(idx):
    return [i in idx for i in range(N_)]


def _open(S, want, compare, repair=False):
    from callfs_amd.erasure import DecodeSession
    return DecodeSession(K, M, S, _flags(EXPECT), _flags(want), _flags(compare), repair=repair)


def _counters():
    from callfs_amd.erasure import host_counters
    c = host_counters()
    return np.array([c["calls"], c["launches"], c["copies"]], dtype=np.int64)


def _implied(shards):
    """What the expected shards of `shards`, as they are, imply for every index."""
    return np.stack(cref.reconstruct([shards[i] if i in EXPECT else None for i in range(N_)], _flags(EXPECT), K, M))


def _one_shot(S, shards, want, compare, repair):
    """The reference call: every delivered shard at once. Returns (raised, dst, fix, counts)."""
    from callfs_amd import erasure as E
    dst = [bytearray(S) if i in want else None for i in range(N_)]
    chk = [bytearray(S) if i in compare else None for i in range(N_)]
    inputs = [bytes(shards[i]) if i in EXPECT or i in compare else None for i in range(N_)]
    fix = [bytearray(S) if i in EXPECT or i in compare else None for i in range(N_)]
    raised, counts = False, None
    try:
        if repair:
            counts = E.decode_repair(dst, chk, fix, _flags(EXPECT), inputs, K, M, store=True)
        else:
            E.decode_check(dst, chk, _flags(EXPECT), inputs, K, M, store=True, final=True)
    except E.ErrShardCorrupted:
        raised = True
    return raised, dst, fix, counts


def _finish(s, fix=None):
    from callfs_amd import erasure as E
    try:
        return False, s.finish(fix=fix)
    except E.ErrShardCorrupted:
        return True, None


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("S", SIZES)
def test_feeds_peeks_and_finish(S, route, monkeypatch):
    monkeypatch.setenv("CALLFS_RS_SESSION_INPLACE_MAX", ROUTES[route])
    st = _stripe(S)
    want, compare = (1,), (2, 3, 4)
    rows = list(compare) + list(want)
    C = coef(K, M, EXPECT)
    order = [int(i) for i in np.random.default_rng(S + len(route)).permutation(list(EXPECT) + list(compare))]
    with _open(S, want, compare) as s:
        for r in rows:  # before the first feed the rows read zero
            assert not any(s.peek(r))
        acc = {r: np.zeros(S, dtype=np.uint8) for r in rows}
        # the first five one by one, every row peeked after each; the counters move by one call,
        # one launch and the route's copies per feed
        for idx in order[:5]:
            c0 = _counters()
            s.feed(idx, bytes(st[idx]))
            assert (_counters() - c0).tolist() == [1, 1, 1 if route == "staged" else 0], (idx, route)
            terms = (apply_rows(C, rows, [EXPECT.index(idx)], [st[idx]], S) if idx in EXPECT
                     else {r: st[idx] if r == idx else np.zeros(S, dtype=np.uint8) for r in rows})
            for r in rows:
                acc[r] = acc[r] ^ terms[r]
                assert bytes(s.peek(r)) == acc[r].tobytes(), (idx, r)
            assert bytes(s.peek(rows[0], 7 if S > 7 else S)) == acc[rows[0]][:7].tobytes()
        # the rest from eight threads
        c0 = _counters()
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
            list(ex.map(lambda i: s.feed(i, bytes(st[i])), order[5:]))
        assert (_counters() - c0).tolist() == [len(order) - 5] * 2 + [(len(order) - 5) * (route == "staged")]
        for j in compare:  # a clean codeword: every syndrome is zero
            assert not any(s.peek(j)), j
        assert bytes(s.peek(1)) == st[1].tobytes()
        c0 = _counters()
        raised, counts = _finish(s)
        # one final launch; the status words and one span of wanted rows
        assert (_counters() - c0).tolist() == [1, 1, 2]
        assert not raised and counts == [0] * (N_ + 1)
        assert bytes(s.shards[1]) == st[1].tobytes()
        ref_raised, ref_dst, _, _ = _one_shot(S, st, want, compare, False)
        assert not ref_raised and bytes(ref_dst[1]) == bytes(s.shards[1])


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("col", (4096 + 3, 8209))  # in the vector body; in the S % 16 tail
def test_a_corrupt_survivor_is_flagged_or_repaired(col, route, monkeypatch):
    monkeypatch.setenv("CALLFS_RS_SESSION_INPLACE_MAX", ROUTES[route])
    S, bad = 8211, 7
    sh = _stripe(S).copy()
    sh[bad, col] ^= 0x31
    want, compare = (1,), (2, 3, 4)
    implied = _implied(sh)
    assert not np.array_equal(implied[1], _stripe(S)[1])
    order = [int(i) for i in np.random.default_rng(col).permutation(list(EXPECT) + list(compare))]
    # check mode: RS_E_CORRUPT, and the wanted bytes as built from the corrupted survivor
    with _open(S, want, compare) as s:
        for idx in order:
            s.feed(idx, bytes(sh[idx]))
        raised, _ = _finish(s)
        ref_raised, ref_dst, _, _ = _one_shot(S, sh, want, compare, False)
        assert raised and ref_raised
        assert bytes(s.shards[1]) == implied[1].tobytes() == bytes(ref_dst[1])
    # repair mode: the true shard, the survivor's name in counts, the error row in fix
    with _open(S, want, compare, repair=True) as s:
        for idx in order:
            s.feed(idx, bytes(sh[idx]))
        fix = [bytearray(S) if i in EXPECT or i in compare else None for i in range(N_)]
        raised, counts = _finish(s, fix)
        ref_raised, ref_dst, ref_fix, ref_counts = _one_shot(S, sh, want, compare, True)
        assert not raised and not ref_raised
        assert counts == ref_counts == [int(i == bad) for i in range(N_ + 1)]
        assert bytes(s.shards[1]) == _stripe(S)[1].tobytes() == bytes(ref_dst[1])
        error = np.zeros(S, dtype=np.uint8)
        error[col] = 0x31
        for i in range(N_):
            if fix[i] is not None:
                assert bytes(fix[i]) == bytes(ref_fix[i]) == (error if i == bad else np.zeros(S, np.uint8)).tobytes(), i


def test_with_two_compared_shards_repair_only_flags():
    from callfs_amd import erasure as E
    S, bad, col = 8211, 9, 100
    sh = _stripe(S).copy()
    sh[bad, col] ^= 0x80
    want, compare = (1, 4), (2, 3)
    implied = _implied(sh)
    with _open(S, want, compare, repair=True) as s:
        for idx in list(EXPECT) + list(compare):
            s.feed(idx, bytes(sh[idx]))
        with pytest.raises(E.ErrShardCorrupted):
            s.finish()
        ref_raised, ref_dst, _, _ = _one_shot(S, sh, want, compare, True)
        assert ref_raised
        assert s.counts == [0] * N_ + [1]  # one column, unexplained
        for w in want:  # stored as computed from the corrupted survivor
            assert bytes(s.shards[w]) == implied[w].tobytes() == bytes(ref_dst[w]), w


def test_a_compared_shard_that_never_arrives_is_left_out():
    S = 8211
    st = _stripe(S)
    want, compare = (1,), (2, 3, 4)
    with _open(S, want, compare) as s:
        for idx in list(EXPECT) + [2, 4]:
            s.feed(idx, bytes(st[idx]))
        assert bytes(s.peek(3)) == _implied(st)[3].tobytes()  # the implied shard, never compared
        raised, _ = _finish(s)
        assert not raised and bytes(s.shards[1]) == st[1].tobytes()
    ref_raised, ref_dst, _, _ = _one_shot(S, st, want, (2, 4), False)
    assert not ref_raised and bytes(ref_dst[1]) == st[1].tobytes()
    # with no compared shard delivered, finish only copies the wanted rows out
    with _open(S, want, compare) as s:
        for idx in EXPECT:
            s.feed(idx, bytes(st[idx]))
        c0 = _counters()
        raised, _ = _finish(s)
        assert (_counters() - c0).tolist() == [1, 0, 1]
        assert not raised and bytes(s.shards[1]) == st[1].tobytes()


def test_refusals_leave_the_session_usable():
    from callfs_amd import erasure as E
    S = 40
    st = _stripe(S)
    with _open(S, (1,), (2,)) as s:
        for idx in EXPECT[:-1]:
            s.feed(idx, bytes(st[idx]))
        with pytest.raises(E.ErrTooFewShards):  # before the k-th expected feed, compared or not
            s.finish()
        s.feed(2, bytes(st[2]))
        with pytest.raises(E.ErrTooFewShards):
            s.finish()
        with pytest.raises(E.ErrInvalidInput):  # a duplicate feed
            s.feed(EXPECT[0], bytes(st[EXPECT[0]]))
        with pytest.raises(E.ErrInvalidInput):  # neither expected nor compared
            s.feed(3, bytes(st[3]))
        with pytest.raises(E.ErrInvalidInput):  # a wanted shard is not fed
            s.feed(1, bytes(st[1]))
        with pytest.raises(E.ErrInvalidInput):
            s.peek(3)
        with pytest.raises(E.ErrShardSize):
            s.feed(EXPECT[-1], bytes(st[EXPECT[-1]][:-1]))
        s.feed(EXPECT[-1], bytes(st[EXPECT[-1]]))
        assert s.finish() == [0] * (N_ + 1)
        assert bytes(s.shards[1]) == st[1].tobytes()
        with pytest.raises(E.ErrInvalidInput):  # finished
            s.finish()
        assert bytes(s.peek(1)) == st[1].tobytes()


def test_dst_lens_trim_into_a_guarded_buffer():
    S = 8211
    st = _stripe(S)
    with _open(S, (1, 4), (2,)) as s:
        for idx in list(EXPECT) + [2]:
            s.feed(idx, bytes(st[idx]))
        buf = bytearray(b"\x5a" * (2 * S + 64))
        view = memoryview(buf)
        lens = [0] * N_
        lens[1], lens[4] = S - 5, 1
        dst = [None] * N_
        dst[1], dst[4] = view[16:16 + S - 5], view[S + 32:S + 33]
        assert s.finish(dst, lens) == [0] * (N_ + 1)
    want = bytearray(b"\x5a" * (2 * S + 64))
    want[16:16 + S - 5] = st[1][:S - 5].tobytes()
    want[S + 32:S + 33] = st[4][:1].tobytes()
    assert buf == want


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_shards_in_host_alloc_memory_at_odd_offsets(route, monkeypatch):
    from callfs_amd import _native as N
    monkeypatch.setenv("CALLFS_RS_SESSION_INPLACE_MAX", ROUTES[route])
    S = 8211
    st = _stripe(S)
    fed = list(EXPECT) + [2, 3]
    pb = N.PinnedBuffer((len(fed) + 1) * (S + 64) + 1, N.default_context())
    try:
        at = {i: (q * (S + 64)) | 1 for q, i in enumerate(fed)}
        out = (len(fed) * (S + 64)) | 1
        for i in fed:
            pb.array[at[i]:at[i] + S] = st[i]
        pb.array[out - 1:] = 0x5A
        with _open(S, (1,), (2, 3)) as s:
            for i in fed:
                c0 = _counters()
                s.feed(i, pb.array[at[i]:at[i] + S])
                # in place: read where it lies, no copy at all
                assert (_counters() - c0).tolist() == [1, 1, 1 if route == "staged" else 0]
            dst = [None] * N_
            dst[1] = pb.array[out:out + S]
            c0 = _counters()
            assert s.finish(dst) == [0] * (N_ + 1)
            assert (_counters() - c0).tolist() == [1, 1, 2]  # the status words; the row, straight to dst
        assert pb.array[out:out + S].tobytes() == st[1].tobytes()
        assert pb.array[out - 1] == 0x5A and (pb.array[out + S:] == 0x5A).all()
    finally:
        pb.close()


@pytest.mark.parametrize("size", (2, 10 * 8211 - 7, 10 << 20))
@pytest.mark.parametrize("repair", (False, True))
def test_codec_decode_session_round_trips(size, repair):
    from callfs_amd.erasure import Codec, ErasureProfile
    codec, prof = Codec(), ErasureProfile(K, M)
    data = np.random.default_rng(size).integers(0, 256, size, dtype=np.uint8).tobytes()
    shards = [bytes(s) for s in codec.encode(data, prof)]
    expect, compare = [0] + list(range(3, 12)), [12, 13] if not repair else [2, 12, 13]
    with codec.decode_session(prof, size, expect, compare, repair=repair) as ds:
        order = expect + compare
        with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
            list(ex.map(lambda i: ds.feed(i, shards[i]), order))
        got = ds.finish()
    assert bytes(got) == data
    have = [shards[i] if i in order else None for i in range(N_)]
    assert bytes(codec.decode(have, prof, size)) == data
