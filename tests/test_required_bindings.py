"""The Python bindings of the calls that rebuild only the shards a caller asks for
(callfs_amd/erasure.py: reconstruct_some, reconstruct_batch(required=), Codec.decode and
decode_many with data_only), without a GPU: the native entry points are replaced by stand-ins
that record what they were given and rebuild what they were asked for, so what is checked is
the marshalling -- which entries get a buffer, which pointers are NULL, the flags, and which
entries of the caller's lists are replaced."""
import ctypes
import types

import pytest


@pytest.fixture
def fake(native_lib, monkeypatch):
    """Stand-ins for the four native calls. A wanted missing shard is filled with 0xEE and its
    length set; a missing shard with a NULL pointer that the call would write is an error."""
    calls = []

    def rebuild(n, b, ptrs, lens, wanted):
        S = max(lens[b * n + i] for i in range(n))
        for i in range(n):
            if lens[b * n + i] == 0 and wanted(i):
                assert ptrs[b * n + i], ("a wanted shard without a buffer", b, i)
                ctypes.memset(ptrs[b * n + i], 0xEE, S)
                lens[b * n + i] = S
        return S

    def some(ctx, k, m, ptrs, lens, req):
        calls.append(("some", [bool(p) for p in ptrs[:k + m]], list(req[:k + m])))
        rebuild(k + m, 0, ptrs, lens, lambda i: req[i])
        return 0

    def some_batch(ctx, k, m, B, ptrs, lens, req, verify, status):
        n = k + m
        calls.append(("some_batch", [bool(p) for p in ptrs[:B * n]], list(req[:B * n]), verify))
        for b in range(B):
            rebuild(n, b, ptrs, lens, lambda i: req[b * n + i])
            status[b] = 0
        return 0

    def decode_data(ctx, k, m, ptrs, lens, out, size):
        calls.append(("decode_data", [bool(p) for p in ptrs[:k + m]], size))
        rebuild(k + m, 0, ptrs, lens, lambda i: i < k)
        ctypes.memset(out, 0x77, size)
        return 0

    def decode_data_batch(ctx, k, m, B, ptrs, lens, outs, sizes, status):
        n = k + m
        calls.append(("decode_data_batch", [bool(p) for p in ptrs[:B * n]]))
        for b in range(B):
            rebuild(n, b, ptrs, lens, lambda i: i < k)
            ctypes.memset(outs[b], 0x77, sizes[b])
            status[b] = 0
        return 0

    lib = native_lib.lib
    monkeypatch.setattr(lib, "rs_reconstruct_some", some, raising=False)
    monkeypatch.setattr(lib, "rs_reconstruct_some_batch", some_batch, raising=False)
    monkeypatch.setattr(lib, "rs_codec_decode_data", decode_data, raising=False)
    monkeypatch.setattr(lib, "rs_codec_decode_data_batch", decode_data_batch, raising=False)
    return types.SimpleNamespace(calls=calls, ctx=types.SimpleNamespace(handle=ctypes.c_void_p(1)))


def _stripe(n, S, lost):
    return [None if i in lost else bytearray([i + 1]) * S for i in range(n)]


def test_reconstruct_some_marshalling(fake):
    from callfs_amd import reconstruct_some
    k, m, n, S = 4, 2, 6, 40
    sh = _stripe(n, S, (1, 5))
    reconstruct_some(sh, k, m, [False, True, True, False, False, False], context=fake.ctx)
    name, ptrs, req = fake.calls[-1]
    assert name == "some" and req == [0, 1, 1, 0, 0, 0]
    assert ptrs == [True, True, True, True, True, False]  # the unwanted missing shard: NULL
    assert bytes(sh[1]) == b"\xee" * S and sh[5] is None
    assert bytes(sh[0]) == b"\x01" * S
    with pytest.raises(ValueError):
        reconstruct_some(sh, k, m, [True] * 5, context=fake.ctx)


def test_reconstruct_batch_required_marshalling(fake):
    from callfs_amd.erasure import reconstruct_batch
    k, m, n = 4, 2, 6
    stripes = [_stripe(n, 16, (0, 4)), _stripe(n, 100, (3,)), _stripe(n, 7, ())]
    required = [[True, False, False, False, False, False], [False] * n, [True] * n]
    st = reconstruct_batch(stripes, k, m, verify=False, context=fake.ctx, required=required)
    name, ptrs, req, verify = fake.calls[-1]
    assert st == [0, 0, 0] and name == "some_batch" and verify == 0
    assert req == [1, 0, 0, 0, 0, 0] + [0] * n + [1] * n
    assert ptrs == [True, True, True, True, False, True] + [True, True, True, False, True, True] + [True] * n
    assert bytes(stripes[0][0]) == b"\xee" * 16 and stripes[0][4] is None and stripes[1][3] is None
    with pytest.raises(ValueError):
        reconstruct_batch(stripes, k, m, context=fake.ctx, required=required[:2])


def test_decode_data_only_marshalling(fake):
    from callfs_amd import Codec, ErasureProfile
    k, m, n, S = 4, 2, 6, 32
    codec = Codec(context=fake.ctx)
    sh = _stripe(n, S, (2, 4, 5))
    out = codec.decode(sh, ErasureProfile(k, m), 100, data_only=True)
    name, ptrs, size = fake.calls[-1]
    assert name == "decode_data" and size == 100 and bytes(out) == b"\x77" * 100
    assert ptrs == [True, True, True, True, False, False]  # missing parity: no buffer
    assert bytes(sh[2]) == b"\xee" * S and sh[4] is None and sh[5] is None
    objs = [_stripe(n, 8, (0, 5)), _stripe(n, 50, (4,))]
    outs, errs = codec.decode_many(objs, ErasureProfile(k, m), [30, 200], data_only=True)
    name, ptrs = fake.calls[-1]
    assert name == "decode_data_batch" and errs == [None, None]
    assert ptrs == [True, True, True, True, True, False] + [True, True, True, True, False, True]
    assert bytes(outs[0]) == b"\x77" * 30 and bytes(outs[1]) == b"\x77" * 200
    assert bytes(objs[0][0]) == b"\xee" * 8 and objs[0][5] is None and objs[1][4] is None
