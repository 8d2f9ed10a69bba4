"""rs_codec_encode with `shards_out` placed against `data` in every way the header allows: in
place, disjoint, and partly overlapping from below and from above. Split's shape of the single
object call is codec_batch.hpp's (split_prepare moves an overlapping object before the pipeline
reads it), and no other test reaches the overlapping placements.

The shards and `shard_size` equal the CPU oracle's Split + Encode (oracle.cref) byte for byte,
and no byte outside `shards_out` changes. At length 1 there is no byte to share from above:
that placement abuts the object instead.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 64


def _env():
    sys.path.insert(0, ROOT)
    from callfs_amd import _native as Nat
    from oracle import cref
    return Nat, cref


@functools.lru_cache(maxsize=None)
def _ref(k, m, length):
    """(object, S, the n shards back to back) from the oracle; shared, never written."""
    _, cref = _env()
    obj = np.random.default_rng(1000 * k + length).integers(0, 256, length, dtype=np.uint8)
    S = -(-length // k)
    padded = np.zeros(k * S, np.uint8)
    padded[:length] = obj
    data = [padded[i * S:(i + 1) * S].copy() for i in range(k)]
    flat = np.concatenate(data + [np.ascontiguousarray(p) for p in cref.encode(data, k, m)])
    flat.setflags(write=False)
    obj.setflags(write=False)
    return obj, S, flat


@pytest.fixture(scope="module")
def cx():
    Nat, _ = _env()
    c = Nat.Context(1)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("place", ["below", "above", "inplace", "disjoint"])
@pytest.mark.parametrize("length", ["1", "k+1", "4099"])
@pytest.mark.parametrize("k,m", [(4, 2), (10, 4)])
def test_codec_encode_where_shards_out_meets_data(cx, k, m, length, place):
    Nat, _ = _env()
    L = {"1": 1, "k+1": k + 1, "4099": 4099}[length]
    obj, S, flat = _ref(k, m, L)
    need = S * (k + m)
    data_off = SENT + need  # room for shards_out below the object
    out_off = {"below": data_off - min(L // 2 + 1, need - 1),  # ends inside the object or past it
               "above": data_off + max(1, L // 2),             # starts inside the object
               "inplace": data_off,
               "disjoint": data_off + L + 7}[place]
    if place in ("below", "above") and L > 1:
        assert out_off != data_off and out_off < data_off + L and data_off < out_off + need
    arena = np.full(max(data_off + L, out_off + need) + SENT, 0xA5, np.uint8)
    arena[data_off:data_off + L] = obj
    before = arena.copy()
    base = arena.ctypes.data
    size = ctypes.c_size_t(12345)
    rc = Nat.lib.rs_codec_encode(cx.handle, k, m, base + data_off, L, base + out_off, need,
                                 ctypes.byref(size))
    assert rc == 0 and size.value == S
    assert arena[out_off:out_off + need].tobytes() == flat.tobytes()
    # only shards_out is written: the sentinels, and the object's bytes outside it, stay
    assert (arena[:out_off] == before[:out_off]).all()
    assert (arena[out_off + need:] == before[out_off + need:]).all()
