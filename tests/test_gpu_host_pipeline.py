"""The host-memory chunk pipeline at sizes where its loops rotate and drain.

The tuning variables are read once per process, so each transport runs in a fresh child
Python process: CALLFS_RS_CHUNK_BYTES=65536 and CALLFS_RS_SMALL_MAX_BYTES=0 make a 240 KB
object five chunks on three slots, once on the staged transport (H2D / kernels / D2H) and
once with CALLFS_RS_INPLACE_PIPELINE=1 (in-place kernels on coherent staging). The child
compares every result byte for byte with the CPU oracle and prints one JSON line of named
checks; the tests here assert them one by one.

  python tests/test_gpu_host_pipeline.py child     # what the child runs
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K, M, N = 4, 2, 6
S_OBJ = 40_003                 # 5 column chunks of 8,192 (the last 7,235 wide)
LEN_OBJ = 4 * S_OBJ - 3        # not a multiple of S: the last data shard is padded
B, S_B = 40, 1_000             # 10 stripes per chunk, 4 chunks
BAD = 23                       # chunk 2, offset 3
EMPTY = 30                     # the mixed batch's stripe of size 0 (after BAD)


def _ptrs(arrs):
    return (ctypes.c_void_p * max(len(arrs), 1))(*[a.ctypes.data if a is not None and a.size else 0
                                                   for a in arrs])


def _child():
    sys.path.insert(0, ROOT)
    from callfs_amd import _native as Nat
    from oracle import cref
    lib, ctx = Nat.lib, Nat.default_context().handle
    rng = np.random.default_rng(0x9157)
    res = {}

    # ---- one object --------------------------------------------------------------------
    data = rng.integers(0, 256, LEN_OBJ, dtype=np.uint8)
    padded = np.zeros(K * S_OBJ, np.uint8)
    padded[:LEN_OBJ] = data
    dsh = [padded[i * S_OBJ:(i + 1) * S_OBJ] for i in range(K)]
    want = np.concatenate(dsh + cref.encode(dsh, K, M))
    out = np.full(N * S_OBJ, 0xA5, np.uint8)
    ss = ctypes.c_size_t(0)
    rc = lib.rs_codec_encode(ctx, K, M, data.ctypes.data, LEN_OBJ, out.ctypes.data, out.size,
                             ctypes.byref(ss))
    res["encode_rc"] = rc
    res["encode_shard_size"] = ss.value
    res["encode_bytes"] = bool(np.array_equal(out, want))

    def decode(missing, flip=None):
        sh = [want[i * S_OBJ:(i + 1) * S_OBJ].copy() for i in range(N)]
        lens = (ctypes.c_size_t * N)(*[S_OBJ] * N)
        for i in missing:
            sh[i][:] = 0x5A
            lens[i] = 0
        if flip:
            sh[flip[0]][flip[1]] ^= 0x10
        obj = np.full(LEN_OBJ, 0xC3, np.uint8)
        rc = lib.rs_codec_decode(ctx, K, M, _ptrs(sh), lens, obj.ctypes.data, LEN_OBJ)
        restored = all(np.array_equal(sh[i], want[i * S_OBJ:(i + 1) * S_OBJ]) for i in missing)
        return rc, restored, bool(np.array_equal(obj, data)), [lens[i] for i in range(N)]

    rc, restored, joined, lens = decode((1, 4))
    res["decode_rc"], res["decode_restored"], res["decode_joined"] = rc, restored, joined
    res["decode_lens"] = lens
    # shard 5 is a present parity beyond the first k present: compared, not used. The flipped
    # byte sits in the last (odd-width) chunk.
    rc, restored, _, _ = decode((1,), flip=(5, 35_000))
    res["corrupt_rc"], res["corrupt_restored"] = rc, restored

    # ---- batches -------------------------------------------------------------------------
    def batch(sizes):
        full = []
        for S in sizes:
            d = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(K)]
            full.append(d + (cref.encode(d, K, M) if S else [np.zeros(0, np.uint8)] * M))
        nb = len(sizes)
        par = [[np.full(S, 0xEE, np.uint8) for _ in range(M)] for S in sizes]
        st = (ctypes.c_int * nb)(*[77] * nb)
        rc = lib.rs_encode_batch(ctx, K, M, nb, (ctypes.c_size_t * nb)(*sizes),
                                 _ptrs([f[i] for f in full for i in range(K)]),
                                 _ptrs([p for ps in par for p in ps]), st)
        enc_ok = all(np.array_equal(par[b][j], full[b][K + j]) for b in range(nb) for j in range(M))
        # shard 0 missing everywhere, one byte of stripe BAD's compared parity flipped
        sh = [[x.copy() for x in f] for f in full]
        lens = (ctypes.c_size_t * (nb * N))(*[S for S in sizes for _ in range(N)])
        for b in range(nb):
            sh[b][0][:] = 0x5A
            lens[b * N] = 0
        sh[BAD][5][sizes[BAD] // 2] ^= 1
        st2 = (ctypes.c_int * nb)(*[77] * nb)
        rc2 = lib.rs_reconstruct_batch(ctx, K, M, nb, _ptrs([x for s in sh for x in s]), lens, 1, st2)
        restored = all(np.array_equal(sh[b][0], full[b][0]) for b in range(nb))
        lens_ok = all(lens[b * N] == sizes[b] for b in range(nb))
        return {"enc_rc": rc, "enc_status": list(st), "enc_bytes": enc_ok, "rec_rc": rc2,
                "rec_status": list(st2), "rec_restored": restored, "rec_lens": lens_ok}

    res["uniform"] = batch([S_B] * B)
    res["mixed"] = batch([0 if b == EMPTY else S_B + (b & 1) for b in range(B)])
    print("RESULT " + json.dumps(res))


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
    sys.exit(0)


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["staged", "inplace"])
def res(request, native_lib):
    env = dict(os.environ, CALLFS_RS_CHUNK_BYTES="65536", CALLFS_RS_SMALL_MAX_BYTES="0")
    env.pop("CALLFS_RS_INPLACE_PIPELINE", None)
    env.pop("CALLFS_RS_SLOTS", None)
    if request.param == "inplace":
        env["CALLFS_RS_INPLACE_PIPELINE"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(lines[0][len("RESULT "):])


def test_object_encode_tees_into_shards_out(res, native_lib):
    assert res["encode_rc"] == native_lib.RS_OK
    assert res["encode_shard_size"] == S_OBJ
    assert res["encode_bytes"]


def test_object_decode_joins_through_the_pipeline(res, native_lib):
    assert res["decode_rc"] == native_lib.RS_OK
    assert res["decode_restored"] and res["decode_joined"]
    assert res["decode_lens"] == [S_OBJ] * N


def test_object_decode_flags_corrupt_parity_and_still_reconstructs(res, native_lib):
    assert res["corrupt_rc"] == native_lib.RS_E_CORRUPT
    assert res["corrupt_restored"]


def test_batch_status_lands_on_the_right_stripe(res, native_lib):
    u = res["uniform"]
    assert u["enc_rc"] == native_lib.RS_OK and u["enc_status"] == [0] * B and u["enc_bytes"]
    want = [native_lib.RS_E_CORRUPT if b == BAD else native_lib.RS_OK for b in range(B)]
    assert u["rec_status"] == want
    assert u["rec_rc"] == native_lib.RS_E_CORRUPT
    assert u["rec_restored"] and u["rec_lens"]


def test_batch_of_two_sizes_and_an_empty_stripe(res, native_lib):
    x = res["mixed"]
    no_data = [native_lib.RS_E_NO_DATA if b == EMPTY else native_lib.RS_OK for b in range(B)]
    assert x["enc_status"] == no_data and x["enc_bytes"]
    assert x["enc_rc"] == native_lib.RS_E_NO_DATA
    want = list(no_data)
    want[BAD] = native_lib.RS_E_CORRUPT
    assert x["rec_status"] == want
    assert x["rec_rc"] == native_lib.RS_E_CORRUPT  # the first error in stripe order
    assert x["rec_restored"] and x["rec_lens"]
