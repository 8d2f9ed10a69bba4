"""Host-side tables of locate plans and the classification rule the kernel runs (DESIGN.md
§5.12: callfs_amd/csrc/locate_tables.hpp build_locate_tables and locate_classify) built with
g++ under AddressSanitizer+UBSan and run on the CPU as a stand-alone program, and the C ABI's
side of it: the header declares the new calls, the library exports them and their argument
errors come back without a device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "locate_host_test.cpp")
INC = os.path.join(ROOT, "callfs_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "callfs_rs.h")

CALLS = ("rs_plan_create_locate", "rs_plan_blame", "rs_locate", "rs_locate_batch", "rs_heal_batch",
         "rs_codec_decode_heal")


def test_locate_tables_and_rule_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "locate_host_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", INC, SRC,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "locate_host_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


def test_header_declares_and_library_exports_the_locate_calls(native_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "#define RS_ORDER_LOCATE 8192" in text
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(native_lib.lib, name), name
        assert name in native_lib.SIGNATURES, name


def test_locate_argument_errors_without_device(native_lib):
    """The profile, NULL and count errors come before any device work."""
    L, N = native_lib.lib, native_lib
    h = ctypes.c_void_p()
    fake_ctx = ctypes.c_void_p(1)  # never dereferenced on these paths
    szs = (ctypes.c_size_t * 1)(16)
    ptrs = (ctypes.c_void_p * 6)()
    flags = (ctypes.c_uint8 * 6)(1, 1, 1, 1, 1, 0)
    create = L.rs_plan_create_locate
    assert create(fake_ctx, 0, 0, 2, 1, szs, flags, ptrs, ctypes.byref(h)) == N.RS_E_INVALID_PROFILE
    assert create(fake_ctx, 0, 200, 100, 1, szs, flags, ptrs, ctypes.byref(h)) == N.RS_E_UNSUPPORTED
    assert create(None, 0, 4, 2, 1, szs, flags, ptrs, ctypes.byref(h)) == N.RS_E_ARG
    assert create(fake_ctx, 0, 4, 2, 0, szs, flags, ptrs, ctypes.byref(h)) == N.RS_E_ARG
    assert create(fake_ctx, 0, 4, 2, 1, None, flags, ptrs, ctypes.byref(h)) == N.RS_E_ARG
    assert create(fake_ctx, 0, 4, 2, 1, szs, flags, None, ctypes.byref(h)) == N.RS_E_ARG
    assert create(fake_ctx, 0, 4, 2, 1, szs, flags, ptrs, None) == N.RS_E_ARG
    zero = (ctypes.c_size_t * 1)(0)
    assert create(fake_ctx, 0, 4, 2, 1, zero, flags, ptrs, ctypes.byref(h)) == N.RS_E_NO_DATA
    counts = (ctypes.c_uint64 * 7)()
    assert L.rs_plan_blame(None, None, counts) == N.RS_E_ARG
    assert L.rs_plan_blame(fake_ctx, None, None) == N.RS_E_ARG

    lens = (ctypes.c_size_t * 6)(16, 16, 16, 16, 16, 16)
    status = (ctypes.c_int * 1)()
    healed = (ctypes.c_uint8 * 6)()
    out = (ctypes.c_uint8 * 64)()
    assert L.rs_locate(fake_ctx, 0, 2, ptrs, lens, counts) == N.RS_E_INVALID_PROFILE
    assert L.rs_locate(fake_ctx, 200, 100, ptrs, lens, counts) == N.RS_E_UNSUPPORTED
    assert L.rs_locate(None, 4, 2, ptrs, lens, counts) == N.RS_E_ARG
    assert L.rs_locate(fake_ctx, 4, 2, None, lens, counts) == N.RS_E_ARG
    assert L.rs_locate(fake_ctx, 4, 2, ptrs, None, counts) == N.RS_E_ARG
    assert L.rs_locate(fake_ctx, 4, 2, ptrs, lens, None) == N.RS_E_ARG
    assert L.rs_locate_batch(fake_ctx, 4, 0, 1, ptrs, lens, counts, status) == N.RS_E_INVALID_PROFILE
    assert L.rs_locate_batch(None, 4, 2, 1, ptrs, lens, counts, status) == N.RS_E_ARG
    assert L.rs_locate_batch(fake_ctx, 4, 2, -1, ptrs, lens, counts, status) == N.RS_E_ARG
    assert L.rs_locate_batch(fake_ctx, 4, 2, 1, ptrs, lens, None, status) == N.RS_E_ARG
    assert L.rs_locate_batch(fake_ctx, 4, 2, 1, ptrs, lens, counts, None) == N.RS_E_ARG
    assert L.rs_locate_batch(fake_ctx, 4, 2, 0, None, None, None, None) == N.RS_OK
    assert L.rs_heal_batch(fake_ctx, 0, 2, 1, ptrs, lens, healed, status) == N.RS_E_INVALID_PROFILE
    assert L.rs_heal_batch(None, 4, 2, 1, ptrs, lens, healed, status) == N.RS_E_ARG
    assert L.rs_heal_batch(fake_ctx, 4, 2, -1, ptrs, lens, healed, status) == N.RS_E_ARG
    assert L.rs_heal_batch(fake_ctx, 4, 2, 1, ptrs, lens, None, status) == N.RS_E_ARG
    assert L.rs_heal_batch(fake_ctx, 4, 2, 0, None, None, None, None) == N.RS_OK
    assert L.rs_codec_decode_heal(fake_ctx, 0, 2, ptrs, lens, out, 64, healed) == N.RS_E_INVALID_PROFILE
    assert L.rs_codec_decode_heal(None, 4, 2, ptrs, lens, out, 64, healed) == N.RS_E_ARG
    assert L.rs_codec_decode_heal(fake_ctx, 4, 2, ptrs, lens, out, -1, healed) == N.RS_E_ARG
    assert L.rs_codec_decode_heal(fake_ctx, 4, 2, ptrs, lens, None, 64, healed) == N.RS_E_ARG
    assert L.rs_codec_decode_heal(fake_ctx, 4, 2, ptrs, lens, out, 64, None) == N.RS_E_ARG


def test_stripe_errors_of_the_host_calls_without_device(native_lib):
    """Per-stripe shard checks are rs_reconstruct_batch's, and a call in which no stripe runs
    reaches no device: a stripe of exactly k present shards is RS_OK with zero counts."""
    L, N = native_lib.lib, native_lib
    fake_ctx = ctypes.c_void_p(1)  # no stripe runs: never dereferenced
    k, m, n = 4, 2, 6
    bufs = [ctypes.create_string_buffer(16) for _ in range(n)]
    rows = [
        ([16] * 4 + [0, 0], N.RS_OK),               # exactly k present: nothing to compare
        ([0] * 6, N.RS_E_NO_DATA),
        ([16, 16, 8, 16, 16, 16], N.RS_E_SHARD_SIZE),
        ([16, 16, 16, 0, 0, 0], N.RS_E_TOO_FEW_SHARDS),
    ]
    B = len(rows)
    ptrs = (ctypes.c_void_p * (B * n))(*[ctypes.addressof(b) for _ in range(B) for b in bufs])
    lens = (ctypes.c_size_t * (B * n))(*[x for r, _ in rows for x in r])
    counts = (ctypes.c_uint64 * (B * (n + 1)))(*([7] * (B * (n + 1))))
    status = (ctypes.c_int * B)()
    rc = L.rs_locate_batch(fake_ctx, k, m, B, ptrs, lens, counts, status)
    assert list(status) == [want for _, want in rows]
    assert rc == N.RS_E_NO_DATA  # the first nonzero status in stripe order
    assert list(counts) == [0] * (B * (n + 1))
    one = (ctypes.c_uint64 * (n + 1))(*([9] * (n + 1)))
    assert L.rs_locate(fake_ctx, k, m, ptrs, lens, one) == N.RS_OK and list(one) == [0] * (n + 1)
