"""The correction rule of correct plans (callfs_amd/csrc/locate_tables.hpp
locate_correct, the function rs_apply_correct runs) built with g++ under AddressSanitizer+UBSan
and run on the CPU as a stand-alone program, and the C ABI's side of it: the header declares
the new calls, the library exports them and their argument errors come back without a device,
in rs_plan_create_locate's and rs_locate_batch's order."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "correct_host_test.cpp")
INC = os.path.join(ROOT, "callfs_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "callfs_rs.h")

CALLS = ("rs_plan_create_correct", "rs_correct", "rs_correct_batch", "rs_codec_decode_correct")


def test_correct_rule_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "correct_host_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", INC, SRC,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "correct_host_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


def test_header_declares_and_library_exports_the_correct_calls(native_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "#define RS_ORDER_CORRECT 16384" in text
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(native_lib.lib, name), name
        assert name in native_lib.SIGNATURES, name
    # the plan constructor takes rs_plan_create_locate's arguments, the batch call rs_locate_batch's
    assert native_lib.SIGNATURES["rs_plan_create_correct"] == native_lib.SIGNATURES["rs_plan_create_locate"]
    assert native_lib.SIGNATURES["rs_correct_batch"] == native_lib.SIGNATURES["rs_locate_batch"]
    assert native_lib.SIGNATURES["rs_correct"] == native_lib.SIGNATURES["rs_locate"]
    assert native_lib.SIGNATURES["rs_codec_decode_correct"] == native_lib.SIGNATURES["rs_codec_decode_heal"]


def test_correct_argument_errors_without_device(native_lib):
    """The profile, NULL and count errors come before any device work, and every one is the
    locate sibling's answer to the same arguments."""
    L, N = native_lib.lib, native_lib
    h = ctypes.c_void_p()
    fake_ctx = ctypes.c_void_p(1)  # never dereferenced on these paths
    szs = (ctypes.c_size_t * 1)(16)
    zero = (ctypes.c_size_t * 1)(0)
    ptrs = (ctypes.c_void_p * 6)()
    flags = (ctypes.c_uint8 * 6)(1, 1, 1, 1, 1, 0)
    ref = ctypes.byref(h)
    plan_cases = [
        ((fake_ctx, 0, 0, 2, 1, szs, flags, ptrs, ref), N.RS_E_INVALID_PROFILE),
        ((fake_ctx, 0, 4, 0, 1, szs, flags, ptrs, ref), N.RS_E_INVALID_PROFILE),
        ((fake_ctx, 0, 200, 100, 1, szs, flags, ptrs, ref), N.RS_E_UNSUPPORTED),
        # the profile is looked at first: unsupported wins over a NULL context
        ((None, 0, 200, 100, 1, szs, flags, ptrs, ref), N.RS_E_UNSUPPORTED),
        ((None, 0, 4, 2, 1, szs, flags, ptrs, ref), N.RS_E_ARG),
        ((fake_ctx, 0, 4, 2, 0, szs, flags, ptrs, ref), N.RS_E_ARG),
        ((fake_ctx, 0, 4, 2, 1, None, flags, ptrs, ref), N.RS_E_ARG),
        ((fake_ctx, 0, 4, 2, 1, szs, flags, None, ref), N.RS_E_ARG),
        ((fake_ctx, 0, 4, 2, 1, szs, flags, ptrs, None), N.RS_E_ARG),
        # NULL arguments are found before the sizes are read
        ((fake_ctx, 0, 4, 2, 1, zero, flags, None, ref), N.RS_E_ARG),
        ((fake_ctx, 0, 4, 2, 1, zero, flags, ptrs, ref), N.RS_E_NO_DATA),
    ]
    for args, want in plan_cases:
        assert L.rs_plan_create_correct(*args) == want, args
        assert L.rs_plan_create_locate(*args) == want, args

    counts = (ctypes.c_uint64 * 7)()
    lens = (ctypes.c_size_t * 6)(16, 16, 16, 16, 16, 16)
    status = (ctypes.c_int * 1)()
    flags6 = (ctypes.c_uint8 * 6)()
    out = (ctypes.c_uint8 * 64)()
    one_cases = [
        ((fake_ctx, 0, 2, ptrs, lens, counts), N.RS_E_INVALID_PROFILE),
        ((fake_ctx, 200, 100, ptrs, lens, counts), N.RS_E_UNSUPPORTED),
        ((None, 200, 100, ptrs, lens, counts), N.RS_E_UNSUPPORTED),
        ((None, 4, 2, ptrs, lens, counts), N.RS_E_ARG),
        ((fake_ctx, 4, 2, None, lens, counts), N.RS_E_ARG),
        ((fake_ctx, 4, 2, ptrs, None, counts), N.RS_E_ARG),
        ((fake_ctx, 4, 2, ptrs, lens, None), N.RS_E_ARG),
    ]
    for args, want in one_cases:
        assert L.rs_correct(*args) == want, args
        assert L.rs_locate(*args) == want, args
    batch_cases = [
        ((fake_ctx, 4, 0, 1, ptrs, lens, counts, status), N.RS_E_INVALID_PROFILE),
        ((fake_ctx, 200, 100, 1, ptrs, lens, counts, status), N.RS_E_UNSUPPORTED),
        ((None, 200, 100, 1, ptrs, lens, counts, status), N.RS_E_UNSUPPORTED),
        ((None, 4, 2, 1, ptrs, lens, counts, status), N.RS_E_ARG),
        ((fake_ctx, 4, 2, -1, ptrs, lens, counts, status), N.RS_E_ARG),
        ((fake_ctx, 4, 2, 1, None, lens, counts, status), N.RS_E_ARG),
        ((fake_ctx, 4, 2, 1, ptrs, None, counts, status), N.RS_E_ARG),
        ((fake_ctx, 4, 2, 1, ptrs, lens, None, status), N.RS_E_ARG),
        ((fake_ctx, 4, 2, 1, ptrs, lens, counts, None), N.RS_E_ARG),
        ((fake_ctx, 4, 2, 0, None, None, None, None), N.RS_OK),
    ]
    for args, want in batch_cases:
        assert L.rs_correct_batch(*args) == want, args
        assert L.rs_locate_batch(*args) == want, args
    codec_cases = [
        ((fake_ctx, 0, 2, ptrs, lens, out, 64, flags6), N.RS_E_INVALID_PROFILE),
        ((fake_ctx, 200, 100, ptrs, lens, out, 64, flags6), N.RS_E_UNSUPPORTED),
        ((None, 4, 2, ptrs, lens, out, 64, flags6), N.RS_E_ARG),
        ((fake_ctx, 4, 2, None, lens, out, 64, flags6), N.RS_E_ARG),
        ((fake_ctx, 4, 2, ptrs, None, out, 64, flags6), N.RS_E_ARG),
        ((fake_ctx, 4, 2, ptrs, lens, out, -1, flags6), N.RS_E_ARG),
        ((fake_ctx, 4, 2, ptrs, lens, None, 64, flags6), N.RS_E_ARG),
        ((fake_ctx, 4, 2, ptrs, lens, out, 64, None), N.RS_E_ARG),
    ]
    for args, want in codec_cases:
        assert L.rs_codec_decode_correct(*args) == want, args
        assert L.rs_codec_decode_heal(*args) == want, args


def test_stripe_errors_of_the_correct_calls_without_device(native_lib):
    """Per-stripe shard checks are rs_locate_batch's, and a call in which no stripe runs reaches
    no device: a stripe of exactly k present shards is RS_OK with zero counts, and no shard byte
    is touched."""
    L, N = native_lib.lib, native_lib
    fake_ctx = ctypes.c_void_p(1)  # no stripe runs: never dereferenced
    k, m, n = 4, 2, 6
    bufs = [ctypes.create_string_buffer(bytes([0x30 + i]) * 16, 16) for i in range(n)]
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
    rc = L.rs_correct_batch(fake_ctx, k, m, B, ptrs, lens, counts, status)
    assert list(status) == [want for _, want in rows]
    assert rc == N.RS_E_NO_DATA  # the first nonzero status in stripe order
    assert list(counts) == [0] * (B * (n + 1))
    ref_counts = (ctypes.c_uint64 * (B * (n + 1)))()
    ref_status = (ctypes.c_int * B)()
    assert L.rs_locate_batch(fake_ctx, k, m, B, ptrs, lens, ref_counts, ref_status) == rc
    assert list(ref_status) == list(status)
    one = (ctypes.c_uint64 * (n + 1))(*([9] * (n + 1)))
    assert L.rs_correct(fake_ctx, k, m, ptrs, lens, one) == N.RS_OK and list(one) == [0] * (n + 1)
    for i, b in enumerate(bufs):
        assert b.raw == bytes([0x30 + i]) * 16
