"""The pair rule of locate plans and its tables (DESIGN.md §5.12.1:
callfs_amd/csrc/locate_tables.hpp locate_classify2 and build_locate_tables with max_errors = 2)
built with g++ under AddressSanitizer+UBSan and run on the CPU as a stand-alone program, and
the C ABI's side of it: the header declares the five _ex calls, the library exports them and
their argument errors, max_errors 0 and 3 among them, come back without a device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "locate2_host_test.cpp")
INC = os.path.join(ROOT, "callfs_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "callfs_rs.h")

CALLS = ("rs_plan_create_locate_ex", "rs_locate_ex", "rs_locate_batch_ex", "rs_heal_batch_ex",
         "rs_codec_decode_heal_ex")


def test_pair_rule_and_tables_under_sanitizer(tmp_path):
    """Every check of locate2_host_test.cpp runs locate_classify2 in each packing width that
    holds the pattern's rows (1, 2 and 4 words) and requires the widths to agree."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "locate2_host_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", INC, SRC,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "locate2_host_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr
    got = dict(zip(lines[-2].split()[0::2], map(int, lines[-2].split()[1::2])))
    assert got["pairs"] >= 91 * 255 * 255 and got["singles"] > 0 and got["multis"] > 0 and got["short"] > 0


def test_header_declares_and_library_exports_the_ex_calls(native_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(native_lib.lib, name), name
        assert name in native_lib.SIGNATURES, name
        # each takes its sibling's arguments plus one int
        sib = native_lib.SIGNATURES[name[:-3]][1]
        args = list(native_lib.SIGNATURES[name][1])
        at = len(args) - 2 if name == "rs_plan_create_locate_ex" else len(args) - 1
        assert args[at] is ctypes.c_int
        assert args[:at] + args[at + 1:] == list(sib), name


def test_ex_argument_errors_without_device(native_lib):
    """The profile, NULL, count and max_errors errors come before any device work:
    max_errors < 1 is RS_E_ARG, max_errors > 2 RS_E_UNSUPPORTED."""
    L, N = native_lib.lib, native_lib
    h = ctypes.c_void_p()
    fake_ctx = ctypes.c_void_p(1)  # never dereferenced on these paths
    szs = (ctypes.c_size_t * 1)(16)
    bufs = [ctypes.create_string_buffer(16) for _ in range(6)]
    ptrs = (ctypes.c_void_p * 6)(*[ctypes.addressof(b) for b in bufs])
    flags = (ctypes.c_uint8 * 6)(1, 1, 1, 1, 1, 0)
    create = L.rs_plan_create_locate_ex
    for me in (1, 2):
        assert create(fake_ctx, 0, 0, 2, 1, szs, flags, ptrs, me, ctypes.byref(h)) == N.RS_E_INVALID_PROFILE
        assert create(fake_ctx, 0, 200, 100, 1, szs, flags, ptrs, me, ctypes.byref(h)) == N.RS_E_UNSUPPORTED
        assert create(None, 0, 4, 2, 1, szs, flags, ptrs, me, ctypes.byref(h)) == N.RS_E_ARG
        assert create(fake_ctx, 0, 4, 2, 0, szs, flags, ptrs, me, ctypes.byref(h)) == N.RS_E_ARG
        assert create(fake_ctx, 0, 4, 2, 1, None, flags, ptrs, me, ctypes.byref(h)) == N.RS_E_ARG
        assert create(fake_ctx, 0, 4, 2, 1, szs, flags, None, me, ctypes.byref(h)) == N.RS_E_ARG
        assert create(fake_ctx, 0, 4, 2, 1, szs, flags, ptrs, me, None) == N.RS_E_ARG
        zero = (ctypes.c_size_t * 1)(0)
        assert create(fake_ctx, 0, 4, 2, 1, zero, flags, ptrs, me, ctypes.byref(h)) == N.RS_E_NO_DATA
    for me in (0, -1):
        assert create(fake_ctx, 0, 4, 2, 1, szs, flags, ptrs, me, ctypes.byref(h)) == N.RS_E_ARG
    for me in (3, 16):
        assert create(fake_ctx, 0, 4, 2, 1, szs, flags, ptrs, me, ctypes.byref(h)) == N.RS_E_UNSUPPORTED
    assert create(fake_ctx, 0, 0, 2, 1, szs, flags, ptrs, 3, ctypes.byref(h)) == N.RS_E_INVALID_PROFILE
    assert create(None, 0, 4, 2, 1, szs, flags, ptrs, 3, ctypes.byref(h)) == N.RS_E_ARG

    counts = (ctypes.c_uint64 * 7)()
    lens = (ctypes.c_size_t * 6)(16, 16, 16, 16, 16, 16)
    status = (ctypes.c_int * 1)()
    healed = (ctypes.c_uint8 * 6)()
    out = (ctypes.c_uint8 * 64)()
    for me in (1, 2):
        assert L.rs_locate_ex(fake_ctx, 0, 2, ptrs, lens, counts, me) == N.RS_E_INVALID_PROFILE
        assert L.rs_locate_ex(fake_ctx, 200, 100, ptrs, lens, counts, me) == N.RS_E_UNSUPPORTED
        assert L.rs_locate_ex(None, 4, 2, ptrs, lens, counts, me) == N.RS_E_ARG
        assert L.rs_locate_ex(fake_ctx, 4, 2, None, lens, counts, me) == N.RS_E_ARG
        assert L.rs_locate_ex(fake_ctx, 4, 2, ptrs, None, counts, me) == N.RS_E_ARG
        assert L.rs_locate_ex(fake_ctx, 4, 2, ptrs, lens, None, me) == N.RS_E_ARG
        assert L.rs_locate_batch_ex(fake_ctx, 4, 0, 1, ptrs, lens, counts, status, me) == N.RS_E_INVALID_PROFILE
        assert L.rs_locate_batch_ex(None, 4, 2, 1, ptrs, lens, counts, status, me) == N.RS_E_ARG
        assert L.rs_locate_batch_ex(fake_ctx, 4, 2, -1, ptrs, lens, counts, status, me) == N.RS_E_ARG
        assert L.rs_locate_batch_ex(fake_ctx, 4, 2, 1, ptrs, lens, None, status, me) == N.RS_E_ARG
        assert L.rs_locate_batch_ex(fake_ctx, 4, 2, 1, ptrs, lens, counts, None, me) == N.RS_E_ARG
        assert L.rs_locate_batch_ex(fake_ctx, 4, 2, 0, None, None, None, None, me) == N.RS_OK
        assert L.rs_heal_batch_ex(fake_ctx, 0, 2, 1, ptrs, lens, healed, status, me) == N.RS_E_INVALID_PROFILE
        assert L.rs_heal_batch_ex(None, 4, 2, 1, ptrs, lens, healed, status, me) == N.RS_E_ARG
        assert L.rs_heal_batch_ex(fake_ctx, 4, 2, -1, ptrs, lens, healed, status, me) == N.RS_E_ARG
        assert L.rs_heal_batch_ex(fake_ctx, 4, 2, 1, ptrs, lens, None, status, me) == N.RS_E_ARG
        assert L.rs_heal_batch_ex(fake_ctx, 4, 2, 0, None, None, None, None, me) == N.RS_OK
        assert L.rs_codec_decode_heal_ex(fake_ctx, 0, 2, ptrs, lens, out, 64, healed, me) == N.RS_E_INVALID_PROFILE
        assert L.rs_codec_decode_heal_ex(None, 4, 2, ptrs, lens, out, 64, healed, me) == N.RS_E_ARG
        assert L.rs_codec_decode_heal_ex(fake_ctx, 4, 2, ptrs, lens, out, -1, healed, me) == N.RS_E_ARG
        assert L.rs_codec_decode_heal_ex(fake_ctx, 4, 2, ptrs, lens, None, 64, healed, me) == N.RS_E_ARG
        assert L.rs_codec_decode_heal_ex(fake_ctx, 4, 2, ptrs, lens, out, 64, None, me) == N.RS_E_ARG
    # max_errors itself: every pointer valid, no device reached
    for me, want in ((0, N.RS_E_ARG), (-5, N.RS_E_ARG), (3, N.RS_E_UNSUPPORTED), (255, N.RS_E_UNSUPPORTED)):
        assert L.rs_locate_ex(fake_ctx, 4, 2, ptrs, lens, counts, me) == want
        assert L.rs_locate_batch_ex(fake_ctx, 4, 2, 1, ptrs, lens, counts, status, me) == want
        assert L.rs_locate_batch_ex(fake_ctx, 4, 2, 0, None, None, None, None, me) == want
        assert L.rs_heal_batch_ex(fake_ctx, 4, 2, 1, ptrs, lens, healed, status, me) == want
        assert L.rs_heal_batch_ex(fake_ctx, 4, 2, 0, None, None, None, None, me) == want
        assert L.rs_codec_decode_heal_ex(fake_ctx, 4, 2, ptrs, lens, out, 64, healed, me) == want
    # the profile comes first, a NULL before "unsupported"
    assert L.rs_locate_ex(fake_ctx, 0, 2, ptrs, lens, counts, 3) == N.RS_E_INVALID_PROFILE
    assert L.rs_locate_ex(None, 4, 2, ptrs, lens, counts, 3) == N.RS_E_ARG
    assert L.rs_heal_batch_ex(fake_ctx, 4, 2, 1, ptrs, lens, None, status, 3) == N.RS_E_ARG


def test_stripe_errors_of_the_ex_calls_without_device(native_lib):
    """Per-stripe shard checks equal the single calls': a call in which no stripe runs reaches
    no device, with either max_errors."""
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
    for me in (1, 2):
        counts = (ctypes.c_uint64 * (B * (n + 1)))(*([7] * (B * (n + 1))))
        status = (ctypes.c_int * B)()
        rc = L.rs_locate_batch_ex(fake_ctx, k, m, B, ptrs, lens, counts, status, me)
        assert list(status) == [want for _, want in rows]
        assert rc == N.RS_E_NO_DATA  # the first nonzero status in stripe order
        assert list(counts) == [0] * (B * (n + 1))
        one = (ctypes.c_uint64 * (n + 1))(*([9] * (n + 1)))
        assert L.rs_locate_ex(fake_ctx, k, m, ptrs, lens, one, me) == N.RS_OK and list(one) == [0] * (n + 1)
