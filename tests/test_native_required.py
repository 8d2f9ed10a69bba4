"""Host-side tables of required device plans (decode_plan with a wanted set,
callfs_amd/csrc/mixed_tables.hpp build_mixed_tables, ragged_tables.hpp build_ragged_tables
with a wanted set) built with g++ under AddressSanitizer+UBSan and run on the CPU as a
stand-alone program, and the C ABI's side of it: the header declares the new calls and the
library exports them."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "required_host_test.cpp")
INC = os.path.join(ROOT, "callfs_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "callfs_rs.h")


def test_required_tables_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "required_host_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", INC, SRC,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "required_host_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


def test_header_declares_and_library_exports_the_required_calls(native_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "#define RS_ORDER_REQUIRED 2048" in text
    for name in ("rs_plan_create_required", "rs_decode_dev_required"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(native_lib.lib, name), name
        assert name in native_lib.SIGNATURES, name
    # without a device: argument and profile errors come before any device work
    import ctypes
    L, N = native_lib.lib, native_lib
    h = ctypes.c_void_p()
    fake_ctx = ctypes.c_void_p(1)  # never dereferenced on these paths
    szs = (ctypes.c_size_t * 1)(16)
    ptrs = (ctypes.c_void_p * 6)()
    flags = (ctypes.c_uint8 * 6)(1, 1, 1, 1, 0, 0)
    assert L.rs_plan_create_required(fake_ctx, 0, 0, 2, 1, szs, flags, flags, ptrs,
                                     ctypes.byref(h)) == N.RS_E_INVALID_PROFILE
    assert L.rs_plan_create_required(fake_ctx, 0, 200, 100, 1, szs, flags, flags, ptrs,
                                     ctypes.byref(h)) == N.RS_E_UNSUPPORTED
    assert L.rs_plan_create_required(None, 0, 4, 2, 1, szs, flags, flags, ptrs,
                                     ctypes.byref(h)) == N.RS_E_ARG
    assert L.rs_plan_create_required(fake_ctx, 0, 4, 2, 0, szs, flags, flags, ptrs,
                                     ctypes.byref(h)) == N.RS_E_ARG
    assert L.rs_plan_create_required(fake_ctx, 0, 4, 2, 1, None, flags, flags, ptrs,
                                     ctypes.byref(h)) == N.RS_E_ARG
    assert L.rs_plan_create_required(fake_ctx, 0, 4, 2, 1, szs, flags, flags, ptrs, None) == N.RS_E_ARG
