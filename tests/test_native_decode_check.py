"""The CPU side of the decode-check plans: the host tables
(callfs_amd/csrc/decode_check_tables.hpp) built with g++ under ASan + UBSan and run as a
stand-alone program; what a decode-check plan dispatches, on host-only builds of the plan code and
the kernel files linked against the recording HIP stand-ins (also under ASan + UBSan, also
stand-alone: nothing sanitized is loaded into Python); the header and the exports; the profile and
argument errors without a device; and the registers the build recorded for the new kernels."""
import concurrent.futures
import ctypes
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "callfs_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "callfs_rs.h")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-fno-omit-frame-pointer"]


def test_decode_check_tables_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "decode_check_host_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + SANITIZE + ["-I", CSRC,
                    os.path.join(NATIVE, "decode_check_host_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "decode_check_host_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


def test_routes_dispatch_the_check_kernel(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sources = [os.path.join(CSRC, f) for f in ("rs_kernels.hip", "rs_mixed.hip", "sha256.hip",
                                               "rs_plan.cpp", "rs_context.cpp")] + [
        os.path.join(NATIVE, f) for f in ("decode_check_routes.cpp", "fake_hip_runtime.cpp", "fake_hip_memory.cpp")]
    flags = ["--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC, "-I", NATIVE] + SANITIZE

    def compile_one(src):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.run(["hipcc"] + flags + ["-x", "hip", "-c", src, "-o", obj], check=True)
        return obj

    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(compile_one, sources))
    # host-only compilation leaves the fat binaries' data symbols undefined: 0 at link time
    undefined = subprocess.run(["nm", "-u"] + objs, check=True, capture_output=True, text=True).stdout
    fatbin = sorted({w for w in undefined.split() if w.startswith("__hip_fatbin_")})
    exe = str(tmp_path / "decode_check_routes")
    subprocess.run(["hipcc"] + SANITIZE + objs + ["-o", exe, "-no-pie"] +
                   ["-Wl,--defsym=%s=0" % s for s in fatbin], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CALLFS_RS_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "decode_check_routes ok", r.stdout[-2000:] + r.stderr[-4000:]
    cases, name = {}, None
    for line in lines[:-1]:
        w = line.split()
        if w[0] == "case":
            name = w[1].rstrip(":")
            cases[name] = []
        else:
            assert w[0] == "dispatch", line
            cases[name].append(w[1])

    def instance(symbol):
        """(kernel, RT, STORE) of a mangled rs_check_ragged / rs_merge_ragged<RT, Policy, STORE>."""
        mo = re.search(r"15rs_(check|merge)_raggedILi(\d+)E.*Lb([01])EEEv", symbol)
        assert mo, symbol
        return mo.group(1), int(mo.group(2)), bool(int(mo.group(3)))

    got = {name: [instance(s) for s in syms] for name, syms in cases.items()}
    assert got == {
        # a final plan: rs_check_ragged once per group of 16 rows, in the smallest instance that
        # holds the group's rows
        "final-merge": [("check", 4, False)], "final-store": [("check", 4, True)],
        "final-merge-8": [("check", 8, False)], "final-store-8": [("check", 8, True)],
        "final-merge-two-groups": [("check", 16, False), ("check", 4, False)],
        "final-store-two-groups": [("check", 16, True), ("check", 4, True)],
        # a final stripe with nothing delivered is dispatched (two rows: one wanted, one check)
        "final-nothing-delivered": [("check", 4, False)],
        # a non-final plan: a check row is an ordinary row of the decode-idx kernels
        "merge": [("merge", 4, False)], "store": [("merge", 4, True)],
        "merge-two-groups": [("merge", 16, False), ("merge", 4, False)],
        "nothing-delivered": [],
        # a decode-idx plan dispatches what it always did
        "idx-merge": [("merge", 4, False)], "idx-store": [("merge", 4, True)],
    }
    # merge mode and store mode are different instances, and the same decode-idx ones as ever
    assert set(cases["final-merge"]).isdisjoint(cases["final-store"])
    assert cases["merge"] == cases["idx-merge"] and cases["store"] == cases["idx-store"]


def test_header_declares_and_library_exports_the_decode_check_call(native_lib):
    full = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert "#define RS_ORDER_DECODE_CHECK 65536" in text
    assert "#define RS_DECODE_CHECK_FINAL 2u" in text
    assert "#define RS_DECODE_IDX_STORE 1u" in text and "#define RS_ABI_VERSION 1" in text
    assert native_lib.RS_DECODE_CHECK_FINAL == 2 and native_lib.RS_ORDER_DECODE_CHECK == 65536
    name = "rs_plan_create_decode_check"
    assert re.search(r"\bint\s+%s\s*\(" % name, text)
    assert hasattr(native_lib.lib, name) and name in native_lib.SIGNATURES
    # the header states what is and is not idempotent, what a final launch does to a check row and
    # the order of the refusals
    assert "A NON-FINAL MERGE LAUNCH IS NOT IDEMPOTENT" in full
    assert "A FINAL LAUNCH WITHOUT WANTED ROWS IS IDEMPOTENT" in full
    assert "a check row is NOT WRITTEN" in full
    assert "Errors, in rs_plan_create_decode_idx's order" in full


def test_profile_and_argument_errors_need_no_device(native_lib):
    L, N = native_lib.lib, native_lib
    h = ctypes.c_void_p()
    ctx = ctypes.c_void_p(1)  # never dereferenced on these paths
    k, m, n = 4, 2, 6
    szs = (ctypes.c_size_t * 1)(16)
    zero = (ctypes.c_size_t * 1)(0)
    expect = (ctypes.c_uint8 * n)(1, 1, 1, 1, 0, 0)
    few = (ctypes.c_uint8 * n)(1, 1, 1, 0, 0, 0)
    many = (ctypes.c_uint8 * n)(1, 1, 1, 1, 1, 0)
    none = (ctypes.c_void_p * n)()
    inp = (ctypes.c_void_p * n)(4096, None, None, None, None, 4096)  # shard 0, and compared shard 5 itself
    dst = (ctypes.c_void_p * n)(None, None, None, None, 8192, None)
    chk = (ctypes.c_void_p * n)(None, None, None, None, None, 12288)
    in_unexpected = (ctypes.c_void_p * n)(None, None, None, None, 4096, None)  # wanted, not compared
    dst_expected = (ctypes.c_void_p * n)(None, 8192, None, None, None, None)
    chk_expected = (ctypes.c_void_p * n)(None, 12288, None, None, None, None)
    chk_and_dst = (ctypes.c_void_p * n)(None, None, None, None, 12288, None)

    def plan(kk=k, mm=m, c=ctx, sizes=szs, e=expect, i=inp, d=dst, x=chk, bits=0, out=ctypes.byref(h), batch=1):
        return L.rs_plan_create_decode_check(c, 0, kk, mm, batch, sizes, e, i, d, x, bits, out)

    # 1. the profile, before the NULL arrays, the flag bits and everything else
    for kk, mm, want in ((0, 2, N.RS_E_INVALID_PROFILE), (4, 0, N.RS_E_INVALID_PROFILE),
                         (200, 100, N.RS_E_UNSUPPORTED)):
        assert plan(kk, mm) == want
    assert L.rs_plan_create_decode_check(None, 0, 0, 2, 1, None, None, None, None, None, 12,
                                         None) == N.RS_E_INVALID_PROFILE
    # 2. NULL arrays, counts and flag bits, before the expect count
    assert plan(c=None, e=few) == N.RS_E_ARG and plan(batch=0, e=few) == N.RS_E_ARG
    assert plan(sizes=None, e=few) == N.RS_E_ARG and plan(e=None) == N.RS_E_ARG
    assert plan(i=None, e=few) == N.RS_E_ARG and plan(d=None, e=few) == N.RS_E_ARG
    assert plan(x=None, e=few) == N.RS_E_ARG and plan(out=None, e=few) == N.RS_E_ARG
    for bits in (4, 5, 8, 0x80000000):
        assert plan(bits=bits, e=few) == N.RS_E_ARG
    for bits in (0, 1, 2, 3):
        # 3. the expect count, before a misplaced pointer and a zero size
        assert plan(e=few, i=in_unexpected, sizes=zero, bits=bits) == N.RS_E_TOO_FEW_SHARDS
        assert plan(e=many, sizes=zero, bits=bits) == N.RS_E_ARG
        # 4. a misplaced pointer, before a zero size
        assert plan(i=in_unexpected, sizes=zero, bits=bits) == N.RS_E_ARG
        assert plan(d=dst_expected, sizes=zero, bits=bits) == N.RS_E_ARG
        assert plan(x=chk_expected, sizes=zero, bits=bits) == N.RS_E_ARG
        assert plan(x=chk_and_dst, sizes=zero, bits=bits) == N.RS_E_ARG
        # 5. a zero size on a stripe in the launch
        assert plan(sizes=zero, bits=bits) == N.RS_E_NO_DATA
    # a check row alone puts a stripe into a final launch, and only there
    assert plan(sizes=zero, i=none, bits=2) == N.RS_E_NO_DATA
    assert not h.value  # nothing created


# what callfs_amd/build.py records (kernel_resources.json) for the rs_merge_ragged instances: a
# check instance holds the same live state plus one lane flag and one uniform
MERGE_WAVES = {4: 8, 8: 7, 16: 4}


def test_check_kernel_resources():
    from callfs_amd import build as nb
    if nb._stale() or not os.path.exists(nb.RESOURCES):
        nb.build()
    with open(nb.RESOURCES) as fh:
        rep = json.load(fh)
    merge, seen = {}, {}
    for k in rep["kernels"]:
        mo = re.search(r"rs_(merge|check)_ragged<(\d+), .*, (true|false)>\(", k["name"])
        if not mo:
            continue
        key = (int(mo.group(2)), mo.group(3) == "true")
        into = merge if mo.group(1) == "merge" else seen
        assert key not in into, k["name"]
        into[key] = k
    every = sorted((rt, st) for rt in (4, 8, 16) for st in (False, True))
    assert sorted(seen) == every and sorted(merge) == every
    for key, k in seen.items():
        assert "rs_merge_ragged<" not in k["name"]
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert merge[key]["waves_per_simd"] == MERGE_WAVES[key[0]]
        assert k["waves_per_simd"] >= merge[key]["waves_per_simd"], (k["name"], k["vgprs"], k["waves_per_simd"])
        if key[0] > 8:  # two 512-thread blocks per CU need 4 waves per SIMD
            assert k["vgprs"] + k.get("agprs", 0) <= 128, k["name"]
