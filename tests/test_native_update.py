"""The CPU side of the update calls: the host tables and the overwrite planner
(callfs_amd/csrc/update_tables.hpp, overwrite_plan.hpp) built with g++ under ASan + UBSan and
run as a stand-alone program; what an update plan dispatches, on host-only builds of the plan
code and the kernel files linked against the recording HIP stand-ins (also under ASan + UBSan,
also stand-alone: nothing sanitized is loaded into Python); the header and the exports; the
profile errors without a device; and the registers the build recorded for the new kernels."""
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
CALLS = ("rs_plan_create_update", "rs_update", "rs_encode_idx", "rs_update_batch",
         "rs_codec_overwrite")


def test_update_tables_and_overwrite_planner_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "update_host_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + SANITIZE + ["-I", CSRC,
                    os.path.join(NATIVE, "update_host_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "update_host_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


def test_routes_dispatch_the_update_kernel(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sources = [os.path.join(CSRC, f) for f in ("rs_kernels.hip", "rs_mixed.hip", "sha256.hip",
                                               "rs_plan.cpp", "rs_context.cpp")] + [
        os.path.join(NATIVE, f) for f in ("update_routes.cpp", "fake_hip_runtime.cpp", "fake_hip_memory.cpp")]
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
    exe = str(tmp_path / "update_routes")
    subprocess.run(["hipcc"] + SANITIZE + objs + ["-o", exe, "-no-pie"] +
                   ["-Wl,--defsym=%s=0" % s for s in fatbin], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CALLFS_RS_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "update_routes ok", r.stdout[-2000:] + r.stderr[-4000:]
    cases, name = {}, None
    for line in lines[:-1]:
        w = line.split()
        if w[0] == "case":
            name = w[1].rstrip(":")
            cases[name] = []
        else:
            assert w[0] == "dispatch", line
            cases[name].append(w[1])
    assert sorted(cases) == sorted(["pair", "single", "pair-8", "pair-two-groups", "single-two-groups",
                                    "unchanged"])

    def instance(symbol):
        """(RT, PAIR) of a mangled rs_update_ragged<RT, Policy, PAIR> instance."""
        mo = re.search(r"16rs_update_raggedILi(\d+)E.*Lb([01])EEEv", symbol)
        assert mo, symbol
        return int(mo.group(1)), bool(int(mo.group(2)))

    got = {name: [instance(s) for s in syms] for name, syms in cases.items()}
    # once per group of 16 parity rows, in the smallest instance that holds the group's rows
    assert got["pair"] == [(4, True)] and got["single"] == [(4, False)]
    assert got["pair-8"] == [(8, True)]
    assert got["pair-two-groups"] == [(16, True), (4, True)]
    assert got["single-two-groups"] == [(16, False), (4, False)]
    # pair mode and EncodeIdx mode are different instances
    assert set(cases["pair"]).isdisjoint(cases["single"])
    assert got["unchanged"] == []


def test_header_declares_and_library_exports_the_update_calls(native_lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "#define RS_ORDER_UPDATE 4096" in text
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(native_lib.lib, name), name
        assert name in native_lib.SIGNATURES, name
    # the header states that a launch is not idempotent
    assert "NOT IDEMPOTENT" in open(HEADER).read()


def test_profile_and_argument_errors_need_no_device(native_lib):
    L, N = native_lib.lib, native_lib
    h = ctypes.c_void_p()
    ctx = ctypes.c_void_p(1)  # never dereferenced on these paths
    szs = (ctypes.c_size_t * 1)(16)
    ptrs = (ctypes.c_void_p * 8)()
    flags = (ctypes.c_uint8 * 4)(1, 0, 0, 0)
    st = (ctypes.c_int * 1)()
    for k, m, want in ((0, 2, N.RS_E_INVALID_PROFILE), (4, 0, N.RS_E_INVALID_PROFILE),
                       (200, 100, N.RS_E_UNSUPPORTED)):
        assert L.rs_plan_create_update(ctx, 0, k, m, 1, szs, flags, ptrs, ptrs, ptrs, ctypes.byref(h)) == want
        assert L.rs_update(ctx, k, m, 16, ptrs, ptrs, ptrs) == want
        assert L.rs_encode_idx(ctx, k, m, 16, ptrs, 0, ptrs) == want
        assert L.rs_update_batch(ctx, k, m, 1, szs, ptrs, ptrs, ptrs, st) == want
        assert L.rs_codec_overwrite(ctx, k, m, 16, ptrs, 0, ptrs, 1) == want
    # the profile comes before the NULL arrays
    assert L.rs_plan_create_update(None, 0, 0, 2, 1, None, None, None, None, None, None) == N.RS_E_INVALID_PROFILE
    assert L.rs_update(None, 0, 2, 16, None, None, None) == N.RS_E_INVALID_PROFILE
    # NULL arrays and bad counts
    assert L.rs_plan_create_update(None, 0, 4, 2, 1, szs, flags, ptrs, ptrs, ptrs, ctypes.byref(h)) == N.RS_E_ARG
    assert L.rs_plan_create_update(ctx, 0, 4, 2, 0, szs, flags, ptrs, ptrs, ptrs, ctypes.byref(h)) == N.RS_E_ARG
    assert L.rs_plan_create_update(ctx, 0, 4, 2, 1, None, flags, ptrs, ptrs, ptrs, ctypes.byref(h)) == N.RS_E_ARG
    assert L.rs_plan_create_update(ctx, 0, 4, 2, 1, szs, flags, ptrs, ptrs, ptrs, None) == N.RS_E_ARG
    # a zero size on a changed stripe, then a changed shard without pointers
    zero = (ctypes.c_size_t * 1)(0)
    assert L.rs_plan_create_update(ctx, 0, 4, 2, 1, zero, flags, ptrs, ptrs, ptrs, ctypes.byref(h)) == N.RS_E_NO_DATA
    assert L.rs_plan_create_update(ctx, 0, 4, 2, 1, szs, flags, ptrs, ptrs, ptrs, ctypes.byref(h)) == N.RS_E_ARG
    assert not h.value
    assert L.rs_update(ctx, 4, 2, 16, None, ptrs, ptrs) == N.RS_E_ARG
    assert L.rs_update(None, 4, 2, 16, ptrs, ptrs, ptrs) == N.RS_E_ARG
    one = (ctypes.c_void_p * 4)(0, 4096, 0, 0)
    assert L.rs_update(ctx, 4, 2, 16, ptrs, one, ptrs) == N.RS_E_ARG  # new without old: ErrInvalidInput
    assert L.rs_encode_idx(ctx, 4, 2, 16, ctypes.c_void_p(4096), 4, ptrs) == N.RS_E_ARG  # ErrInvalidShardIdx
    assert L.rs_encode_idx(ctx, 4, 2, 16, ctypes.c_void_p(4096), -1, ptrs) == N.RS_E_ARG
    assert L.rs_encode_idx(ctx, 4, 2, 16, None, 0, ptrs) == N.RS_E_ARG
    assert L.rs_update_batch(ctx, 4, 2, -1, szs, ptrs, ptrs, ptrs, st) == N.RS_E_ARG
    assert L.rs_update_batch(ctx, 4, 2, 1, szs, ptrs, ptrs, ptrs, None) == N.RS_E_ARG
    # nothing changed: RS_OK without a device
    assert L.rs_update_batch(ctx, 4, 2, 1, szs, ptrs, ptrs, ptrs, st) == N.RS_OK and st[0] == N.RS_OK
    assert L.rs_update(ctx, 4, 2, 16, ptrs, ptrs, ptrs) == N.RS_OK
    # rs_codec_overwrite: the range
    assert L.rs_codec_overwrite(ctx, 4, 2, 16, ptrs, 0, ptrs, 0) == N.RS_E_ARG   # (data NULL too)
    data = ctypes.c_void_p(4096)
    assert L.rs_codec_overwrite(ctx, 4, 2, 16, ptrs, 0, data, 0) == N.RS_E_ARG
    assert L.rs_codec_overwrite(ctx, 4, 2, 16, ptrs, -1, data, 1) == N.RS_E_ARG
    assert L.rs_codec_overwrite(ctx, 4, 2, 16, ptrs, 64, data, 1) == N.RS_E_ARG
    assert L.rs_codec_overwrite(ctx, 4, 2, 16, ptrs, 60, data, 5) == N.RS_E_ARG
    assert L.rs_codec_overwrite(ctx, 4, 2, 16, ptrs, 0, data, 1) == N.RS_E_ARG   # NULL touched shard
    assert L.rs_codec_overwrite(ctx, 4, 2, 16, None, 0, data, 1) == N.RS_E_ARG


# what callfs_amd/build.py recorded for the instances when they were first compiled
# (DESIGN.md §5.11): waves per SIMD by (RT, PAIR)
RECORDED_WAVES = {(4, False): 8, (8, False): 7, (16, False): 4,
                  (4, True): 6, (8, True): 5, (16, True): 4}


def test_update_kernel_resources():
    from callfs_amd import build as nb
    if nb._stale() or not os.path.exists(nb.RESOURCES):
        nb.build()
    with open(nb.RESOURCES) as fh:
        rep = json.load(fh)
    ks = [k for k in rep["kernels"] if "rs_update_ragged<" in k["name"]]
    seen = {}
    for k in ks:
        assert "rs_apply_lds<" not in k["name"]
        mo = re.search(r"rs_update_ragged<(\d+), .*, (true|false)>\(", k["name"])
        assert mo, k["name"]
        key = (int(mo.group(1)), mo.group(2) == "true")
        assert key not in seen, k["name"]
        seen[key] = k
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["waves_per_simd"] >= RECORDED_WAVES[key], (k["name"], k["vgprs"], k["waves_per_simd"])
        if key[0] > 8:  # two 512-thread blocks per CU need 4 waves per SIMD
            assert k["vgprs"] + k.get("agprs", 0) <= 128, k["name"]
    assert sorted(seen) == sorted(RECORDED_WAVES)
