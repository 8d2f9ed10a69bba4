"""The CPU side of the decode-idx calls: the host tables
(callfs_amd/csrc/decode_idx_tables.hpp) built with g++ under ASan + UBSan and run as a
stand-alone program; what a decode-idx plan dispatches, on host-only builds of the plan code and
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
CALLS = ("rs_plan_create_decode_idx", "rs_decode_idx", "rs_decode_idx_batch")


def test_decode_idx_tables_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "decode_idx_host_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + SANITIZE + ["-I", CSRC,
                    os.path.join(NATIVE, "decode_idx_host_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "decode_idx_host_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


def test_routes_dispatch_the_merge_kernel(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sources = [os.path.join(CSRC, f) for f in ("rs_kernels.hip", "rs_mixed.hip", "sha256.hip",
                                               "rs_plan.cpp", "rs_context.cpp")] + [
        os.path.join(NATIVE, f) for f in ("decode_idx_routes.cpp", "fake_hip_runtime.cpp", "fake_hip_memory.cpp")]
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
    exe = str(tmp_path / "decode_idx_routes")
    subprocess.run(["hipcc"] + SANITIZE + objs + ["-o", exe, "-no-pie"] +
                   ["-Wl,--defsym=%s=0" % s for s in fatbin], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CALLFS_RS_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "decode_idx_routes ok", r.stdout[-2000:] + r.stderr[-4000:]
    cases, name = {}, None
    for line in lines[:-1]:
        w = line.split()
        if w[0] == "case":
            name = w[1].rstrip(":")
            cases[name] = []
        else:
            assert w[0] == "dispatch", line
            cases[name].append(w[1])
    assert sorted(cases) == sorted(["merge", "store", "merge-8", "store-8", "merge-two-groups",
                                    "store-two-groups", "nothing-delivered"])

    def instance(symbol):
        """(RT, STORE) of a mangled rs_merge_ragged<RT, Policy, STORE> instance."""
        mo = re.search(r"15rs_merge_raggedILi(\d+)E.*Lb([01])EEEv", symbol)
        assert mo, symbol
        return int(mo.group(1)), bool(int(mo.group(2)))

    got = {name: [instance(s) for s in syms] for name, syms in cases.items()}
    # once per group of 16 wanted rows, in the smallest instance that holds the group's rows
    assert got["merge"] == [(4, False)] and got["store"] == [(4, True)]
    assert got["merge-8"] == [(8, False)] and got["store-8"] == [(8, True)]
    assert got["merge-two-groups"] == [(16, False), (4, False)]
    assert got["store-two-groups"] == [(16, True), (4, True)]
    # merge mode and store mode are different instances
    assert set(cases["merge"]).isdisjoint(cases["store"])
    assert got["nothing-delivered"] == []


def test_header_declares_and_library_exports_the_decode_idx_calls(native_lib):
    full = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert "#define RS_ORDER_DECODE_IDX 32768" in text
    assert "#define RS_DECODE_IDX_STORE 1u" in text
    assert native_lib.RS_DECODE_IDX_STORE == 1
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(native_lib.lib, name), name
        assert name in native_lib.SIGNATURES, name
    # the header states that a merge launch is not idempotent, that a store call skips the upload
    # and the order of the refusals
    assert "A MERGE LAUNCH IS NOT IDEMPOTENT" in full
    assert "A STORE CALL DOES NOT UPLOAD THE WANTED SHARDS" in full
    assert "Each check runs over the whole batch before the next" in full


def test_profile_and_argument_errors_need_no_device(native_lib):
    L, N = native_lib.lib, native_lib
    h = ctypes.c_void_p()
    ctx = ctypes.c_void_p(1)  # never dereferenced on these paths
    k, m, n = 4, 2, 6
    szs = (ctypes.c_size_t * 1)(16)
    zero = (ctypes.c_size_t * 1)(0)
    none = (ctypes.c_void_p * n)()
    st = (ctypes.c_int * 1)(77)
    expect = (ctypes.c_uint8 * n)(1, 1, 1, 1, 0, 0)
    few = (ctypes.c_uint8 * n)(1, 1, 1, 0, 0, 0)
    many = (ctypes.c_uint8 * n)(1, 1, 1, 1, 1, 0)
    inp = (ctypes.c_void_p * n)(4096, None, None, None, None, None)
    dst = (ctypes.c_void_p * n)(None, None, None, None, 8192, None)
    in_unexpected = (ctypes.c_void_p * n)(None, None, None, None, None, 4096)
    dst_expected = (ctypes.c_void_p * n)(None, 8192, None, None, None, None)

    def plan(kk=k, mm=m, c=ctx, sizes=szs, e=expect, i=inp, d=dst, bits=0, out=ctypes.byref(h), batch=1):
        return L.rs_plan_create_decode_idx(c, 0, kk, mm, batch, sizes, e, i, d, bits, out)

    def batch(kk=k, mm=m, c=ctx, sizes=szs, e=expect, i=inp, d=dst, bits=0, status=st, count=1):
        return L.rs_decode_idx_batch(c, kk, mm, count, sizes, d, e, i, bits, status)

    def one(kk=k, mm=m, c=ctx, S=16, e=expect, i=inp, d=dst, bits=0):
        return L.rs_decode_idx(c, kk, mm, S, d, e, i, bits)

    # 1. the profile, before the NULL arrays, the flag bits and everything else
    for kk, mm, want in ((0, 2, N.RS_E_INVALID_PROFILE), (4, 0, N.RS_E_INVALID_PROFILE),
                         (200, 100, N.RS_E_UNSUPPORTED)):
        assert plan(kk, mm) == want and batch(kk, mm) == want and one(kk, mm) == want
    assert L.rs_plan_create_decode_idx(None, 0, 0, 2, 1, None, None, None, None, 6, None) == N.RS_E_INVALID_PROFILE
    assert L.rs_decode_idx_batch(None, 0, 2, 1, None, None, None, None, 6, None) == N.RS_E_INVALID_PROFILE
    assert L.rs_decode_idx(None, 0, 2, 16, None, None, None, 6) == N.RS_E_INVALID_PROFILE
    # 2. NULL arrays, counts and flag bits, before the expect count
    assert plan(c=None, e=few) == N.RS_E_ARG
    assert plan(batch=0, e=few) == N.RS_E_ARG
    assert plan(sizes=None, e=few) == N.RS_E_ARG and plan(e=None) == N.RS_E_ARG
    assert plan(i=None, e=few) == N.RS_E_ARG and plan(d=None, e=few) == N.RS_E_ARG
    assert plan(out=None, e=few) == N.RS_E_ARG
    for bits in (2, 3, 0x80000000):
        assert plan(bits=bits, e=few) == N.RS_E_ARG
        assert batch(bits=bits, e=few) == N.RS_E_ARG and st[0] == 77
        assert one(bits=bits, e=few) == N.RS_E_ARG
    assert batch(c=None) == N.RS_E_ARG and batch(count=-1) == N.RS_E_ARG
    assert batch(sizes=None) == N.RS_E_ARG and batch(e=None) == N.RS_E_ARG
    assert batch(i=None) == N.RS_E_ARG and batch(d=None) == N.RS_E_ARG and batch(status=None) == N.RS_E_ARG
    assert one(c=None) == N.RS_E_ARG and one(e=None) == N.RS_E_ARG
    assert one(i=None) == N.RS_E_ARG and one(d=None) == N.RS_E_ARG
    # 3. the expect count, before a misplaced pointer and a zero size
    for f in (plan, batch):
        assert f(e=few, i=in_unexpected, sizes=zero) == N.RS_E_TOO_FEW_SHARDS
        assert f(e=many, sizes=zero) == N.RS_E_ARG
    assert st[0] == N.RS_E_ARG
    assert one(e=few, i=in_unexpected, S=0) == N.RS_E_TOO_FEW_SHARDS
    # 4. a misplaced pointer, before a zero size
    for f in (plan, batch):
        assert f(i=in_unexpected, sizes=zero) == N.RS_E_ARG
        assert f(d=dst_expected, sizes=zero) == N.RS_E_ARG
    assert one(d=dst_expected, S=0) == N.RS_E_ARG
    # 5. a zero size on a stripe with both an input and a dst
    assert plan(sizes=zero) == N.RS_E_NO_DATA
    assert batch(sizes=zero) == N.RS_E_NO_DATA and st[0] == N.RS_E_NO_DATA
    assert one(S=0) == N.RS_E_NO_DATA
    assert not h.value  # nothing created
    # nothing to do: no input, or no wanted shard -- RS_OK without a device, whatever the size
    st[0] = 77
    assert batch(i=none) == N.RS_OK and st[0] == N.RS_OK
    assert batch(d=none, sizes=zero) == N.RS_OK
    assert one(i=none) == N.RS_OK and one(d=none, S=0) == N.RS_OK
    assert batch(count=0, sizes=None, e=None, i=None, d=None, status=None) == N.RS_OK


# what callfs_amd/build.py records for the single-source rs_update_ragged instance of the same
# RT (kernel_resources.json): a merge instance holds the same live state plus one uniform, a
# store instance less
UPDATE_WAVES = {4: 8, 8: 7, 16: 4}


def test_merge_kernel_resources():
    from callfs_amd import build as nb
    if nb._stale() or not os.path.exists(nb.RESOURCES):
        nb.build()
    with open(nb.RESOURCES) as fh:
        rep = json.load(fh)
    recorded = {}
    for k in rep["kernels"]:
        mo = re.search(r"rs_update_ragged<(\d+), .*, false>\(", k["name"])
        if mo:
            recorded[int(mo.group(1))] = k["waves_per_simd"]
    assert recorded == UPDATE_WAVES
    ks = [k for k in rep["kernels"] if "rs_merge_ragged<" in k["name"]]
    seen = {}
    for k in ks:
        mo = re.search(r"rs_merge_ragged<(\d+), .*, (true|false)>\(", k["name"])
        assert mo, k["name"]
        key = (int(mo.group(1)), mo.group(2) == "true")
        assert key not in seen, k["name"]
        seen[key] = k
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["waves_per_simd"] >= UPDATE_WAVES[key[0]], (k["name"], k["vgprs"], k["waves_per_simd"])
        if key[0] > 8:  # two 512-thread blocks per CU need 4 waves per SIMD
            assert k["vgprs"] + k.get("agprs", 0) <= 128, k["name"]
    assert sorted(seen) == sorted((rt, st) for rt in (4, 8, 16) for st in (False, True))
    # the early destination loads of RT 4 are the merge instance's alone: the store instance
    # does not carry their registers
    assert seen[(4, True)]["vgprs"] < seen[(4, False)]["vgprs"]
    for rt in (8, 16):
        assert seen[(rt, True)]["vgprs"] <= seen[(rt, False)]["vgprs"]
