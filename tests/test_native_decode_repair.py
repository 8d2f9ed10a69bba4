"""The CPU side of the decode-repair plans: the host tables and the rule
(callfs_amd/csrc/decode_repair_tables.hpp) built with g++ under ASan + UBSan and run as a
stand-alone program; what a decode-repair plan dispatches and refuses, on host-only builds of the
plan code and the kernel files linked against the recording HIP stand-ins (also under ASan +
UBSan, also stand-alone: nothing sanitized is loaded into Python); the header and the exports; the
profile and argument errors without a device; and the registers the build recorded for the new
kernels, with the rows of the kernels they are modelled on unchanged."""
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


def test_decode_repair_tables_and_rule_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "decode_repair_host_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + SANITIZE + ["-I", CSRC,
                    os.path.join(NATIVE, "decode_repair_host_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "decode_repair_host_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


def test_routes_dispatch_the_repair_kernel(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sources = [os.path.join(CSRC, f) for f in ("rs_kernels.hip", "rs_mixed.hip", "sha256.hip",
                                               "rs_plan.cpp", "rs_context.cpp")] + [
        os.path.join(NATIVE, f) for f in ("decode_repair_routes.cpp", "fake_hip_runtime.cpp", "fake_hip_memory.cpp")]
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
    exe = str(tmp_path / "decode_repair_routes")
    subprocess.run(["hipcc"] + SANITIZE + objs + ["-o", exe, "-no-pie"] +
                   ["-Wl,--defsym=%s=0" % s for s in fatbin], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CALLFS_RS_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "decode_repair_routes ok", r.stdout[-2000:] + r.stderr[-4000:]
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
        """(kernel, RT, STORE) of a mangled rs_{repair,check,merge}_ragged<RT, Policy, STORE>."""
        mo = re.search(r"\d+rs_(repair|check|merge)_raggedILi(\d+)E.*Lb([01])EEEv", symbol)
        assert mo, symbol
        return mo.group(1), int(mo.group(2)), bool(int(mo.group(3)))

    got = {name: [instance(s) for s in syms] for name, syms in cases.items()}
    assert got == {
        # exactly one rs_repair_ragged dispatch per launch, in the smallest instance that holds the rows
        "repair-merge": [("repair", 4, False)], "repair-store": [("repair", 4, True)],
        "repair-merge-8": [("repair", 8, False)], "repair-store-8": [("repair", 8, True)],
        "repair-merge-16": [("repair", 16, False)], "repair-store-16": [("repair", 16, True)],
        # a stripe with nothing delivered is dispatched: its accumulators are scanned and classified
        "repair-nothing-delivered": [("repair", 4, False)],
        # decode-check and decode-idx plans dispatch what they did before
        "final-merge": [("check", 4, False)], "final-store": [("check", 4, True)],
        "merge": [("merge", 4, False)],
        "idx-merge": [("merge", 4, False)], "idx-store": [("merge", 4, True)],
    }
    assert set(cases["repair-merge"]).isdisjoint(cases["repair-store"])
    assert cases["merge"] == cases["idx-merge"]


def test_header_declares_and_library_exports_the_decode_repair_call(native_lib):
    full = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert "#define RS_ORDER_DECODE_REPAIR 131072" in text
    assert "#define RS_ORDER_DECODE_CHECK 65536" in text and "#define RS_ABI_VERSION 1" in text
    assert native_lib.RS_ORDER_DECODE_REPAIR == 131072
    name = "rs_plan_create_decode_repair"
    assert re.search(r"\bint\s+%s\s*\(" % name, text)
    assert hasattr(native_lib.lib, name) and name in native_lib.SIGNATURES
    # one more pointer array than the decode-check constructor, in front of the flags
    sib = list(native_lib.SIGNATURES["rs_plan_create_decode_check"][1])
    assert list(native_lib.SIGNATURES[name][1]) == sib[:10] + [sib[9]] + sib[10:]
    # the header states the order of the refusals, what is idempotent and the fix contract
    assert "ALWAYS FINAL" in full and "XOR in place" in full
    assert "A LAUNCH WITH WANTED ROWS IN MERGE MODE IS NOT IDEMPOTENT" in full
    assert "A LAUNCH WITH NO WANTED AND NO FIX ROWS IS IDEMPOTENT" in full
    section = full[full.index("decode-repair plans: progressive repair"):full.index("#define RS_ORDER_DECODE_REPAIR")]
    errors = " ".join(section[section.index("Errors, in this order"):].replace("*", " ").split())
    order = [errors.index(s) for s in ("the profile", "a NULL sizes, expect, input, dst, check, fix or out",
                                       "the expect count", "a misplaced pointer", "a fix at an index",
                                       "more than 16 rows (RS_E_UNSUPPORTED)", "sizes[b] == 0", "RS_E_NO_DATA")]
    assert order == sorted(order)


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
    fix = (ctypes.c_void_p * n)(16384, None, None, None, None, 20480)  # an expected and a compared shard
    in_unexpected = (ctypes.c_void_p * n)(None, None, None, None, 4096, None)  # wanted, not compared
    dst_expected = (ctypes.c_void_p * n)(None, 8192, None, None, None, None)
    chk_expected = (ctypes.c_void_p * n)(None, 12288, None, None, None, None)
    chk_and_dst = (ctypes.c_void_p * n)(None, None, None, None, 12288, None)
    fix_wanted = (ctypes.c_void_p * n)(None, None, None, None, 16384, None)

    def plan(kk=k, mm=m, c=ctx, sizes=szs, e=expect, i=inp, d=dst, x=chk, f=fix, bits=0, out=ctypes.byref(h), batch=1):
        return L.rs_plan_create_decode_repair(c, 0, kk, mm, batch, sizes, e, i, d, x, f, bits, out)

    # 1. the profile, before the NULL arrays, the flag bits and everything else
    for kk, mm, want in ((0, 2, N.RS_E_INVALID_PROFILE), (4, 0, N.RS_E_INVALID_PROFILE),
                         (200, 100, N.RS_E_UNSUPPORTED)):
        assert plan(kk, mm) == want
    assert L.rs_plan_create_decode_repair(None, 0, 0, 2, 1, None, None, None, None, None, None, 12,
                                          None) == N.RS_E_INVALID_PROFILE
    # 2. NULL arrays, counts and flag bits, before the expect count
    assert plan(c=None, e=few) == N.RS_E_ARG and plan(batch=0, e=few) == N.RS_E_ARG
    assert plan(sizes=None, e=few) == N.RS_E_ARG and plan(e=None) == N.RS_E_ARG
    assert plan(i=None, e=few) == N.RS_E_ARG and plan(d=None, e=few) == N.RS_E_ARG
    assert plan(x=None, e=few) == N.RS_E_ARG and plan(f=None, e=few) == N.RS_E_ARG
    assert plan(out=None, e=few) == N.RS_E_ARG
    for bits in (2, 3, 4, 8, 0x80000000):  # the plan is always final: FINAL is no flag of this call
        assert plan(bits=bits, e=few) == N.RS_E_ARG
    for bits in (0, 1):
        # 3. the expect count, before a misplaced pointer and a zero size
        assert plan(e=few, i=in_unexpected, sizes=zero, bits=bits) == N.RS_E_TOO_FEW_SHARDS
        assert plan(e=many, sizes=zero, bits=bits) == N.RS_E_ARG
        # 4. a misplaced pointer, the fix placement included, before a zero size
        assert plan(i=in_unexpected, sizes=zero, bits=bits) == N.RS_E_ARG
        assert plan(d=dst_expected, sizes=zero, bits=bits) == N.RS_E_ARG
        assert plan(x=chk_expected, sizes=zero, bits=bits) == N.RS_E_ARG
        assert plan(x=chk_and_dst, sizes=zero, bits=bits) == N.RS_E_ARG
        assert plan(f=fix_wanted, sizes=zero, bits=bits) == N.RS_E_ARG
        assert plan(f=fix_wanted, x=none, sizes=zero, bits=bits) == N.RS_E_ARG  # shard 5 is no longer compared
        # 6. a zero size on a stripe in the launch (5., the row limit, needs more than 16 rows:
        # tests/native/decode_repair_routes.cpp)
        assert plan(sizes=zero, bits=bits) == N.RS_E_NO_DATA
        # a check row alone puts a stripe into the launch
        assert plan(sizes=zero, i=none, bits=bits) == N.RS_E_NO_DATA
    # RS(10,20) with 9 + 8 rows: the row limit, after a misplaced pointer and before a zero size
    k, m, n = 10, 20, 30
    expect = (ctypes.c_uint8 * n)(*([1] * 10 + [0] * 20))
    dst = (ctypes.c_void_p * n)(*([None] * 10 + [8192] * 9 + [None] * 11))
    chk = (ctypes.c_void_p * n)(*([None] * 19 + [12288] * 8 + [None] * 3))
    none = (ctypes.c_void_p * n)()
    fix_wanted = (ctypes.c_void_p * n)(*([None] * 10 + [16384] + [None] * 19))
    inp = (ctypes.c_void_p * n)(*([4096] + [None] * 29))
    create = lambda f, sizes: L.rs_plan_create_decode_repair(ctx, 0, k, m, 1, sizes, expect, inp, dst, chk, f, 0,  # noqa: E731
                                                             ctypes.byref(h))
    assert create(none, szs) == N.RS_E_UNSUPPORTED and create(none, zero) == N.RS_E_UNSUPPORTED
    assert create(fix_wanted, zero) == N.RS_E_ARG
    assert not h.value  # nothing created


# what callfs_amd/build.py records (kernel_resources.json) for the rs_check_ragged instances: a
# repair instance keeps its twin's waves per SIMD, the slow path living in registers the clean
# path has free
CHECK_WAVES = {4: 8, 8: 7, 16: 4}


def _kernels():
    from callfs_amd import build as nb
    if nb._stale() or not os.path.exists(nb.RESOURCES):
        nb.build()
    with open(nb.RESOURCES) as fh:
        return json.load(fh)["kernels"]


def test_repair_kernel_resources():
    check, seen = {}, {}
    for k in _kernels():
        mo = re.search(r"rs_(check|repair)_ragged<(\d+), .*, (true|false)>\(", k["name"])
        if not mo:
            continue
        key = (int(mo.group(2)), mo.group(3) == "true")
        into = check if mo.group(1) == "check" else seen
        assert key not in into, k["name"]
        into[key] = k
    every = sorted((rt, st) for rt in (4, 8, 16) for st in (False, True))
    assert sorted(seen) == every and sorted(check) == every
    for key, k in seen.items():
        # the name stays out of the pattern by which test_native_decode_check.py counts instances
        assert not re.search(r"rs_(merge|check)_ragged<", k["name"])
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0, k
        assert check[key]["waves_per_simd"] == CHECK_WAVES[key[0]]
        assert k["waves_per_simd"] >= check[key]["waves_per_simd"], (k["name"], k["vgprs"], k["waves_per_simd"])
        if key[0] > 8:  # two 512-thread blocks per CU need 4 waves per SIMD
            assert k["vgprs"] + k.get("agprs", 0) <= 128, k["name"]


def test_modelled_kernels_rows_unchanged():
    """rs_apply_locate, rs_apply_correct and rs_check_ragged compile to what they did: the
    recorded registers, spills and occupancy of every instance."""
    want = {
        ("rs_apply_locate", 4): (59, 60, 0, 8), ("rs_apply_locate", 8): (64, 76, 0, 8),
        ("rs_apply_locate", 16): (121, 106, 4, 4),
        ("rs_apply_correct", 4): (59, 68, 0, 8), ("rs_apply_correct", 8): (64, 84, 0, 8),
        ("rs_apply_correct", 16): (121, 106, 17, 4),
        ("rs_check_ragged", 4, False): (62, 40, 0, 8), ("rs_check_ragged", 8, False): (68, 41, 0, 7),
        ("rs_check_ragged", 16, False): (120, 40, 0, 4),
        ("rs_check_ragged", 4, True): (46, 40, 0, 8), ("rs_check_ragged", 8, True): (68, 40, 0, 7),
        ("rs_check_ragged", 16, True): (120, 40, 0, 4),
    }
    got = {}
    for k in _kernels():
        mo = re.search(r"(rs_apply_locate|rs_apply_correct)<(\d+),", k["name"])
        if mo:
            key = (mo.group(1), int(mo.group(2)))
        else:
            mo = re.search(r"(rs_check_ragged)<(\d+), .*, (true|false)>\(", k["name"])
            if not mo:
                continue
            key = (mo.group(1), int(mo.group(2)), mo.group(3) == "true")
        assert key not in got, k["name"]
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0
        got[key] = (k["vgprs"], k["sgprs"], k.get("sgpr_spill", 0), k["waves_per_simd"])
    assert got == want
