"""The CPU side of feed objects: the host tables
(callfs_amd/csrc/feed_tables.hpp) built with g++ under ASan + UBSan and run as a stand-alone
program; what a feed launch dispatches, on host-only builds of the plan code and the kernel files
linked against the recording HIP stand-ins (also under ASan + UBSan, also stand-alone: nothing
sanitized is loaded into Python); the header and the exports; the profile and argument errors
without a device; and the registers the build recorded for the six rs_feed instances."""
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
CALLS = ("rs_feed_create", "rs_feed_launch", "rs_feed_destroy", "rs_session_open", "rs_session_feed",
         "rs_session_peek", "rs_session_finish", "rs_session_close")
TILE = 4096  # bytes of the source per block (rs_kernels.hpp kFeedTileBytes)
WRAPPED = ("hipMalloc", "hipHostMalloc", "hipFree", "hipHostFree", "hipStreamSynchronize",
           "hipEventSynchronize")


def test_feed_tables_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "feed_tables_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + SANITIZE + ["-I", CSRC,
                    os.path.join(NATIVE, "feed_tables_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "feed_tables_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


def test_launches_dispatch_the_feed_kernel(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sources = [os.path.join(CSRC, f) for f in ("rs_kernels.hip", "rs_mixed.hip", "sha256.hip",
                                               "rs_plan.cpp", "rs_context.cpp", "rs_session.cpp")] + [
        os.path.join(NATIVE, f) for f in ("feed_routes.cpp", "fake_hip_runtime.cpp", "fake_hip_memory.cpp")]
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
    exe = str(tmp_path / "feed_routes")
    subprocess.run(["hipcc"] + SANITIZE + objs + ["-o", exe, "-no-pie"] +
                   ["-Wl,--defsym=%s=0" % s for s in fatbin] +
                   ["-Wl,--wrap=%s" % s for s in WRAPPED], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CALLFS_RS_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "feed_routes ok", r.stdout[-2000:] + r.stderr[-4000:]
    cases, name = {}, None
    for line in lines[:-1]:
        w = line.split()
        if w[0] == "case":
            name = w[1].rstrip(":")
            cases[name] = {"S": int(w[2].split("=")[1]), "rows": int(w[3].split("=")[1]), "launches": []}
        else:
            assert w[0] == "dispatch", line
            mo = re.search(r"7rs_feedILi(\d+)ELb([01])EEEv", w[2])
            assert mo, line
            fields = dict(f.split("=") for f in w[3:])
            cases[name]["launches"].append((w[1], int(mo.group(1)), bool(int(mo.group(2))), w[2], fields))
    assert sorted(cases) == sorted(["rows-4", "rows-4-wanted", "rows-2-mixed", "rows-1-tiny", "rows-5", "rows-8",
                                    "rows-9", "rows-12", "rows-16", "rows-0", "session-inplace",
                                    "session-staged"])
    assert cases.pop("rows-0")["launches"] == []
    symbols = {False: set(), True: set()}
    for name, c in cases.items():
        S, rows = c["S"], c["rows"]
        rt = 4 if rows <= 4 else 8 if rows <= 8 else 16
        assert len(c["launches"]) >= 3, name
        for at, (mode, inst, store, symbol, f) in enumerate(c["launches"]):
            # the first launch of a case stores, every later one merges
            assert (mode == "store") == (at == 0) == store, (name, at, mode, store)
            assert inst == rt, (name, rows, inst)  # the smallest instance that holds the rows
            assert f["grid"] == "%d,1" % -(-S // TILE), (name, S, f)
            assert f["block"] == "256" and f["lds"] == "0", (name, f)
            assert int(f["nvec"]) == S // 16, (name, f)
            symbols[store].add(symbol)
    assert len(symbols[False]) == 3 and len(symbols[True]) == 3
    assert symbols[False].isdisjoint(symbols[True])


def test_header_declares_and_library_exports_the_feed_calls(native_lib):
    full = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert "#define RS_ABI_VERSION 1\n" in text
    assert re.search(r"\btypedef\s+struct\s+rs_feed\s+rs_feed\s*;", text)
    for name in CALLS:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, text), name
        assert hasattr(native_lib.lib, name), name
        assert name in native_lib.SIGNATURES, name
    assert len(native_lib.SIGNATURES["rs_feed_create"][1]) == 9
    assert len(native_lib.SIGNATURES["rs_feed_launch"][1]) == 5
    section = full[full.index("---- feed objects"):]
    section = section[:section.index("rs_feed_destroy")]
    # the header states that a merge launch is not idempotent, in the words of the other
    # progressive calls, what a launch may not do, and the order of the refusals
    assert "A MERGE LAUNCH IS NOT IDEMPOTENT" in section
    assert "no allocation, no copy, no sync" in section and "graph-capturable" in section
    assert "Each check runs\n * before the next" in section or "Each check runs before the next" in section
    from callfs_amd import device
    assert callable(device.Feed) and callable(device.Feed.launch)


def test_profile_and_argument_errors_need_no_device(native_lib):
    L, N = native_lib.lib, native_lib
    h = ctypes.c_void_p()
    ctx = ctypes.c_void_p(1)  # never dereferenced on these paths
    k, m, n = 4, 2, 6
    u8 = lambda *v: (ctypes.c_uint8 * len(v))(*v)  # noqa: E731
    vp = lambda *v: (ctypes.c_void_p * len(v))(*v)  # noqa: E731
    expect, few, many = u8(1, 1, 1, 1, 0, 0), u8(1, 1, 1, 0, 0, 0), u8(1, 1, 1, 1, 1, 0)
    dst = vp(None, None, None, None, 8192, None)
    chk = vp(None, None, None, None, None, 4096)
    dst_expected = vp(None, 8192, None, None, None, None)
    chk_expected = vp(4096, None, None, None, None, None)
    chk_on_dst = vp(None, None, None, None, 4096, None)

    def create(kk=k, mm=m, c=ctx, S=16, e=expect, d=dst, ch=chk, out=ctypes.byref(h)):
        return L.rs_feed_create(c, 0, kk, mm, S, e, d, ch, out)

    # 1. the profile, before the NULL arrays and everything else
    for kk, mm, want in ((0, 2, N.RS_E_INVALID_PROFILE), (4, 0, N.RS_E_INVALID_PROFILE),
                         (200, 100, N.RS_E_UNSUPPORTED)):
        assert create(kk, mm) == want
    assert L.rs_feed_create(None, 0, 0, 2, 0, None, None, None, None) == N.RS_E_INVALID_PROFILE
    # 2. NULL arrays, before the expect count
    assert create(c=None, e=few) == N.RS_E_ARG
    assert create(e=None) == N.RS_E_ARG
    assert create(d=None, e=few) == N.RS_E_ARG and create(ch=None, e=few) == N.RS_E_ARG
    assert create(out=None, e=few) == N.RS_E_ARG
    # 3. the expect count, before a misplaced pointer, the row count and a zero size
    assert create(e=few, d=dst_expected, S=0) == N.RS_E_TOO_FEW_SHARDS
    assert create(e=many, S=0) == N.RS_E_ARG
    # 4. a misplaced pointer, before the row count and a zero size
    assert create(d=dst_expected, S=0) == N.RS_E_ARG
    assert create(ch=chk_expected, S=0) == N.RS_E_ARG
    assert create(ch=chk_on_dst, S=0) == N.RS_E_ARG
    # 5. more than 16 rows, before a zero size (RS(10,20): 9 wanted and 8 compared)
    e30 = u8(*([1] * 10 + [0] * 20))
    d30 = vp(*([None] * 10 + [8192 + 64 * i for i in range(9)] + [None] * 11))
    c30 = vp(*([None] * 19 + [4096 + 64 * i for i in range(8)] + [None] * 3))
    assert L.rs_feed_create(ctx, 0, 10, 20, 0, e30, d30, c30, ctypes.byref(h)) == N.RS_E_UNSUPPORTED
    d30_bad = vp(*([8192] + [None] * 9 + [8192 + 64 * i for i in range(9)] + [None] * 11))
    assert L.rs_feed_create(ctx, 0, 10, 20, 0, e30, d30_bad, c30, ctypes.byref(h)) == N.RS_E_ARG
    # 6. a zero size
    assert create(S=0) == N.RS_E_NO_DATA
    assert not h.value  # nothing created
    # a launch on no object, and destroying none
    assert L.rs_feed_launch(None, 0, ctypes.c_void_p(4096), 0, None) == N.RS_E_ARG
    L.rs_feed_destroy(None)


def test_feed_kernel_resources():
    from callfs_amd import build as nb
    if nb._stale() or not os.path.exists(nb.RESOURCES):
        nb.build()
    with open(nb.RESOURCES) as fh:
        rep = json.load(fh)
    seen = {}
    for k in rep["kernels"]:
        if "rs_feed<" not in k["name"]:
            continue
        mo = re.search(r"rs_feed<(\d+), (true|false)>\(", k["name"])
        assert mo, k["name"]
        key = (int(mo.group(1)), mo.group(2) == "true")
        assert key not in seen, k["name"]
        seen[key] = k
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 128, k["name"]
    assert sorted(seen) == sorted((rt, st) for rt in (4, 8, 16) for st in (False, True))
    # a store instance holds no row vector it loaded
    for rt in (4, 8, 16):
        assert seen[(rt, True)]["vgprs"] <= seen[(rt, False)]["vgprs"]
