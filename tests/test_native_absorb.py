"""The CPU side of absorb objects and encode sessions: the host tables, the
launch planner, a scalar model of the launches and the session's book
(callfs_amd/csrc/absorb_tables.hpp, host_encode_session.hpp) built with g++ under ASan + UBSan and
run as a stand-alone program; what an absorb launch and a session feed dispatch, on host-only
builds of the plan code and the kernel files linked against the recording HIP stand-ins (also
under ASan + UBSan, also stand-alone: nothing sanitized is loaded into Python); the header and the
exports; the profile and argument errors without a device; and the registers the build recorded
for the three rs_absorb instances."""
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
CALLS = ("rs_absorb_create", "rs_absorb_launch", "rs_absorb_destroy", "rs_encode_session_open",
         "rs_encode_session_feed", "rs_encode_session_peek", "rs_encode_session_finish",
         "rs_encode_session_close")
TILE = 4096  # columns of one interval per block (absorb_tables.hpp kAbsorbTileBytes)
WRAPPED = ("hipMalloc", "hipHostMalloc", "hipFree", "hipHostFree", "hipStreamSynchronize",
           "hipEventSynchronize")


def test_absorb_tables_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "absorb_tables_test"
    subprocess.run(["g++", "-std=c++17", "-O1"] + SANITIZE + ["-I", CSRC,
                    os.path.join(NATIVE, "absorb_tables_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "absorb_tables_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


def _blocks(k, S, off, n):
    """The sum over the range's column intervals of ceil(columns / TILE), by brute force: a column's
    run of shards is what the range covers there, and an interval is a maximal run of columns with
    one run of shards."""
    runs = []
    for c in range(S):
        # shards i with off <= i * S + c < off + n
        lo = max(0, -(-(off - c) // S))
        hi = min(k - 1, (off + n - 1 - c) // S)
        runs.append((lo, hi) if lo <= hi else None)
    total, at = 0, 0
    while at < S:
        end = at
        while end < S and runs[end] == runs[at]:
            end += 1
        if runs[at] is not None:
            total += -(-(end - at) // TILE)
        at = end
    return total


def test_launches_dispatch_the_absorb_kernel(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sources = [os.path.join(CSRC, f) for f in ("rs_kernels.hip", "rs_mixed.hip", "sha256.hip", "rs_plan.cpp",
                                               "rs_context.cpp", "rs_encode_session.cpp")] + [
        os.path.join(NATIVE, f) for f in ("absorb_routes.cpp", "fake_hip_runtime.cpp", "fake_hip_memory.cpp")]
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
    exe = str(tmp_path / "absorb_routes")
    subprocess.run(["hipcc"] + SANITIZE + objs + ["-o", exe, "-no-pie"] +
                   ["-Wl,--defsym=%s=0" % s for s in fatbin] +
                   ["-Wl,--wrap=%s" % s for s in WRAPPED], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CALLFS_RS_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "absorb_routes ok", r.stdout[-2000:] + r.stderr[-4000:]
    cases, name = {}, None
    for line in lines[:-1]:
        w = line.split()
        if w[0] == "case":
            name = w[1].rstrip(":")
            cases[name] = dict(f.split("=") for f in w[2:])
            cases[name]["launches"] = []
        else:
            assert w[0] == "dispatch", line
            mo = re.search(r"9rs_absorbILi(\d+)EEEv", w[3])
            assert mo, line
            fields = dict(f.split("=") for f in w[1:3] + w[4:])
            cases[name]["launches"].append((int(mo.group(1)), w[3], fields))
    assert sorted(cases) == sorted(["rows-4", "rows-4-tiny", "rows-2", "rows-3", "rows-8", "rows-12", "rows-16",
                                    "session-inplace", "session-direct", "session-staged"])
    symbols = set()
    for name, c in cases.items():
        k, m, S = int(c["k"]), int(c["m"]), int(c["S"])
        rt = 4 if m <= 4 else 8 if m <= 8 else 16
        assert len(c["launches"]) >= 3, name
        for inst, symbol, f in c["launches"]:
            assert inst == rt, (name, m, inst)  # the smallest instance that holds m
            assert f["grid"] == "%d,1" % _blocks(k, S, int(f["off"]), int(f["len"])), (name, f)
            assert f["block"] == "256" and f["lds"] == "0", (name, f)
            symbols.add(symbol)
        if name.startswith("session"):  # a feed of 2.5 slots first: three launches, in order
            first = [(int(f["off"]), int(f["len"])) for _, _, f in c["launches"][:3]]
            assert first == [(4003, 8000), (12003, 8000), (20003, 4000)], (name, first)
            fed = sorted((int(f["off"]), int(f["len"])) for _, _, f in c["launches"])
            assert all(n <= 8000 for _, n in fed)
            assert fed[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(fed, fed[1:]))
            assert fed[-1][0] + fed[-1][1] == 10 * 8211 - 7  # every body byte in exactly one launch
    assert len(symbols) == 3


def test_header_declares_and_library_exports_the_absorb_calls(native_lib):
    full = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    assert "#define RS_ABI_VERSION 1\n" in text
    assert re.search(r"\btypedef\s+struct\s+rs_absorb\s+rs_absorb\s*;", text)
    assert re.search(r"\btypedef\s+struct\s+rs_encode_session\s+rs_encode_session\s*;", text)
    for name in CALLS:
        assert re.search(r"\b(int|void)\s+%s\s*\(" % name, text), name
        assert hasattr(native_lib.lib, name), name
        assert name in native_lib.SIGNATURES, name
    assert len(native_lib.SIGNATURES["rs_absorb_create"][1]) == 7
    assert len(native_lib.SIGNATURES["rs_absorb_launch"][1]) == 5
    assert len(native_lib.SIGNATURES["rs_encode_session_feed"][1]) == 4
    section = full[full.index("---- absorb objects"):]
    section = section[:section.index("rs_absorb_destroy")]
    # the header states that a launch is not idempotent, what a launch may not do, and the order
    # of the refusals
    assert "A LAUNCH IS NOT IDEMPOTENT" in section
    assert "no\n * allocation, no copy, no sync" in section or "no allocation, no copy, no sync" in section
    assert "graph-capturable" in section
    assert "Each check runs\n * before the next" in section or "Each check runs before the next" in section
    session = full[full.index("---- encode sessions"):]
    session = session[:session.index("rs_encode_session_close(")]
    assert "A FEED IS NOT IDEMPOTENT" in session and "RS_E_SHORT_DATA" in session
    from callfs_amd import device
    assert callable(device.Absorb) and callable(device.Absorb.launch)


def test_profile_and_argument_errors_need_no_device(native_lib):
    L, N = native_lib.lib, native_lib
    h = ctypes.c_void_p()
    ctx = ctypes.c_void_p(1)  # never dereferenced on these paths
    vp = lambda *v: (ctypes.c_void_p * len(v))(*v)  # noqa: E731
    rows4 = vp(4096, 8192, 12288, 16384)

    def create(k=10, m=4, c=ctx, S=16, rows=rows4, out=ctypes.byref(h)):
        return L.rs_absorb_create(c, 0, k, m, S, rows, out)

    # 1. the profile, before the NULL arguments and everything else
    for k, m, want in ((0, 2, N.RS_E_INVALID_PROFILE), (4, 0, N.RS_E_INVALID_PROFILE),
                       (200, 100, N.RS_E_UNSUPPORTED)):
        assert create(k, m, c=None, rows=None, out=None, S=0) == want
    # 2. NULL arguments, before the row count and a zero size
    rows20 = vp(*[4096 * (j + 1) for j in range(20)])
    assert create(c=None, S=0) == N.RS_E_ARG
    assert create(rows=None, S=0) == N.RS_E_ARG and create(out=None, S=0) == N.RS_E_ARG
    assert create(10, 20, c=None, S=0, rows=rows20) == N.RS_E_ARG
    assert create(10, 20, rows=None, S=0) == N.RS_E_ARG
    assert create(rows=vp(4096, None, 12288, 16384), S=0) == N.RS_E_ARG
    # 3. more than 16 rows, before a zero size: RS(10,20), and 17 rows
    assert create(10, 20, S=0, rows=rows20) == N.RS_E_UNSUPPORTED
    assert create(10, 17, S=16, rows=rows20) == N.RS_E_UNSUPPORTED
    # 4. a zero size
    assert create(S=0) == N.RS_E_NO_DATA
    assert create(10, 16, S=0, rows=rows20) == N.RS_E_NO_DATA
    assert not h.value  # nothing created
    # a launch on no object, and destroying none
    assert L.rs_absorb_launch(None, 0, 16, ctypes.c_void_p(4096), None) == N.RS_E_ARG
    L.rs_absorb_destroy(None)
    # sessions: the profile; NULL arguments; an empty body; more than 16 rows
    s = ctypes.c_void_p()
    assert L.rs_encode_session_open(None, 0, 4, 0, None) == N.RS_E_INVALID_PROFILE
    assert L.rs_encode_session_open(None, 200, 100, 0, None) == N.RS_E_UNSUPPORTED
    assert L.rs_encode_session_open(None, 10, 20, 0, ctypes.byref(s)) == N.RS_E_ARG
    assert L.rs_encode_session_open(ctx, 10, 20, 0, None) == N.RS_E_ARG
    assert L.rs_encode_session_open(ctx, 10, 20, 0, ctypes.byref(s)) == N.RS_E_SHORT_DATA
    assert L.rs_encode_session_open(ctx, 10, 20, 1, ctypes.byref(s)) == N.RS_E_UNSUPPORTED
    assert not s.value
    assert L.rs_encode_session_feed(None, 0, ctypes.c_void_p(4096), 1) == N.RS_E_ARG
    assert L.rs_encode_session_peek(None, 0, ctypes.c_void_p(4096), 1) == N.RS_E_ARG
    assert L.rs_encode_session_finish(None, None, None) == N.RS_E_ARG
    L.rs_encode_session_close(None)


def test_absorb_kernel_resources():
    from callfs_amd import build as nb
    if nb._stale() or not os.path.exists(nb.RESOURCES):
        nb.build()
    with open(nb.RESOURCES) as fh:
        rep = json.load(fh)
    seen = {}
    for k in rep["kernels"]:
        if "rs_absorb<" not in k["name"]:
            continue
        mo = re.search(r"rs_absorb<(\d+)>\(", k["name"])
        assert mo, k["name"]
        rt = int(mo.group(1))
        assert rt not in seen, k["name"]
        seen[rt] = k
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert k["vgprs"] + k.get("agprs", 0) <= 128, k["name"]
        assert k["vgprs"] >= 4 * rt  # the accumulators stay in registers
    assert sorted(seen) == [4, 8, 16]
