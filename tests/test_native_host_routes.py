"""The chunk pipeline of the host-memory batch routes on the CPU: rs_host.cpp and
the rest of the library compiled for the host only, linked against the HIP stand-ins and run as
a stand-alone program under ASan + UBSan (tests/native/host_routes.cpp; nothing sanitized is
loaded into Python). A 64 KiB chunk budget sends every call through more chunks than a lane has
slots; the program checks return codes, statuses, guard bytes, read-only bytes and the update
calls' parity, and this test what each call cost and dispatched."""
import concurrent.futures
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "callfs_amd", "csrc")
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-fno-omit-frame-pointer"]
SLOTS = 3  # a lane's default pipeline depth (host_common.hpp pipeline_slots)

# Recorded by running this same program on the code as it was before the three chunk loops became
# one (run_ragged_chunks, run_update_chunks, run_locate_chunks; commit 3ea7e2e), RS(4,2) over the
# sizes of host_routes.cpp: (calls, chunks, launches, copies, uploads, async H2D, async D2H,
# dispatches, grid blocks summed, kernel, RT, PAIR). A repeated call (".again") finds its tables
# on the lane: one upload and one counted copy fewer, everything else the same.
FIRST = {
    "encode": (1, 26, 26, 53, 1, 26, 26, 26, 29, "rs_apply_ragged", 4, None),
    "reconstruct": (1, 26, 26, 53, 1, 26, 26, 26, 29, "rs_apply_ragged", 4, None),
    "reconstruct-some": (1, 26, 26, 53, 1, 26, 26, 26, 29, "rs_apply_ragged", 4, None),
    "update-pair": (1, 25, 25, 51, 1, 25, 25, 25, 29, "rs_update_ragged", 4, True),
    "encode-idx": (1, 6, 6, 13, 1, 6, 6, 6, 13, "rs_update_ragged", 4, False),
    "locate": (1, 26, 26, 53, 1, 26, 26, 26, 29, "rs_apply_locate", 4, None),
    "locate2": (1, 26, 26, 53, 1, 26, 26, 26, 29, "rs_apply_locate2", 4, None),
    "correct": (1, 26, 26, 53, 1, 26, 26, 26, 29, "rs_apply_correct", 4, None),
}
# The in-place transport (CALLFS_RS_INPLACE_PIPELINE=1): no copy but the table upload.
FIRST_INPLACE = {
    "encode": (1, 26, 26, 1, 1, 0, 0, 26, 59, "rs_apply_small_ragged", 2, None),
    "reconstruct": (1, 26, 26, 1, 1, 0, 0, 26, 59, "rs_apply_small_ragged", 2, None),
}
FIELDS = ("calls", "chunks", "launches", "copies", "uploads", "h2d", "d2h", "dispatches", "blocks")


def expected(first):
    out = {}
    for name, row in first.items():
        out[name] = row
        out[name + ".again"] = row[:3] + (row[3] - 1, row[4] - 1) + row[5:]
    return out


def instance(symbol):
    """(kernel, RT, PAIR or None) of a mangled kernel instance."""
    mo = re.match(r"_ZN6callfs3dev\d+(rs_[a-z0-9_]+?)ILi(\d+)E", symbol)
    assert mo, symbol
    pair = None
    if mo.group(1) == "rs_update_ragged":
        pm = re.search(r"EELb([01])EEEvNS_9ApplyArgsE", symbol)
        assert pm, symbol
        pair = bool(int(pm.group(1)))
    return mo.group(1), int(mo.group(2)), pair


def parse(stdout):
    lines = stdout.splitlines()
    assert lines and lines[-1] == "host_routes ok", stdout[-2000:]
    cases, name = {}, None
    for line in lines[:-1]:
        w = line.split()
        if w[0] == "case":
            name = w[1].rstrip(":")
            got = dict(f.split("=") for f in w[2:])
            cases[name] = [tuple(int(got[f]) for f in FIELDS), []]
        else:
            assert w[0] == "dispatch", line
            cases[name][1].append((instance(w[1]), int(w[2].lstrip("x"))))
    return cases


def check(cases, want):
    assert sorted(cases) == sorted(want)
    for name, row in want.items():
        counts, dispatched = cases[name]
        assert counts == row[:9], (name, dict(zip(FIELDS, counts)))
        assert counts[1] > SLOTS, name  # the slots are reused
        # one instance, dispatched once per launch
        assert dispatched == [(row[9:], row[7])], (name, dispatched)


def test_host_routes_under_sanitizer(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    sources = [os.path.join(CSRC, f) for f in ("rs_kernels.hip", "rs_mixed.hip", "sha256.hip", "rs_plan.cpp",
                                               "rs_context.cpp", "rs_host.cpp")] + [
        os.path.join(NATIVE, f) for f in ("host_routes.cpp", "fake_hip_runtime.cpp", "fake_hip_memory.cpp")]
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
    exe = str(tmp_path / "host_routes")
    subprocess.run(["hipcc"] + SANITIZE + objs + ["-o", exe, "-no-pie"] +
                   ["-Wl,--defsym=%s=0" % s for s in fatbin], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("CALLFS_RS_")}
    env.update(CALLFS_RS_CHUNK_BYTES="65536", CALLFS_RS_SMALL_MAX_BYTES="0")
    for args, extra, want in (([], {}, expected(FIRST)),
                              (["inplace"], {"CALLFS_RS_INPLACE_PIPELINE": "1"}, expected(FIRST_INPLACE))):
        r = subprocess.run([exe] + args, capture_output=True, text=True, env=dict(env, **extra), timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "runtime error" not in r.stderr, r.stderr[-4000:]
        check(parse(r.stdout), want)
