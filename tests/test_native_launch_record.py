"""Kernel dispatch pinned on the CPU: tests/native/launch_record.cpp links a host-only build of
callfs_amd/csrc/rs_kernels.hip against a recording stand-in for the HIP runtime
(tests/native/fake_hip_runtime.cpp) and prints, per case of a seeded sweep, the rule's form and
a hash of every dispatch launch_apply and launch_ceiling issue (kernel symbol, grid, block,
LDS bytes, tail placement, slicing, event marking). tests/golden/launch_record/ holds the
record of the dispatch code before it was restructured around one decoded order form and one
select_kernel; the code must keep reproducing it, in both build flavours and under every
environment toggle. A stand-alone program: nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "callfs_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_record")

TILE_ORDERS = ["consecutive", "g8", "g2", "q8", "q16", "x8", "x32"]
# (environment, stride over the sweep's cases): the toggles are read once per process
COMMON = [({}, 1)] + [({"CALLFS_RS_TILE_ORDER": o}, 20) for o in TILE_ORDERS] + [
    ({"CALLFS_RS_MAX_TILES_PER_LAUNCH": "2048"}, 20)]
SETTINGS = {
    "product": COMMON,
    "ab": COMMON + [({"CALLFS_RS_WIX": "0"}, 20), ({"CALLFS_RS_TRIDB": "0"}, 20),
                    ({"CALLFS_RS_REALIGN": "0"}, 20), ({"CALLFS_RS_TAIL_LAST_TPS": "4"}, 20)],
}
TOGGLES = ["CALLFS_RS_TILE_ORDER", "CALLFS_RS_MAX_TILES_PER_LAUNCH", "CALLFS_RS_WIX",
           "CALLFS_RS_TRIDB", "CALLFS_RS_REALIGN", "CALLFS_RS_TAIL_LAST_TPS",
           "CALLFS_RS_TUNE_TABLE", "CALLFS_RS_BITSLICE"]


def build(csrc, flavour, exe, workdir, extra=()):
    """Compiles rs_kernels.hip for the host only and links the recorder against the fake
    runtime. Host-only compilation leaves the fat binary's data symbol undefined: it is
    defined as 0 at link time (the fake runtime never reads it)."""
    flags = ["--cuda-host-only", "-std=c++17", "-O1", "-I", csrc, "-I", NATIVE,
             "-DCALLFS_RS_AB_INSTANCES=%d" % (flavour == "ab")] + list(extra)
    objs = []
    for src in (os.path.join(csrc, "rs_kernels.hip"), os.path.join(NATIVE, "launch_record.cpp"),
                os.path.join(NATIVE, "fake_hip_runtime.cpp")):
        obj = os.path.join(workdir, flavour + "_" + os.path.basename(src) + ".o")
        subprocess.run(["hipcc"] + flags + ["-x", "hip", "-c", src, "-o", obj], check=True)
        objs.append(obj)
    undefined = subprocess.run(["nm", "-u", objs[0]], check=True, capture_output=True, text=True).stdout
    fatbin = [w for w in undefined.split() if w.startswith("__hip_fatbin_")]
    subprocess.run(["hipcc"] + list(extra) + objs + ["-o", exe, "-no-pie"] +
                   ["-Wl,--defsym=%s=0" % s for s in fatbin], check=True)


def run(exe, env_extra, args):
    env = {k: v for k, v in os.environ.items() if k not in TOGGLES}
    env.update(env_extra)
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "launch_record ok", r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()[:-1]


def section_name(env):
    return " ".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


def read_golden(flavour):
    sections, name = {}, None
    with open(os.path.join(GOLDEN, flavour + ".txt")) as f:
        for line in f.read().splitlines():
            if line.startswith("# "):
                name = line[2:]
                sections[name] = []
            else:
                sections[name].append(line)
    return sections


@pytest.mark.parametrize("flavour", ["product", "ab"])
def test_dispatch_matches_record(tmp_path, flavour):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / ("launch_record_" + flavour))
    build(CSRC, flavour, exe, str(tmp_path))
    golden = read_golden(flavour)
    assert sorted(golden) == sorted(section_name(env) for env, _ in SETTINGS[flavour])
    for env, stride in SETTINGS[flavour]:
        got = run(exe, env, ["--stride", str(stride)])
        want = golden[section_name(env)]
        assert len(got) == len(want), section_name(env)
        for g, w in zip(got, want):
            if g != w:
                case = g.split()[0]
                full = "\n".join(run(exe, env, ["--full", case]))
                pytest.fail("%s [%s]: the dispatch differs from the record\nrecord: %s\nnow:    %s\n%s"
                            % (flavour, section_name(env), w, g, full[-20000:]))


def test_wide_ring_launches_reach_sixteen_kernels(tmp_path):
    """The wide ring of rs_apply_lds has 16 instances (R 9..16 in consecutive order and in Q8),
    and ring_kernel() falls back silently to the consecutive one where a table entry is null: a
    byte-exact GPU test cannot tell which instance it ran. With the bit-sliced path off, the 16
    (R, order) pins must dispatch 16 different registered kernels, and the rule the Q8 one of
    its R from 256 tiles per stripe and the consecutive one below
    (tests/test_gpu_nibble_fallback.py runs the same launches on the GPU)."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "launch_record_product")
    build(CSRC, "product", exe, str(tmp_path))
    pinned, rule = {}, {}
    for line in run(exe, {}, ["--wide"]):
        w = line.split()
        if w[0] == "wide":
            pinned[int(w[1][2:]), w[2][len("order="):]] = w[3]
        else:
            assert w[0] == "rule", line
            rule[int(w[1][2:]), int(w[2][len("tiles="):])] = w[3]
    assert sorted(pinned) == [(R, o) for R in range(9, 17) for o in ("consecutive", "q8")]
    assert all("rs_apply_lds" in s for s in pinned.values()), pinned
    assert len(set(pinned.values())) == 16, pinned
    assert sorted(rule) == [(R, t) for R in range(9, 17) for t in (255, 256)]
    for R in range(9, 17):
        assert rule[R, 256] == pinned[R, "q8"], (R, rule[R, 256])
        assert rule[R, 255] == pinned[R, "consecutive"], (R, rule[R, 255])


def test_recorder_under_sanitizer(tmp_path):
    """The whole sweep, the codes between and beyond the order families included, with the
    dispatch code and the recorder built under ASan + UBSan (host code with its own main)."""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "launch_record_asan")
    build(CSRC, "ab", exe, str(tmp_path),
          extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                 "-fno-omit-frame-pointer"])
    got = run(exe, {}, [])
    assert got == read_golden("ab")["default"]
