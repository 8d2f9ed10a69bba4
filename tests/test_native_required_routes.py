"""The routes of rs_plan_create_required pinned on the CPU:
tests/native/required_routes.cpp links host-only builds of the device-plan code and the kernel
files against recording stand-ins for the HIP runtime (tests/native/fake_hip_runtime.cpp,
fake_hip_memory.cpp), builds a plan per route and prints what one launch dispatches. Built
under ASan + UBSan; a stand-alone program: nothing is loaded into Python."""
import concurrent.futures
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
CSRC = os.path.join(ROOT, "callfs_amd", "csrc")
SOURCES = [os.path.join(CSRC, f) for f in ("rs_kernels.hip", "rs_mixed.hip", "sha256.hip", "rs_plan.cpp",
                                           "rs_context.cpp")] + [
    os.path.join(NATIVE, f) for f in ("required_routes.cpp", "fake_hip_runtime.cpp", "fake_hip_memory.cpp")]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-fno-omit-frame-pointer"]


def build(exe, workdir):
    """Every source compiled for the host only; host-only compilation leaves the fat binaries'
    data symbols undefined: they are defined as 0 at link time (the stand-ins never read them)."""
    flags = ["--cuda-host-only", "-std=c++17", "-O1", "-I", CSRC, "-I", NATIVE] + SANITIZE

    def compile_one(src):
        obj = os.path.join(workdir, os.path.basename(src) + ".o")
        subprocess.run(["hipcc"] + flags + ["-x", "hip", "-c", src, "-o", obj], check=True)
        return obj

    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    undefined = subprocess.run(["nm", "-u"] + objs, check=True, capture_output=True, text=True).stdout
    fatbin = sorted({w for w in undefined.split() if w.startswith("__hip_fatbin_")})
    subprocess.run(["hipcc"] + SANITIZE + objs + ["-o", exe, "-no-pie"] +
                   ["-Wl,--defsym=%s=0" % s for s in fatbin], check=True)


def test_routes_dispatch_their_kernels(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "required_routes")
    build(exe, str(tmp_path))
    env = {k: v for k, v in os.environ.items() if not k.startswith("CALLFS_RS_")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "required_routes ok", r.stdout[-2000:] + r.stderr[-4000:]
    cases, name = {}, None
    for line in lines[:-1]:
        w = line.split()
        if w[0] == "case":
            name = w[1].rstrip(":")
            cases[name] = []
        else:
            assert w[0] == "dispatch", line
            cases[name].append(w[1])
    assert sorted(cases) == sorted(["null", "all-wanted", "uniform", "uniform-no-rows", "required",
                                    "required-no-rows", "required-two-groups"])

    def kernel(symbol):
        for name in ("rs_apply_ragged_some", "rs_apply_ragged", "rs_apply_mixed"):
            if "%d%sI" % (len(name), name) in symbol:  # (the mangled name and its length)
                return name
        return "uniform" if "rs_apply" in symbol else symbol

    got = {name: [kernel(s) for s in syms] for name, syms in cases.items()}
    # nothing left out: the ragged plan's kernel
    assert got["null"] == ["rs_apply_ragged"] and got["all-wanted"] == ["rs_apply_ragged"]
    # one size, one (mask, wanted) pair: a uniform kernel
    assert got["uniform"] == ["uniform"]
    # a wanted subset over ragged stripes: the new kernel, once per launch group
    assert got["required"] == ["rs_apply_ragged_some"]
    assert got["required-two-groups"] == ["rs_apply_ragged_some"] * 2
    assert "ILi16E" in cases["required-two-groups"][0] and "ILi4E" in cases["required-two-groups"][1]
    # a plan with no stripes in any launch group dispatches nothing
    assert got["uniform-no-rows"] == [] and got["required-no-rows"] == []
