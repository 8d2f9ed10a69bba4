"""The HIP-free parts of the checksummed codec batches, built with g++ under
AddressSanitizer+UBSan and run on the CPU as stand-alone programs: the message table, its slot
mapping and the device / host rule (callfs_amd/csrc/sums_table.hpp), and the host-hash route
with the follow-up run's bookkeeping against a software SHA-256 (sums_host.hpp,
sha256_host.hpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "callfs_amd", "csrc")


def _run(tmp_path, name, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", INC,
                    os.path.join(ROOT, "tests", "native", name + ".cpp"), *extra, "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1].startswith(name + " ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr
    return r.stdout


def test_sums_table_under_sanitizer(tmp_path):
    _run(tmp_path, "sums_table_test")


def test_sums_host_route_under_sanitizer(tmp_path):
    _run(tmp_path, "sums_host_test", ["-pthread"])
