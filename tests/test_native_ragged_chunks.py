"""The work list, chunk packing and staging layout of heterogeneous host batches
(callfs_amd/csrc/ragged_chunks.hpp) and the missing-rows form of the mixed tables, built with
g++ under AddressSanitizer+UBSan and run on the CPU as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ragged_chunks_test.cpp")
INC = os.path.join(ROOT, "callfs_amd", "csrc")


def test_ragged_chunks_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "ragged_chunks_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", INC, SRC,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "ragged_chunks_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr
