"""The per-object plan of the codec-level batch calls (callfs_amd/csrc/codec_batch.hpp: Split's
shape of an object, the source of every input row, the tee spans of an encode and the join
spans of a decode at column cuts) built with g++ under AddressSanitizer+UBSan and run on the
CPU as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "codec_batch_test.cpp")
INC = os.path.join(ROOT, "callfs_amd", "csrc")


def test_codec_batch_plan_under_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "codec_batch_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", INC, SRC,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "codec_batch_test ok", r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr
