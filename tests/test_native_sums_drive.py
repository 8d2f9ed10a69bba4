"""tests/native/sums_drive.c: rs_codec_encode_batch_sums / rs_codec_decode_batch_sums driven the
way the cgo shim drives them (go/erasure/codec_rocm_sums.go: C-malloc'd pointer, lens, size,
status, digest and flag arrays, nil entries as lens 0, bodies split in place, a mismatching
shard rebuilt inside its own buffer). CPU: AddressSanitizer + UBSan build of the driver, the
argument and status paths that need no device. GPU: plain build, mixed batches against the C
oracle and the FIPS 180-4 "abc" vector."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sums_drive.c")


def _build(out, sanitize):
    from oracle import cref
    cref.build()
    flags = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    subprocess.run(["gcc", "-std=c11", "-O1", *flags, "-I", os.path.join(ROOT, "include"), SRC,
                    "-o", str(out), "-L", os.path.join(ROOT, "callfs_amd"), "-lcallfs_rs",
                    "-L", os.path.join(ROOT, "oracle", "build"), "-lrs_oracle",
                    "-Wl,-rpath," + os.path.join(ROOT, "callfs_amd"),
                    "-Wl,-rpath," + os.path.join(ROOT, "oracle", "build")], check=True)


def test_sums_drive_argument_paths_asan(tmp_path, native_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu variant")
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    exe = tmp_path / "sums_drive_asan"
    _build(exe, sanitize=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sums_drive ok (argument paths" in r.stdout
    assert "runtime error" not in r.stderr, r.stderr


@pytest.mark.gpu
def test_sums_drive_device(tmp_path, native_lib):
    exe = tmp_path / "sums_drive"
    _build(exe, sanitize=False)
    r = subprocess.run([str(exe), "gpu"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sums_drive ok (device round trips)" in r.stdout
