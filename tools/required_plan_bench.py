#!/usr/bin/env python3
"""Times a data-only required plan (rs_plan_create_required) against the full
ragged plan of the same batch (rs_plan_create_ragged), on the download shape: §7.5's W1 batch
(256 x RS(10,4), shard sizes log-uniform 64 KiB..4 MiB), every stripe with one lost data shard
and exactly k shards present. The full plan rebuilds the four missing shards (14 S of traffic
per stripe), the required plan the data shard alone (11 S).

Several builds of the library are loaded side by side through ctypes and timed in alternation,
round after round (tools/host_batch_bench.py's protocol): `--lib name=path` more than once. A
library without rs_plan_create_required -- the parent commit's -- runs the full plan; one that
has it runs the required plan, and with `--full name` also the full plan. The spread between
two copies of the same library is the noise floor. One JSON line per (library, plan).

  python tools/required_plan_bench.py --lib parent=/tmp/parent/libcallfs_rs.so \\
      --lib new=callfs_amd/libcallfs_rs.so --lib new2=/tmp/copy_of_new.so --full new
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(os.path.dirname(HERE), "callfs_amd", "libcallfs_rs.so")
_vp, _sz, _int, _u8p = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8)


class Lib:
    def __init__(self, name, path):
        self.name = name
        self.so = so = ctypes.CDLL(path)
        so.rs_init.argtypes = [ctypes.POINTER(_vp), ctypes.c_uint]
        so.rs_plan_create_ragged.argtypes = [_vp, _int, _int, _int, _int, ctypes.POINTER(_sz), _u8p,
                                             ctypes.POINTER(_vp), ctypes.POINTER(_vp)]
        so.rs_plan_launch.argtypes = [_vp, _vp]
        so.rs_plan_status.argtypes = [_vp, _vp, ctypes.POINTER(_int)]
        so.rs_plan_bytes.argtypes = [_vp]
        so.rs_plan_bytes.restype = ctypes.c_uint64
        so.rs_plan_destroy.argtypes = [_vp]
        so.rs_plan_destroy.restype = None
        self.has_required = hasattr(so, "rs_plan_create_required")
        if self.has_required:
            so.rs_plan_create_required.argtypes = [_vp, _int, _int, _int, _int, ctypes.POINTER(_sz), _u8p,
                                                   _u8p, ctypes.POINTER(_vp), ctypes.POINTER(_vp)]
        self.ctx = _vp()
        rc = so.rs_init(ctypes.byref(self.ctx), 1)
        if rc:
            raise RuntimeError(f"{path}: rs_init -> {rc}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", action="append", default=[], help="name=path; repeat to compare builds")
    ap.add_argument("--full", action="append", default=[], help="also time this library's full plan")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default="required_plan.jsonl")
    a = ap.parse_args()
    libs = [Lib(*s.split("=", 1)) for s in (a.lib or [f"current={DEFAULT_LIB}"])]
    k, m, n = 10, 4, 14
    rng = np.random.default_rng(a.seed)
    sizes = [int(x) for x in np.exp(rng.uniform(np.log(64 << 10), np.log(4 << 20), 256))]
    B = len(sizes)
    dev = torch.device("cuda:0")
    pitch = [(S + 255) // 256 * 256 for S in sizes]
    off = np.concatenate(([0], np.cumsum([p * n for p in pitch])))
    buf = torch.empty(int(off[-1]) + 256, dtype=torch.uint8, device=dev)
    buf.random_(0, 256)
    base = (buf.data_ptr() + 255) // 256 * 256
    ptrs = (_vp * (B * n))(*[base + int(off[b]) + i * pitch[b] for b in range(B) for i in range(n)])
    szs = (_sz * B)(*sizes)
    lost = rng.integers(0, k, B)  # one data shard; three parity shards go with it: k present
    pres = (ctypes.c_uint8 * (B * n))(*[0 if (i == lost[b] or i > k) else 1 for b in range(B) for i in range(n)])
    want = (ctypes.c_uint8 * (B * n))(*[1 if i < k else 0 for _ in range(B) for i in range(n)])
    stream = torch.cuda.current_stream()
    s = _vp(stream.cuda_stream)

    plans = []  # (library, plan kind, handle)
    for lib in libs:
        kinds = ["required"] if lib.has_required else ["full"]
        if lib.has_required and lib.name in a.full:
            kinds.append("full")
        for kind in kinds:
            h = _vp()
            if kind == "required":
                rc = lib.so.rs_plan_create_required(lib.ctx, 0, k, m, B, szs, pres, want, ptrs, ctypes.byref(h))
            else:
                rc = lib.so.rs_plan_create_ragged(lib.ctx, 0, k, m, B, szs, pres, ptrs, ctypes.byref(h))
            if rc:
                raise RuntimeError(f"{lib.name} {kind}: create -> {rc}")
            plans.append((lib, kind, h))

    def timed(lib, h):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            rc = lib.so.rs_plan_launch(h, s)
            if rc:
                raise RuntimeError(f"{lib.name}: launch -> {rc}")
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / a.reps * 1e-3

    times = {(lib.name, kind): [] for lib, kind, _ in plans}
    for lib, kind, h in plans:  # warm-up; exactly k present: nothing is compared, nothing can flag
        timed(lib, h)
        c = _int(0)
        lib.so.rs_plan_status(h, s, ctypes.byref(c))
        if c.value:
            raise RuntimeError(f"{lib.name} {kind}: corrupt flag on a plan without compared rows")
    for _ in range(a.rounds):
        for lib, kind, h in plans:
            times[lib.name, kind].append(timed(lib, h))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        for lib, kind, h in plans:
            t = times[lib.name, kind]
            nbytes = int(lib.so.rs_plan_bytes(h))
            line = {"workload": "W1-download", "k": k, "m": m, "stripes": B, "shard_bytes": sum(sizes),
                    "lib": lib.name, "plan": kind, "plan_bytes": nbytes, "reps_per_round": a.reps,
                    "seconds": [round(x, 7) for x in t], "median_s": statistics.median(t),
                    "us_per_launch": round(statistics.median(t) * 1e6, 1),
                    "gb_per_s": round(nbytes / statistics.median(t) / 1e9, 1)}
            out.write(json.dumps(line) + "\n")
            print(json.dumps({key: line[key] for key in ("lib", "plan", "plan_bytes", "us_per_launch", "gb_per_s")}),
                  flush=True)
            lib.so.rs_plan_destroy(h)
    return 0


if __name__ == "__main__":
    sys.exit(main())
