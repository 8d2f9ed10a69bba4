#!/usr/bin/env python3
"""Checksummed codec batches on the staged transport: where the shards' SHA-256
is cheapest. Per (profile, shard size) one call holds at least 64 MiB of objects and is timed

  host     rs_codec_*_batch_sums with CALLFS_RS_SUMS_DEVICE=0 (the copy pool's threads hash)
  device   the same with CALLFS_RS_SUMS_DEVICE=1 (sha256_rows in every chunk)
  auto     the same with the knob unset (the rule of csrc/sums_table.hpp)
  parent   what a caller did before these calls: rs_codec_encode_batch, then hashlib.sha256 over
           every shard on 16 threads (the CPU leg of tools/sha_bench.py); for a decode the
           hashes and their comparison first, then rs_codec_decode_batch

for the encode and for the decode of the same objects with every shard present and clean. The
knob is read once per process, so every (shape, route) runs in a process of its own (`--worker`):
two warm-up calls, then --rounds timed calls, host clock around the call (every call ends in
the pipeline's last event wait). The driver runs the routes of a shape one after another and
the whole list --passes times, so that a drift of the shared machine shows as a difference
between the passes. One JSON line per (shape, route, pass) on stdout and in --out.

  python tools/sums_bench.py --out profiles/r08/sums/sums.jsonl
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [256, 1024, 4096, 16384, 65536, 262144]
PROFILES = [(10, 4), (16, 4)]
ROUTE_ENV = {"host": "0", "device": "1", "auto": None, "parent": None}


def _ptr_array(base, offsets):
    return (ctypes.c_void_p * len(offsets))(*[base + int(o) for o in offsets])


def _hash_all(views, threads):
    """hashlib over every view, `threads` threads, a contiguous share each."""
    step = -(-len(views) // threads)
    parts = [views[i:i + step] for i in range(0, len(views), step)]
    with ThreadPoolExecutor(threads) as ex:
        return [d for part in ex.map(lambda p: [hashlib.sha256(v).digest() for v in p], parts) for d in part]


def worker(args):
    from callfs_amd import _native as Nat
    k, m, S, route = args.k, args.m, args.S, args.route
    n = k + m
    B = max(1, -(-args.bytes // (k * S)))
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, B * k * S, dtype=np.uint8)
    shards = np.zeros(B * n * S, np.uint8)
    outs = np.zeros(B * k * S, np.uint8)
    digests = np.zeros(B * n * 32, np.uint8)
    bad = np.zeros(B * n, np.uint8)
    cx = Nat.default_context()
    L = Nat.lib
    dptr = _ptr_array(data.ctypes.data, np.arange(B) * (k * S))
    sptr = _ptr_array(shards.ctypes.data, np.arange(B) * (n * S))
    shard_ptr = _ptr_array(shards.ctypes.data, np.arange(B * n) * S)
    optr = _ptr_array(outs.ctypes.data, np.arange(B) * (k * S))
    lens = (ctypes.c_size_t * B)(*([k * S] * B))
    caps = (ctypes.c_size_t * B)(*([n * S] * B))
    sizes = (ctypes.c_size_t * B)()
    status = (ctypes.c_int * B)()
    orig = (ctypes.c_int64 * B)(*([k * S] * B))
    mv = memoryview(shards)
    views = [mv[i * S:(i + 1) * S] for i in range(B * n)]

    def encode():
        if route == "parent":
            rc = L.rs_codec_encode_batch(cx.handle, k, m, B, dptr, lens, sptr, caps, sizes, status)
            digests[:] = np.frombuffer(b"".join(_hash_all(views, args.cpu_threads)), np.uint8)
            return rc
        return L.rs_codec_encode_batch_sums(cx.handle, k, m, B, dptr, lens, sptr, caps, sizes,
                                            digests.ctypes.data, status)

    def decode():
        slens = (ctypes.c_size_t * (B * n))(*([S] * (B * n)))
        if route == "parent":
            got = np.frombuffer(b"".join(_hash_all(views, args.cpu_threads)), np.uint8)
            bad[:] = (got.reshape(-1, 32) != digests.reshape(-1, 32)).any(axis=1)
            return L.rs_codec_decode_batch(cx.handle, k, m, B, shard_ptr, slens, optr, orig, status)
        return L.rs_codec_decode_batch_sums(cx.handle, k, m, B, shard_ptr, slens, digests.ctypes.data, optr,
                                            orig, bad.ctypes.data, status)

    res = {"k": k, "m": m, "S": S, "objects": B, "object_bytes": B * k * S, "shards": B * n, "route": route,
           "rounds": args.rounds}
    for name, fn in (("encode", encode), ("decode", decode)):
        for _ in range(2):
            assert fn() == 0, name
        times = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            rc = fn()
            times.append(time.perf_counter() - t0)
            assert rc == 0, name
        res[name + "_ms"] = [round(t * 1e3, 3) for t in times]
        res[name + "_median_ms"] = round(statistics.median(times) * 1e3, 3)
        res[name + "_gbps"] = round(B * k * S / statistics.median(times) / 1e9, 3)
    # what was computed: the digests against hashlib on a sample, the decode's output and flags
    step = max(1, B * n // 64)
    for i in range(0, B * n, step):
        assert digests[32 * i:32 * i + 32].tobytes() == hashlib.sha256(views[i]).digest(), i
    assert not bad.any() and (outs == data).all()
    c = Nat.HostCounters()
    L.rs_host_counters_read(cx.handle, ctypes.byref(c))
    res["counters"] = {f: int(getattr(c, f)) for f, _ in c._fields_}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--worker", action="store_true")
    p.add_argument("--k", type=int)
    p.add_argument("--m", type=int)
    p.add_argument("--S", type=int)
    p.add_argument("--route", choices=sorted(ROUTE_ENV))
    p.add_argument("--bytes", type=int, default=64 << 20, help="object bytes per call, at least")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--passes", type=int, default=2)
    p.add_argument("--cpu-threads", type=int, default=16)
    p.add_argument("--sizes", default=",".join(map(str, SIZES)))
    p.add_argument("--routes", default="host,device,parent")
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.worker:
        return worker(args)
    lines = []
    for ps in range(args.passes):
        for k, m in PROFILES:
            for S in [int(x) for x in args.sizes.split(",")]:
                for route in args.routes.split(","):
                    env = dict(os.environ)
                    env.pop("CALLFS_RS_SUMS_DEVICE", None)
                    if ROUTE_ENV[route] is not None:
                        env["CALLFS_RS_SUMS_DEVICE"] = ROUTE_ENV[route]
                    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--k", str(k), "--m", str(m),
                           "--S", str(S), "--route", route, "--bytes", str(args.bytes), "--rounds",
                           str(args.rounds), "--cpu-threads", str(args.cpu_threads)]
                    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
                    got = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                    if r.returncode != 0 or not got:
                        # a worker that did not end cleanly ends the sweep: nothing more is started
                        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                        return 1
                    rec = json.loads(got[-1][len("RESULT "):])
                    rec["pass"] = ps
                    line = json.dumps(rec)
                    print(line, flush=True)
                    lines.append(line)
                    if args.out:
                        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                        with open(args.out, "w") as fh:
                            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
