#!/usr/bin/env python3
"""Times rs_encode_batch / rs_reconstruct_batch over heterogeneous host batches.

Seeded, single-threaded workloads, each as an encode and as a reconstruct (one random lost
shard per stripe, verify on), with pageable and with rs_host_alloc (pinned) buffers:

  W0  256 stripes   RS(10,4)  1 MiB shards, one group (control: the uniform path)
  W1  256 stripes   RS(10,4)  log-uniform 64 KiB..4 MiB
  W2  4,096 stripes RS(16,4)  uniform 1..16 KiB
  W3  32 stripes    RS(10,4)  uniform 100 B..6.4 KiB (the small-uploads batch)

Several builds of the library are loaded side by side in one process through ctypes (each
has its own context and settings; they share the HIP runtime) and timed in alternation, round
after round, so drift hits all alike: `--lib name=path` more than once, e.g. the parent
commit's build as the baseline and the current one twice (the spread between two runs of the
same library is the noise floor; the second run needs a copy of the file under another name,
since one path loads once). One JSON line per (workload, leg, memory, library) with every
round's time, the median and -- where the library has rs_host_counters_read -- the counters of
one call.

  python tools/host_batch_bench.py --lib parent=/tmp/parent/libcallfs_rs.so \\
      --lib new=callfs_amd/libcallfs_rs.so --lib new2=/tmp/copy_of_new.so --rounds 5

`--crossover` instead times W3-like batches scaled from 64 KiB to 8 MiB of staging on one
library; run it once with CALLFS_RS_SMALL_MAX_BYTES=0 (staged) and once with a large value (in
place) to find where the two transports cross.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(os.path.dirname(HERE), "callfs_amd", "libcallfs_rs.so")

_vp, _sz, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int


class Counters(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("calls", "chunks", "launches", "copies", "ragged_calls")]


class Lib:
    def __init__(self, name, path):
        self.name, self.path = name, path
        self.so = ctypes.CDLL(path)
        for fn, args in (("rs_init", [ctypes.POINTER(_vp), ctypes.c_uint]), ("rs_shutdown", [_vp]),
                         ("rs_host_alloc", [_vp, _sz, ctypes.POINTER(_vp)]), ("rs_host_free", [_vp, _vp]),
                         ("rs_encode_batch", [_vp, _int, _int, _int, ctypes.POINTER(_sz), ctypes.POINTER(_vp),
                                              ctypes.POINTER(_vp), ctypes.POINTER(_int)]),
                         ("rs_reconstruct_batch", [_vp, _int, _int, _int, ctypes.POINTER(_vp),
                                                   ctypes.POINTER(_sz), _int, ctypes.POINTER(_int)])):
            f = getattr(self.so, fn)
            f.argtypes = args
            f.restype = None if fn == "rs_shutdown" else _int
        self.ctx = _vp()
        rc = self.so.rs_init(ctypes.byref(self.ctx), 1)  # one device
        if rc:
            raise RuntimeError(f"{path}: rs_init -> {rc}")
        self.has_counters = hasattr(self.so, "rs_host_counters_read")

    def counters(self):
        if not self.has_counters:
            return None
        c = Counters()
        self.so.rs_host_counters_read(self.ctx, ctypes.byref(c))
        return {n: int(getattr(c, n)) for n, _ in c._fields_}

    def pinned(self, nbytes):
        p = _vp()
        rc = self.so.rs_host_alloc(self.ctx, nbytes, ctypes.byref(p))
        if rc:
            raise RuntimeError(f"rs_host_alloc({nbytes}) -> {rc}")
        return p.value, np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(p.value))

    def free(self, ptr):
        self.so.rs_host_free(self.ctx, _vp(ptr))


def workload(name, rng):
    if name == "W0":
        return 10, 4, [1 << 20] * 256
    if name == "W1":
        return 10, 4, [int(x) for x in np.exp(rng.uniform(np.log(64 << 10), np.log(4 << 20), 256))]
    if name == "W2":
        return 16, 4, [int(x) for x in rng.integers(1 << 10, (16 << 10) + 1, 4096)]
    if name == "W3":
        return 10, 4, [int(x) for x in rng.integers(100, 6401, 32)]
    raise ValueError(name)


class Batch:
    """One flat buffer holding every shard of every stripe (shard i of stripe b at off[b] + i*S_b,
    16-B aligned), the pointer tables of both calls and the lost shard of every stripe."""

    def __init__(self, k, m, sizes, base, arr, rng_seed):
        self.k, self.m, self.n, self.sizes, self.arr = k, m, k + m, sizes, arr
        n, B = k + m, len(sizes)
        self.B = B
        pitch = [(S + 15) // 16 * 16 for S in sizes]
        off = np.concatenate(([0], np.cumsum([p * n for p in pitch])))
        self.shard_ptr = [[base + int(off[b]) + i * pitch[b] for i in range(n)] for b in range(B)]
        self.csizes = (_sz * B)(*sizes)
        self.data = (_vp * (B * k))(*[self.shard_ptr[b][i] for b in range(B) for i in range(k)])
        self.parity = (_vp * (B * m))(*[self.shard_ptr[b][k + j] for b in range(B) for j in range(m)])
        self.shards = (_vp * (B * n))(*[p for row in self.shard_ptr for p in row])
        self.lost = np.random.default_rng(rng_seed).integers(0, n, B)
        self.lens = (_sz * (B * n))()
        self.status = (_int * B)()

    @staticmethod
    def nbytes(k, m, sizes):
        return sum((S + 15) // 16 * 16 * (k + m) for S in sizes)

    def encode(self, lib):
        return lib.so.rs_encode_batch(lib.ctx, self.k, self.m, self.B, self.csizes, self.data, self.parity,
                                      self.status)

    def reset_lens(self):
        n = self.n
        for b, S in enumerate(self.sizes):
            for i in range(n):
                self.lens[b * n + i] = S
            self.lens[b * n + int(self.lost[b])] = 0

    def reconstruct(self, lib):
        return lib.so.rs_reconstruct_batch(lib.ctx, self.k, self.m, self.B, self.shards, self.lens, 1,
                                           self.status)


def fill_random(arr, rng):
    block = rng.integers(0, 256, 1 << 22, dtype=np.uint8)
    for at in range(0, arr.size, block.size):
        n = min(block.size, arr.size - at)
        arr[at:at + n] = np.roll(block, at // block.size)[:n]


def time_leg(batch, lib, leg, reps):
    """Seconds per call: the faster of two for the large workloads, the median of many for the
    small ones."""
    all_dt = []
    for _ in range(reps):
        if leg == "rec":
            batch.reset_lens()
        t0 = time.perf_counter()
        rc = batch.encode(lib) if leg == "enc" else batch.reconstruct(lib)
        dt = time.perf_counter() - t0
        if rc:
            raise RuntimeError(f"{lib.name} {leg}: rc={rc}")
        all_dt.append(dt)
    return min(all_dt) if reps <= 3 else statistics.median(all_dt)


def run_workload(name, libs, rounds, out, seed):
    rng = np.random.default_rng(seed)
    k, m, sizes = workload(name, rng)
    total = Batch.nbytes(k, m, sizes)
    reps = 200 if total < (8 << 20) else 2
    for mem in ("pageable", "pinned"):
        batches, frees = {}, []
        for lib in libs:
            if mem == "pageable":
                if "shared" not in batches:
                    arr = np.empty(total + 16, np.uint8)
                    base = (arr.ctypes.data + 15) // 16 * 16
                    view = arr[base - arr.ctypes.data:][:total]
                    fill_random(view, rng)
                    batches["shared"] = Batch(k, m, sizes, base, view, seed)
                batches[lib.name] = batches["shared"]
            else:
                try:
                    base, arr = lib.pinned(total)
                except RuntimeError as e:  # e.g. a locked-memory limit: say so, go on
                    out.write(json.dumps({"workload": name, "memory": mem, "skipped": str(e)}) + "\n")
                    print(f"{name} pinned skipped: {e}", flush=True)
                    for lb, bs in frees:
                        lb.free(bs)
                    return
                frees.append((lib, base))
                fill_random(arr, np.random.default_rng(seed + 1))
                batches[lib.name] = Batch(k, m, sizes, base, arr, seed)
        for leg in ("enc", "rec"):
            times = {lib.name: [] for lib in libs}
            counters = {}
            for lib in libs:  # warm-up: allocations, tables; the encode also makes the parity valid
                b = batches[lib.name]
                b.encode(lib)
                time_leg(b, lib, leg, 1)
                c0 = lib.counters()
                time_leg(b, lib, leg, 1)
                c1 = lib.counters()
                counters[lib.name] = c0 and {key: c1[key] - c0[key] for key in c0}
            for _ in range(rounds):
                for lib in libs:
                    times[lib.name].append(time_leg(batches[lib.name], lib, leg, reps))
            for lib in libs:
                t = times[lib.name]
                line = {"workload": name, "k": k, "m": m, "stripes": len(sizes), "bytes": total, "leg": leg,
                        "memory": mem, "lib": lib.name, "reps_per_round": reps,
                        "seconds": [round(x, 7) for x in t], "median_s": statistics.median(t),
                        "us_per_call": round(statistics.median(t) * 1e6, 1),
                        "gib_per_s": round(total / statistics.median(t) / 2**30, 2),
                        "counters_per_call": counters[lib.name]}
                out.write(json.dumps(line) + "\n")
                out.flush()
                print(json.dumps({key: line[key] for key in ("workload", "leg", "memory", "lib", "us_per_call",
                                                             "gib_per_s", "counters_per_call")}), flush=True)
        for lib, base in frees:
            lib.free(base)


def run_crossover(lib, rounds, out, seed):
    """W3-like batches scaled to 64 KiB .. 8 MiB of total staging, pageable."""
    for target in (64 << 10, 128 << 10, 256 << 10, 512 << 10, 1 << 20, 2 << 20, 4 << 20, 8 << 20):
        rng = np.random.default_rng(seed)
        k, m = 10, 4
        scale = target / (32 * 3250 * 14)
        sizes = [max(1, int(x * scale)) for x in rng.integers(100, 6401, 32)]
        total = Batch.nbytes(k, m, sizes)
        arr = np.empty(total + 16, np.uint8)
        base = (arr.ctypes.data + 15) // 16 * 16
        view = arr[base - arr.ctypes.data:][:total]
        fill_random(view, rng)
        b = Batch(k, m, sizes, base, view, seed)
        for leg in ("enc", "rec"):
            b.encode(lib)
            time_leg(b, lib, leg, 3)
            c0 = lib.counters()
            time_leg(b, lib, leg, 1)
            c1 = lib.counters()
            t = [time_leg(b, lib, leg, 50) for _ in range(rounds)]
            line = {"crossover_bytes": total, "leg": leg, "lib": lib.name,
                    "small_max": os.environ.get("CALLFS_RS_SMALL_MAX_BYTES"),
                    "us_per_call": round(statistics.median(t) * 1e6, 1),
                    "seconds": [round(x, 7) for x in t],
                    "counters_per_call": c0 and {key: c1[key] - c0[key] for key in c0}}
            out.write(json.dumps(line) + "\n")
            out.flush()
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", action="append", default=[], help="name=path; repeat to compare builds")
    ap.add_argument("--workloads", default="W0,W1,W2,W3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0x5EED)
    ap.add_argument("--out", default="host_batch.jsonl")
    ap.add_argument("--crossover", action="store_true")
    a = ap.parse_args()
    specs = a.lib or [f"current={DEFAULT_LIB}"]
    libs = [Lib(*s.split("=", 1)) for s in specs]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        if a.crossover:
            run_crossover(libs[0], a.rounds, out, a.seed)
        else:
            for w in a.workloads.split(","):
                run_workload(w, libs, a.rounds, out, a.seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
