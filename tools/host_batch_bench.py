#!/usr/bin/env python3
"""Times rs_encode_batch / rs_reconstruct_batch over heterogeneous host batches
and, with --codec, the codec-level batch calls against the routes they replace.

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

`--codec` instead times the codec-level batch calls on the same workloads
taken as objects: object length = k x the workload's shard size minus a seeded pad in [0, k),
as an encode (objects in, n shards per object out, separate buffers) and as a decode with one
seeded lost shard per object (shards in, objects out). A library that has
rs_codec_encode_batch / rs_codec_decode_batch is timed through them (route "batch"); one that
does not -- the parent commit's -- does the same job the two ways it can: route "a", a loop of
rs_codec_encode / rs_codec_decode per object, and route "b", CPU Split + rs_encode_batch and
rs_reconstruct_batch + CPU join (one copy per object each way, the cheapest a caller can do).
A library that has rs_codec_decode_data_batch is also timed through it on the
decode leg (route "data": only the lost data shards are rebuilt).

`--routes` instead times the other calls that take the chunk pipeline, through the same
alternation of libraries: rs_locate_batch and rs_correct_batch on clean stripes, rs_correct_batch
with one corrupt byte per stripe (corrupted again before every call, outside the timed part) and
rs_update_batch with one changed data shard per stripe.

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

_vp, _sz, _int, _i64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int64


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
        self.so.rs_codec_encode.argtypes = [_vp, _int, _int, _vp, _sz, _vp, _sz, ctypes.POINTER(_sz)]
        self.so.rs_codec_decode.argtypes = [_vp, _int, _int, ctypes.POINTER(_vp), ctypes.POINTER(_sz), _vp, _i64]
        self.has_codec_batch = hasattr(self.so, "rs_codec_encode_batch")
        if self.has_codec_batch:
            self.so.rs_codec_encode_batch.argtypes = [
                _vp, _int, _int, _int, ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(_vp),
                ctypes.POINTER(_sz), ctypes.POINTER(_sz), ctypes.POINTER(_int)]
            self.so.rs_codec_decode_batch.argtypes = [
                _vp, _int, _int, _int, ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(_vp),
                ctypes.POINTER(_i64), ctypes.POINTER(_int)]
        self.has_decode_data = hasattr(self.so, "rs_codec_decode_data_batch")
        if self.has_decode_data:
            self.so.rs_codec_decode_data_batch.argtypes = self.so.rs_codec_decode_batch.argtypes
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


class CodecBatch:
    """One flat buffer: every object's bytes, then every object's n shards back to back (the
    layout rs_codec_encode writes), then every joined object; regions and objects 64-B aligned."""

    def __init__(self, k, m, shard_sizes, base, arr, seed):
        rng = np.random.default_rng(seed + 7)
        self.k, self.m, self.n, self.arr, self.base = k, m, k + m, arr, base
        n, B = k + m, len(shard_sizes)
        self.B, self.S = B, shard_sizes
        self.L = [k * S - int(rng.integers(0, k)) if k * S > k else k * S for S in shard_sizes]
        al = lambda x: (x + 63) // 64 * 64  # noqa: E731
        self.d_off, self.s_off, self.o_off = [], [], []
        at = 0
        for L in self.L:
            self.d_off.append(at)
            at += al(L)
        for S in shard_sizes:
            self.s_off.append(at)
            at += al(n * S)
        for L in self.L:
            self.o_off.append(at)
            at += al(L)
        self.total = at
        self.lost = rng.integers(0, n, B)
        self.data = (_vp * B)(*[base + o for o in self.d_off])
        self.dst = (_vp * B)(*[base + o for o in self.s_off])
        self.out = (_vp * B)(*[base + o for o in self.o_off])
        self.clens = (_sz * B)(*self.L)
        self.caps = (_sz * B)(*[n * S for S in shard_sizes])
        self.csizes = (_sz * B)(*shard_sizes)
        self.ss = (_sz * B)()
        self.orig = (_i64 * B)(*self.L)
        self.status = (_int * B)()
        self.shards = (_vp * (B * n))(*[base + self.s_off[b] + i * shard_sizes[b] for b in range(B) for i in range(n)])
        self.dptr = (_vp * (B * k))(*[base + self.s_off[b] + i * shard_sizes[b] for b in range(B) for i in range(k)])
        self.pptr = (_vp * (B * m))(*[base + self.s_off[b] + (k + j) * shard_sizes[b] for b in range(B) for j in range(m)])
        self.lens = (_sz * (B * n))()
        self.lens0 = (_sz * (B * n))(*[0 if i == self.lost[b] else shard_sizes[b] for b in range(B) for i in range(n)])
        # per-object views of lens and shard pointers for the single-object decode
        psz, ssz = ctypes.sizeof(_vp), ctypes.sizeof(_sz)
        self.sh_b = [ctypes.cast(ctypes.addressof(self.shards) + b * n * psz, ctypes.POINTER(_vp)) for b in range(B)]
        self.ln_b = [ctypes.cast(ctypes.addressof(self.lens) + b * n * ssz, ctypes.POINTER(_sz)) for b in range(B)]
        self.one = _sz()

    @staticmethod
    def nbytes(k, m, shard_sizes):
        return sum(2 * (k * S + 64) + (k + m) * S + 64 for S in shard_sizes)

    def prepare(self, leg):
        if leg == "dec":
            ctypes.memmove(self.lens, self.lens0, ctypes.sizeof(self.lens))

    def run(self, lib, route, leg):
        so, ctx, k, m, B, a = lib.so, lib.ctx, self.k, self.m, self.B, self.arr
        if route == "data" and leg == "dec":
            return so.rs_codec_decode_data_batch(ctx, k, m, B, self.shards, self.lens, self.out, self.orig,
                                                 self.status)
        if route in ("batch", "data"):
            if leg == "enc":
                return so.rs_codec_encode_batch(ctx, k, m, B, self.data, self.clens, self.dst, self.caps, self.ss,
                                                self.status)
            return so.rs_codec_decode_batch(ctx, k, m, B, self.shards, self.lens, self.out, self.orig, self.status)
        if route == "a":
            rc = 0
            if leg == "enc":
                for b in range(B):
                    rc |= so.rs_codec_encode(ctx, k, m, self.data[b], self.L[b], self.dst[b], self.caps[b],
                                             ctypes.byref(self.one))
            else:
                for b in range(B):
                    rc |= so.rs_codec_decode(ctx, k, m, self.sh_b[b], self.ln_b[b], self.out[b], self.L[b])
            return rc
        if leg == "enc":  # route b: upstream Split on the CPU (copy the body, zero the pad), then the shard batch
            for L, S, d, s in zip(self.L, self.S, self.d_off, self.s_off):
                a[s:s + L] = a[d:d + L]
                a[s + L:s + k * S] = 0
            return so.rs_encode_batch(ctx, k, m, B, self.csizes, self.dptr, self.pptr, self.status)
        rc = so.rs_reconstruct_batch(ctx, k, m, B, self.shards, self.lens, 1, self.status)
        for L, s, o in zip(self.L, self.s_off, self.o_off):  # join + trim: the data shards lie end to end
            a[o:o + L] = a[s:s + L]
        return rc

    def joined_ok(self):
        return all(np.array_equal(self.arr[o:o + L], self.arr[d:d + L])
                   for L, d, o in zip(self.L, self.d_off, self.o_off))


def time_codec(batch, lib, route, leg, reps):
    all_dt = []
    for _ in range(reps):
        batch.prepare(leg)
        t0 = time.perf_counter()
        rc = batch.run(lib, route, leg)
        dt = time.perf_counter() - t0
        if rc:
            raise RuntimeError(f"{lib.name} {route} {leg}: rc={rc}")
        all_dt.append(dt)
    return min(all_dt) if reps <= 3 else statistics.median(all_dt)


def run_codec_workload(name, libs, rounds, out, seed):
    rng = np.random.default_rng(seed)
    k, m, sizes = workload(name, rng)
    total = CodecBatch.nbytes(k, m, sizes)
    reps = 200 if total < (16 << 20) else 2
    all_runs = [(lib, r) for lib in libs
                for r in ((("batch", "data") if lib.has_decode_data else ("batch",))
                          if lib.has_codec_batch else ("a", "b"))]
    for mem in ("pageable", "pinned"):
        batches, frees = {}, []
        for lib in libs:
            if mem == "pageable" and batches:
                batches[lib.name] = next(iter(batches.values()))
                continue
            if mem == "pageable":
                arr = np.empty(total + 64, np.uint8)
                base = (arr.ctypes.data + 63) // 64 * 64
                arr = arr[base - arr.ctypes.data:][:total]
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
            b = CodecBatch(k, m, sizes, base, arr, seed)
            fill_random(arr[:b.s_off[0]], np.random.default_rng(seed + 1))
            batches[lib.name] = b
        for leg in ("enc", "dec"):
            runs = [(lib, r) for lib, r in all_runs if r != "data" or leg == "dec"]
            times = {(lib.name, r): [] for lib, r in runs}
            counters = {}
            for lib, r in runs:  # warm-up: allocations, tables; the encode also makes the shards valid
                b = batches[lib.name]
                b.prepare("enc")
                b.run(lib, r, "enc")
                time_codec(b, lib, r, leg, 1)
                c0 = lib.counters()
                time_codec(b, lib, r, leg, 1)
                c1 = lib.counters()
                counters[lib.name, r] = c0 and {key: c1[key] - c0[key] for key in c0}
                if leg == "dec" and not b.joined_ok():
                    raise RuntimeError(f"{name} {mem} {lib.name} {r}: joined objects differ from the inputs")
            for _ in range(rounds):
                for lib, r in runs:
                    times[lib.name, r].append(time_codec(batches[lib.name], lib, r, leg, reps))
            obj_bytes = sum(batches[libs[0].name].L)
            for lib, r in runs:
                t = times[lib.name, r]
                line = {"workload": name, "k": k, "m": m, "objects": len(sizes), "object_bytes": obj_bytes,
                        "leg": "codec_" + leg, "memory": mem, "lib": lib.name, "route": r, "reps_per_round": reps,
                        "seconds": [round(x, 7) for x in t], "median_s": statistics.median(t),
                        "us_per_call": round(statistics.median(t) * 1e6, 1),
                        "gib_per_s": round(obj_bytes / statistics.median(t) / 2**30, 2),
                        "counters_per_call": counters[lib.name, r]}
                out.write(json.dumps(line) + "\n")
                out.flush()
                print(json.dumps({key: line[key] for key in ("workload", "leg", "memory", "lib", "route",
                                                             "us_per_call", "gib_per_s", "counters_per_call")}),
                      flush=True)
        for lib, base in frees:
            lib.free(base)


class RoutesBatch(Batch):
    """A Batch for the update, locate and correct calls: one changed data shard per stripe (its
    new bytes are the next data shard's), every shard present, and one byte per stripe to corrupt."""

    def __init__(self, k, m, sizes, base, arr, rng_seed):
        super().__init__(k, m, sizes, base, arr, rng_seed)
        n, B = self.n, self.B
        rng = np.random.default_rng(rng_seed + 11)
        changed = rng.integers(0, k, B)
        self.old = (_vp * (B * k))()
        self.new = (_vp * (B * k))()
        for b in range(B):
            c = int(changed[b])
            self.old[b * k + c] = self.shard_ptr[b][c]
            self.new[b * k + c] = self.shard_ptr[b][(c + 1) % k]
        self.full = (_sz * (B * n))(*[S for S in sizes for _ in range(n)])
        self.counts = (ctypes.c_uint64 * (B * (n + 1)))()
        cols = np.array([int(rng.integers(0, S)) for S in sizes], np.int64)
        ptrs = np.array([self.shard_ptr[b][int(self.lost[b])] for b in range(B)], np.int64)
        self.corrupt_at = ptrs - base + cols

    def prepare(self, leg):
        if leg == "correct_1":
            self.arr[self.corrupt_at] ^= 0x5A

    def run(self, lib, leg):
        so, ctx = lib.so, lib.ctx
        if leg == "update":
            return so.rs_update_batch(ctx, self.k, self.m, self.B, self.csizes, self.old, self.new, self.parity,
                                      self.status)
        fn = so.rs_locate_batch if leg == "locate" else so.rs_correct_batch
        return fn(ctx, self.k, self.m, self.B, self.shards, self.full, self.counts, self.status)


def time_route(batch, lib, leg, reps):
    all_dt = []
    for _ in range(reps):
        batch.prepare(leg)
        t0 = time.perf_counter()
        rc = batch.run(lib, leg)
        dt = time.perf_counter() - t0
        if rc:
            raise RuntimeError(f"{lib.name} {leg}: rc={rc}")
        all_dt.append(dt)
    return min(all_dt) if reps <= 3 else statistics.median(all_dt)


def run_routes_workload(name, libs, rounds, out, seed):
    """rs_locate_batch and rs_correct_batch on clean stripes, rs_correct_batch with one corrupt
    byte per stripe and rs_update_batch with one changed shard per stripe. The update leg comes
    last: it leaves the parity that of other data."""
    rng = np.random.default_rng(seed)
    k, m, sizes = workload(name, rng)
    total = Batch.nbytes(k, m, sizes)
    reps = 200 if total < (8 << 20) else 2
    sig = [_vp, _int, _int, _int, ctypes.POINTER(_vp), ctypes.POINTER(_sz), ctypes.POINTER(ctypes.c_uint64),
           ctypes.POINTER(_int)]
    for lib in libs:
        lib.so.rs_locate_batch.argtypes = lib.so.rs_correct_batch.argtypes = sig
        lib.so.rs_update_batch.argtypes = [_vp, _int, _int, _int, ctypes.POINTER(_sz), ctypes.POINTER(_vp),
                                           ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_int)]
    for mem in ("pageable", "pinned"):
        batches, frees = {}, []
        for lib in libs:
            if mem == "pageable":
                if "shared" not in batches:
                    arr = np.empty(total + 16, np.uint8)
                    base = (arr.ctypes.data + 15) // 16 * 16
                    view = arr[base - arr.ctypes.data:][:total]
                    fill_random(view, rng)
                    batches["shared"] = RoutesBatch(k, m, sizes, base, view, seed)
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
                batches[lib.name] = RoutesBatch(k, m, sizes, base, arr, seed)
        for leg in ("locate", "correct_clean", "correct_1", "update"):
            times = {lib.name: [] for lib in libs}
            counters = {}
            for lib in libs:  # warm-up: allocations, tables; the encode makes the parity valid
                b = batches[lib.name]
                if b.encode(lib):
                    raise RuntimeError(f"{lib.name}: rs_encode_batch failed")
                time_route(b, lib, leg, 1)
                c0 = lib.counters()
                time_route(b, lib, leg, 1)
                c1 = lib.counters()
                counters[lib.name] = c0 and {key: c1[key] - c0[key] for key in c0}
            for _ in range(rounds):
                for lib in libs:
                    times[lib.name].append(time_route(batches[lib.name], lib, leg, reps))
            for lib in libs:
                t = times[lib.name]
                line = {"workload": name, "k": k, "m": m, "stripes": len(sizes), "bytes": total, "leg": leg,
                        "memory": mem, "lib": lib.name, "reps_per_round": reps,
                        "seconds": [round(x, 7) for x in t], "median_s": statistics.median(t),
                        "us_per_call": round(statistics.median(t) * 1e6, 1),
                        "counters_per_call": counters[lib.name]}
                out.write(json.dumps(line) + "\n")
                out.flush()
                print(json.dumps({key: line[key] for key in ("workload", "leg", "memory", "lib", "us_per_call",
                                                             "counters_per_call")}), flush=True)
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
    ap.add_argument("--codec", action="store_true", help="the codec-level batch calls (objects in / out)")
    ap.add_argument("--routes", action="store_true",
                    help="rs_update_batch, rs_locate_batch and rs_correct_batch (DESIGN.md §7.5)")
    a = ap.parse_args()
    specs = a.lib or [f"current={DEFAULT_LIB}"]
    libs = [Lib(*s.split("=", 1)) for s in specs]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        if a.crossover:
            run_crossover(libs[0], a.rounds, out, a.seed)
        else:
            run = run_routes_workload if a.routes else run_codec_workload if a.codec else run_workload
            for w in a.workloads.split(","):
                run(w, libs, a.rounds, out, a.seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
