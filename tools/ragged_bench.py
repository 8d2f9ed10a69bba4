"""Ragged plans against their alternatives, timed in one process.

Per workload, on resident batches in the planar layout with 256-B aligned shards (every
stripe's data shards in one region, the parity shards in another), every stripe its own
random m-erasure pattern:
  (a) mixed   one mixed plan of the same stripe count and the same masks at the mean shard
              size: the equal-bytes reference (a batch of its own);
  (b) ragged  one ragged plan over the stripes' own sizes;
  (c) split   the alternative to (b) without ragged plans: one mixed plan per distinct shard
              size over the stripes of that size, launched back to back on one stream.
Workloads: `rs10_4` RS(10,4), 256 stripes, sizes log-uniform in 64 KiB..4 MiB; `rs16_4`
RS(16,4), 4,096 stripes, sizes uniform in 1..16 KiB.
Each variant is warmed up, then timed over `--reps` launches with rs_plan_launch_timed
events (the kernels' own time, first dispatch start to last dispatch end; for (c) from the
first plan's first dispatch to the last plan's last); the median counts. The variants are
interleaved over `--rounds` rounds. Prints one JSON line per workload: median microseconds,
GB/s of algorithmic bytes, the ratios b/a (per byte) and c/b, and the plan-creation times.
usage: python tools/ragged_bench.py [--workload rs10_4] [--workload rs16_4]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from callfs_amd import _native as N  # noqa: E402
from callfs_amd.device import Plan, StripeBatch  # noqa: E402
from tools.mixed_bench import distinct_masks, timed  # noqa: E402

WORKLOADS = {
    # name: (k, m, stripes, size distribution, lowest, highest shard bytes)
    "rs10_4": (10, 4, 256, "loguniform", 64 << 10, 4 << 20),
    "rs16_4": (16, 4, 4096, "uniform", 1, 16 << 10),
}


def draw_sizes(kind, lo, hi, count, seed):
    rng = np.random.default_rng(seed)
    if kind == "loguniform":
        x = np.exp(rng.uniform(np.log(lo), np.log(hi), count))
        return [int(min(hi, max(lo, round(v)))) for v in x]
    return [int(v) for v in rng.integers(lo, hi + 1, count)]


def planar_offsets(k, m, sizes):
    """Byte offset of every shard, stripe-major: the data shards of every stripe in one
    region, the parity shards in another, each shard at the next 256-B boundary."""
    offs = [[0] * (k + m) for _ in sizes]
    at = 0
    for lo, hi in ((0, k), (k, k + m)):
        for b, S in enumerate(sizes):
            for i in range(lo, hi):
                at = (at + 255) // 256 * 256
                offs[b][i] = at
                at += S
    return offs, at


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append", choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm-ms", type=float, default=150.0)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    for name in a.workload or sorted(WORKLOADS):
        k, m, B, kind, lo, hi = WORKLOADS[name]
        n = k + m
        sizes = draw_sizes(kind, lo, hi, B, a.seed)
        total = sum(sizes)
        mean = max(1, round(total / B))
        masks, ndistinct = distinct_masks(n, m, B, a.seed)
        # the ragged batch: one allocation, planar, 256-B aligned shards
        offs, nbytes = planar_offsets(k, m, sizes)
        raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        lead = -raw.data_ptr() % 256
        g = torch.Generator(device=dev)
        g.manual_seed(0xCA11F5)
        raw.random_(0, 256, generator=g)
        base = raw.data_ptr() + lead
        ptrs = [base + o for row in offs for o in row]
        enc = Plan.ragged(k, m, sizes, ptrs)  # consistent parity
        enc.launch(stream)
        torch.cuda.synchronize()
        enc.close()
        # the equal-bytes reference: the same stripe count at the mean size
        sb = StripeBatch(k, m, mean, B, dev, layout="planar")
        sb.fill_random(0xCA11F5)
        Plan.for_batch(sb).launch(stream)
        torch.cuda.synchronize()

        t0 = time.perf_counter()
        mixed = Plan.for_batch(sb, present=masks)
        t1 = time.perf_counter()
        ragged = Plan.ragged(k, m, sizes, ptrs, present=masks)
        t2 = time.perf_counter()
        by_size = {}
        for b, S in enumerate(sizes):
            by_size.setdefault(S, []).append(b)
        split = []
        for S, ids in sorted(by_size.items()):
            p = [ptrs[b * n + i] for b in ids for i in range(n)]
            split.append(Plan(k, m, S, len(ids), p, present=[masks[b] for b in ids]))
        t3 = time.perf_counter()

        def ev(e):
            return ctypes.c_void_p(e.cuda_event) if e is not None else None

        def launch_split(e0, e1):
            last = len(split) - 1
            for j, p in enumerate(split):
                N.check(N.lib.rs_plan_launch_timed(p.handle, sp, ev(e0 if j == 0 else None),
                                                   ev(e1 if j == last else None)), "split")

        variants = {
            "mixed": lambda e0, e1: mixed.launch(stream, events=(e0, e1)),
            "ragged": lambda e0, e1: ragged.launch(stream, events=(e0, e1)),
            "split": launch_split,
        }
        for fn in variants.values():  # warm-up by time
            w0 = time.perf_counter()
            while (time.perf_counter() - w0) * 1e3 < a.warm_ms:
                timed(fn, 2)
        ms = {v: [] for v in variants}
        names = list(variants)
        for r in range(a.rounds):
            for v in names[r % len(names):] + names[:r % len(names)]:
                ms[v].append(timed(variants[v], a.reps))
        med = {v: statistics.median(x) for v, x in ms.items()}
        nb = {"mixed": mixed.bytes, "ragged": ragged.bytes, "split": sum(p.bytes for p in split)}
        assert nb["ragged"] == n * total == nb["split"] and nb["mixed"] == B * n * mean
        flagged = [v for v, p in (("mixed", mixed), ("ragged", ragged)) if p.corrupt(stream)]
        tiles = sum(max(1, -(-(S // 16) // 512)) for S in sizes)
        print(json.dumps({
            "workload": name, "k": k, "m": m, "stripes": B, "sizes": kind, "size_min": min(sizes),
            "size_max": max(sizes), "size_mean": mean, "distinct_sizes": len(by_size),
            "layout": "planar, 256-B aligned shards", "bytes": nb, "patterns": ndistinct,
            "tiles": tiles, "tile_map_bytes": 4 * tiles,
            "forms": {"mixed": mixed.forms(), "ragged": ragged.forms(),
                      "split": sorted({f for p in split for f in p.forms()})},
            "us": {v: round(x * 1e3, 2) for v, x in med.items()},
            "us_rounds": {v: [round(y * 1e3, 2) for y in x] for v, x in ms.items()},
            "GBps": {v: round(nb[v] / (x * 1e-3) / 1e9, 1) for v, x in med.items()},
            "ragged_over_mixed_per_byte": round((med["ragged"] / nb["ragged"]) / (med["mixed"] / nb["mixed"]), 4),
            "split_over_ragged": round(med["split"] / med["ragged"], 3),
            "plan_create_ms": {"mixed": round((t1 - t0) * 1e3, 2), "ragged": round((t2 - t1) * 1e3, 2),
                               "split": round((t3 - t2) * 1e3, 2)},
            "split_plans": len(split), "reps": a.reps, "rounds": a.rounds,
            "verify_flagged": flagged}), flush=True)
        for p in [mixed, ragged] + split:
            p.close()
        del sb, raw
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
