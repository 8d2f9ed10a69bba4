"""Mixed plans against their alternatives, timed in one process.

Per shape, on one resident planar batch whose parity the encode plan computed:
  (a) uniform  one plan, every stripe erasing the same shards ({0,3,7,12} for RS(10,4));
  (b) mixed    one mixed plan, every stripe its own random m-erasure pattern (distinct);
  (c) split    the alternative to (b) without mixed plans: one one-stripe uniform plan per
               stripe, launched back to back on one stream.
Two more variants split the gap between (a) and (b) into its parts:
  ring         (a) pinned to the mixed kernel's own form and tile order (the ring of three
               in consecutive order): what (b) would run at with one pattern;
  mixed2       a mixed plan with two patterns, alternating: the mixed kernel with its
               per-block table fetch served from L2.
Each variant is warmed up, then timed over `--reps` launches with rs_plan_launch_timed
events (the kernels' own time, first dispatch start to last dispatch end; for (c) from the
first plan's first dispatch to the last plan's last); the median counts. The variants are
interleaved over `--rounds` rounds. Prints one JSON line per shape: median microseconds,
GB/s of algorithmic bytes, and the ratios b/a, c/b, ring/a and b/mixed2.
usage: python tools/mixed_bench.py [--shape 10,4,1048576,256] [--shape 16,4,4096,4096]
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

DEFAULT_SHAPES = ["10,4,1048576,256", "16,4,4096,4096"]


def distinct_masks(n, m, batch, seed):
    """`batch` presence masks with m losses each, all distinct while C(n, m) allows."""
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    tries = 0
    while len(out) < batch:
        lost = tuple(sorted(int(i) for i in rng.choice(n, size=m, replace=False)))
        tries += 1
        if lost in seen and tries < 64 * batch:
            continue
        seen.add(lost)
        out.append([i not in lost for i in range(n)])
    return out, len(seen)


def timed(launch, reps):
    """Median ms of `reps` calls of launch(e0, e1), each synchronised on its own."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        launch(e0, e1)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="k,m,S,stripes (default: the two §5.8 shapes)")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm-ms", type=float, default=150.0)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sp = ctypes.c_void_p(stream.cuda_stream)
    for spec in a.shape or DEFAULT_SHAPES:
        k, m, S, B = (int(x) for x in spec.split(","))
        n = k + m
        sb = StripeBatch(k, m, S, B, dev, layout="planar")
        sb.fill_random(0xCA11F5)
        Plan.for_batch(sb).launch(stream)  # consistent parity
        torch.cuda.synchronize()
        uni_lost = (0, 3, 7, 12)[:m] if n > 12 else tuple(range(m))
        uni_mask = [i not in uni_lost for i in range(n)]
        masks, ndistinct = distinct_masks(n, m, B, a.seed)
        ptrs = sb.pointers()
        t0 = time.perf_counter()
        uniform = Plan.for_batch(sb, present=uni_mask)
        t1 = time.perf_counter()
        mixed = Plan.for_batch(sb, present=masks)
        t2 = time.perf_counter()
        split = [Plan(k, m, S, 1, ptrs[b * n:(b + 1) * n], present=masks[b]) for b in range(B)]
        t3 = time.perf_counter()
        ring = Plan.for_batch(sb, present=uni_mask)
        ring.set_orders(["consecutive"] * len(ring.forms()))
        mixed2 = Plan.for_batch(sb, present=[masks[b % 2] for b in range(B)])

        def ev(e):
            return ctypes.c_void_p(e.cuda_event) if e is not None else None

        def launch_split(e0, e1):
            last = len(split) - 1
            for j, p in enumerate(split):
                N.check(N.lib.rs_plan_launch_timed(p.handle, sp, ev(e0 if j == 0 else None),
                                                   ev(e1 if j == last else None)), "split")

        variants = {
            "uniform": lambda e0, e1: uniform.launch(stream, events=(e0, e1)),
            "mixed": lambda e0, e1: mixed.launch(stream, events=(e0, e1)),
            "split": launch_split,
            "ring": lambda e0, e1: ring.launch(stream, events=(e0, e1)),
            "mixed2": lambda e0, e1: mixed2.launch(stream, events=(e0, e1)),
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
        nb = mixed.bytes
        assert nb == B * n * S and uniform.bytes == nb
        flagged = [v for v, p in (("uniform", uniform), ("mixed", mixed)) if p.corrupt(stream)]
        print(json.dumps({
            "shape": spec, "layout": "planar", "bytes": nb, "patterns": ndistinct,
            "forms": {"uniform": uniform.forms(), "mixed": mixed.forms(), "split": split[0].forms(),
                      "ring": ring.forms(), "mixed2": mixed2.forms()},
            "us": {v: round(x * 1e3, 2) for v, x in med.items()},
            "us_rounds": {v: [round(y * 1e3, 2) for y in x] for v, x in ms.items()},
            "GBps": {v: round(nb / (x * 1e-3) / 1e9, 1) for v, x in med.items()},
            "mixed_over_uniform": round(med["mixed"] / med["uniform"], 4),
            "split_over_mixed": round(med["split"] / med["mixed"], 3),
            "ring_over_uniform": round(med["ring"] / med["uniform"], 4),
            "mixed_over_mixed2": round(med["mixed"] / med["mixed2"], 4),
            "plan_create_ms": {"uniform": round((t1 - t0) * 1e3, 2), "mixed": round((t2 - t1) * 1e3, 2),
                               "split": round((t3 - t2) * 1e3, 2)},
            "reps": a.reps, "rounds": a.rounds, "verify_flagged": flagged}), flush=True)
        for p in [uniform, mixed, ring, mixed2] + split:
            p.close()
        del sb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
