"""Update plans against the full encode they replace, timed in one process.

Per shape, on resident batches in the planar layout with 256-B aligned shards (the old data
shards of every stripe in one region, the new bytes of the changed shards in another, the
parity shards in a third), c changed shards per stripe (stripe b changes shards b, b+1, ..
b+c-1 mod k, so the batch holds k changed sets):
  (a) update  one update plan (rs_plan_create_update): reads old and new of the c changed
              shards and the m parity shards, writes the parity: (2c + 2m) * S per stripe;
  (b) encode  the full-encode plan of the same batch over the new data (the unchanged shards'
              old buffers, the changed shards' new ones), which is what a caller had before
              update plans: (k + m) * S per stripe.
Each variant is warmed up, then timed over `--reps` launches with rs_plan_launch_timed events
(the kernels' own time, first dispatch start to last dispatch end); the median counts. The
variants are interleaved over `--rounds` rounds. Prints one JSON line per (shape, c): median
microseconds, GB/s of algorithmic bytes, a/b beside the byte ratio.
usage: python tools/update_bench.py [--shape k,m,S,stripes ...] [--changed 1 --changed half]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import torch  # noqa: E402

from callfs_amd.device import Plan  # noqa: E402
from tools.mixed_bench import timed  # noqa: E402

SHAPES = ["10,4,1048576,256", "32,4,1048576,256"]


def region(at, count, S):
    """`count` S-byte buffers from offset `at`, each at the next 256-B boundary."""
    offs = []
    for _ in range(count):
        at = (at + 255) // 256 * 256
        offs.append(at)
        at += S
    return offs, at


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="k,m,S,stripes (default: RS(10,4) and RS(32,4), 256 x 1 MiB)")
    ap.add_argument("--changed", action="append", help="changed shards per stripe: a number or 'half' (default: 1, half)")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm-ms", type=float, default=150.0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for shape in a.shape or SHAPES:
        k, m, S, B = (int(x) for x in shape.split(","))
        for cs in a.changed or ["1", "half"]:
            c = max(1, k // 2) if cs == "half" else int(cs)
            old_off, at = region(0, B * k, S)
            new_off, at = region(at, B * c, S)
            par_off, at = region(at, B * m, S)
            raw = torch.empty(at + 256, dtype=torch.uint8, device=dev)
            g = torch.Generator(device=dev)
            g.manual_seed(0xCA11F5)
            raw.random_(0, 256, generator=g)
            base = raw.data_ptr() + (-raw.data_ptr() % 256)
            sets = [[(b + j) % k for j in range(c)] for b in range(B)]
            flags = [[i in set(s) for i in range(k)] for s in sets]
            old = [base + old_off[b * k + i] if flags[b][i] else 0 for b in range(B) for i in range(k)]
            new = [0] * (B * k)
            for b in range(B):
                for j, i in enumerate(sets[b]):
                    new[b * k + i] = base + new_off[b * c + j]
            par = [base + o for o in par_off]
            t0 = time.perf_counter()
            upd = Plan.update(k, m, [S] * B, flags, old, new, par)
            t1 = time.perf_counter()
            # the full encode of the new data
            shards = []
            for b in range(B):
                shards += [new[b * k + i] or base + old_off[b * k + i] for i in range(k)]
                shards += par[b * m:(b + 1) * m]
            enc = Plan(k, m, S, B, shards)
            t2 = time.perf_counter()
            variants = {
                "update": lambda e0, e1: upd.launch(stream, events=(e0, e1)),
                "encode": lambda e0, e1: enc.launch(stream, events=(e0, e1)),
            }
            for fn in variants.values():  # warm-up by time
                w0 = time.perf_counter()
                while (time.perf_counter() - w0) * 1e3 < a.warm_ms:
                    timed(fn, 2)
            ms = {v: [] for v in variants}
            names = list(variants)
            for r in range(a.rounds):
                for v in names[r % 2:] + names[:r % 2]:
                    ms[v].append(timed(variants[v], a.reps))
            med = {v: statistics.median(x) for v, x in ms.items()}
            nb = {"update": upd.bytes, "encode": enc.bytes}
            assert nb["update"] == B * S * (2 * c + 2 * m) and nb["encode"] == B * S * (k + m)
            print(json.dumps({
                "k": k, "m": m, "S": S, "stripes": B, "changed": c, "patterns": len({tuple(sorted(s)) for s in sets}),
                "layout": "planar, 256-B aligned shards", "bytes": nb,
                "forms": {"update": upd.forms(), "encode": enc.forms()},
                "us": {v: round(x * 1e3, 2) for v, x in med.items()},
                "us_rounds": {v: [round(y * 1e3, 2) for y in x] for v, x in ms.items()},
                "GBps": {v: round(nb[v] / (x * 1e-3) / 1e9, 1) for v, x in med.items()},
                "update_over_encode": round(med["update"] / med["encode"], 4),
                "byte_ratio": round(nb["update"] / nb["encode"], 4),
                "plan_create_ms": {"update": round((t1 - t0) * 1e3, 2), "encode": round((t2 - t1) * 1e3, 2)},
                "reps": a.reps, "rounds": a.rounds}), flush=True)
            upd.close()
            enc.close()
            del raw
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
