"""Decode-idx plans against the launches that move the same bytes, timed in one
process.

On a resident batch in the planar layout with 256-B aligned shards (every stripe's n shards, shard
region after shard region), RS(10,4) by default, with the expected set {4..13} and the wanted
shards {0,1,2,3}:
  (a) merge1   a decode-idx merge launch of one delivered shard (4) into the four wanted shards:
               (1 + 2*4) * S per stripe;
  (b) encidx1  the update plan in EncodeIdx mode with one shard (0) into the four parity shards:
               the same bytes, through rs_update_ragged;
  (a') merge1p the decode-idx merge launch over exactly (b)'s buffers (expect = the data shards,
               shard 0 delivered into the four parity shards): the two kernels on the same addresses;
  (c) store10  a decode-idx store launch of all ten expected shards: (10 + 4) * S per stripe;
  (d) recon    the required reconstruct plan of the same erasures (shards 0..3 missing and wanted,
               exactly k present, so nothing is compared): the same bytes.
Each variant is warmed up, then timed over `--reps` launches with rs_plan_launch_timed events (the
kernels' own time, first dispatch start to last dispatch end); the median counts. The variants are
interleaved over `--rounds` rounds. Prints one JSON line per shape: median microseconds per round
and overall, GB/s of algorithmic bytes, a/b, a'/b and c/d, and the spread between rounds.
usage: python tools/decode_idx_bench.py [--shape k,m,S,stripes ...]
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

SHAPES = ["10,4,1048576,256"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="k,m,S,stripes (default: RS(10,4), 256 x 1 MiB)")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm-ms", type=float, default=150.0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for shape in a.shape or SHAPES:
        k, m, S, B = (int(x) for x in shape.split(","))
        n = k + m
        pitch = (S + 255) // 256 * 256
        raw = torch.empty(B * n * pitch + 256, dtype=torch.uint8, device=dev)
        g = torch.Generator(device=dev)
        g.manual_seed(0xCA11F5)
        raw.random_(0, 256, generator=g)
        base = raw.data_ptr() + (-raw.data_ptr() % 256)
        ptr = lambda b, i: base + (i * B + b) * pitch  # noqa: E731  planar: shard i of every stripe together
        sizes = [S] * B
        missing = list(range(m))            # the wanted shards: the first m data shards
        expect = list(range(m, n))          # the k expected: the other data shards and the parity
        eflags = [[i in expect for i in range(n)]] * B
        dst = [ptr(b, i) if i in missing else 0 for b in range(B) for i in range(n)]
        one = [ptr(b, i) if i == expect[0] else 0 for b in range(B) for i in range(n)]
        every = [ptr(b, i) if i in expect else 0 for b in range(B) for i in range(n)]
        t0 = time.perf_counter()
        merge1 = Plan.decode_idx(k, m, sizes, eflags, one, dst)
        t1 = time.perf_counter()
        store10 = Plan.decode_idx(k, m, sizes, eflags, every, dst, store=True)
        encidx1 = Plan.update(k, m, sizes, [[i == 0 for i in range(k)]] * B, None,
                              [ptr(b, i) if i == 0 else 0 for b in range(B) for i in range(k)],
                              [ptr(b, k + j) for b in range(B) for j in range(m)])
        recon = Plan.ragged(k, m, sizes, [ptr(b, i) for b in range(B) for i in range(n)],
                            present=[[i in expect for i in range(n)]] * B,
                            required=[[i in missing for i in range(n)]] * B)
        merge1p = Plan.decode_idx(k, m, sizes, [[i < k for i in range(n)]] * B,
                                  [ptr(b, i) if i == 0 else 0 for b in range(B) for i in range(n)],
                                  [ptr(b, i) if i >= k else 0 for b in range(B) for i in range(n)])
        plans = {"merge1": merge1, "encidx1": encidx1, "merge1p": merge1p, "store10": store10, "recon": recon}
        variants = {v: (lambda e0, e1, p=p: p.launch(stream, events=(e0, e1))) for v, p in plans.items()}
        for fn in variants.values():  # warm-up by time
            w0 = time.perf_counter()
            while (time.perf_counter() - w0) * 1e3 < a.warm_ms:
                timed(fn, 2)
        ms = {v: [] for v in variants}
        names = list(variants)
        for r in range(a.rounds):
            rot = r % len(names)
            for v in names[rot:] + names[:rot]:
                ms[v].append(timed(variants[v], a.reps))
        med = {v: statistics.median(x) for v, x in ms.items()}
        nb = {v: p.bytes for v, p in plans.items()}
        c = len(missing)
        assert nb["merge1"] == nb["encidx1"] == nb["merge1p"] == B * S * (1 + 2 * c)
        assert nb["store10"] == nb["recon"] == B * S * (k + c)
        print(json.dumps({
            "k": k, "m": m, "S": S, "stripes": B, "layout": "planar, 256-B aligned shards", "bytes": nb,
            "forms": {v: p.forms() for v, p in plans.items()},
            "us": {v: round(x * 1e3, 2) for v, x in med.items()},
            "us_rounds": {v: [round(y * 1e3, 2) for y in x] for v, x in ms.items()},
            "spread_pct": {v: round(100 * (max(x) - min(x)) / statistics.median(x), 2) for v, x in ms.items()},
            "GBps": {v: round(nb[v] / (x * 1e-3) / 1e9, 1) for v, x in med.items()},
            "merge1_over_encidx1": round(med["merge1"] / med["encidx1"], 4),
            "merge1_over_encidx1_rounds": [round(x / y, 4) for x, y in zip(ms["merge1"], ms["encidx1"])],
            "merge1p_over_encidx1": round(med["merge1p"] / med["encidx1"], 4),
            "merge1p_over_encidx1_rounds": [round(x / y, 4) for x, y in zip(ms["merge1p"], ms["encidx1"])],
            "store10_over_recon": round(med["store10"] / med["recon"], 4),
            "store10_over_recon_rounds": [round(x / y, 4) for x, y in zip(ms["store10"], ms["recon"])],
            "plan_create_ms": {"merge1": round((t1 - t0) * 1e3, 2)},
            "reps": a.reps, "rounds": a.rounds}), flush=True)
        for p in plans.values():
            p.close()
        del raw
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
