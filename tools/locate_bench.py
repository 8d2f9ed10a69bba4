"""Locate plans against what they replace, timed in one process.

Per workload, on a resident batch in the planar layout with 256-B aligned shards, every
stripe fully present and consistent:
  (a) verify   the equal-traffic reference: a required plan with nothing required over the
               same batch (every present shard beyond the first k compared, nothing written);
  (b) clean    the locate plan on clean data;
  (c) valid / compared   the locate plan with one shard of every stripe wholly corrupt, once
               one of the k read shards and once a compared one (every byte column of every
               stripe is classified);
  (d) sha256   what finding the shard costs without locate: rs_sha256_dev's kernel over all
               shards of the batch (a hash plan's launch between two stream events).
Workloads: `rs10_4` RS(10,4), 256 stripes, sizes log-uniform in 64 KiB..4 MiB; `rs16_4`
RS(16,4), 4,096 stripes, sizes uniform in 1..16 KiB (the §5.9 workloads).
(a)-(c) are timed with rs_plan_launch_timed events over `--reps` launches, the median counts;
the variants are interleaved over `--rounds` rounds, (a) and (b) in alternating order. Which
of the two runs first in a round (right after the previous round's SHA-256 pass) matters more
than which it is, so b/a is also reported per position: first against first, second against
second. Prints one JSON line per workload: median microseconds, GB/s of algorithmic bytes,
the ratios b/a, c/a and d/c, and the counts check of (c).
usage: python tools/locate_bench.py [--workload rs10_4] [--workload rs16_4]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from callfs_amd.device import HashPlan, Plan  # noqa: E402
from tools.mixed_bench import timed  # noqa: E402
from tools.ragged_bench import WORKLOADS, draw_sizes, planar_offsets  # noqa: E402


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
    for name in a.workload or sorted(WORKLOADS):
        k, m, B, kind, lo, hi = WORKLOADS[name]
        n = k + m
        sizes = draw_sizes(kind, lo, hi, B, a.seed)
        total = sum(sizes)
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
        every = [[True] * n] * B
        verify = Plan.ragged(k, m, sizes, ptrs, present=every, required=[[False] * n] * B)
        locate = Plan.locate(k, m, sizes, ptrs)
        hashes = HashPlan(ptrs, [S for S in sizes for _ in range(n)])
        digests = torch.empty(32 * B * n, dtype=torch.uint8, device=dev)
        rng = np.random.default_rng(a.seed)
        which = {"valid": [int(x) for x in rng.integers(0, k, B)],
                 "compared": [int(x) for x in rng.integers(k, n, B)]}

        def flip(shards):
            for b, i in enumerate(shards):
                o = lead + offs[b][i]
                raw[o:o + sizes[b]] ^= 0x55
            torch.cuda.synchronize()

        def sha(e0, e1):
            e0.record(stream)
            hashes.launch(digests, stream)
            e1.record(stream)

        plans = {"verify": verify, "clean": locate, "valid": locate, "compared": locate}
        fns = {v: (lambda e0, e1, p=p: p.launch(stream, events=(e0, e1))) for v, p in plans.items()}
        fns["sha256"] = sha
        for v in ("verify", "clean", "sha256"):  # warm-up by time
            w0 = time.perf_counter()
            while (time.perf_counter() - w0) * 1e3 < a.warm_ms:
                timed(fns[v], 2)
        assert not locate.blame(stream).any() and not verify.corrupt(stream)
        ms = {v: [] for v in fns}
        counts_ok = True
        for r in range(a.rounds):
            for v in (("verify", "clean") if r % 2 == 0 else ("clean", "verify")):
                ms[v].append(timed(fns[v], a.reps))
            assert not locate.blame(stream).any()
            for v in ("valid", "compared"):
                flip(which[v])
                timed(fns[v], 2)
                locate.blame(stream)
                ms[v].append(timed(fns[v], a.reps))
                got = locate.blame(stream)
                want = np.zeros_like(got)
                for b, i in enumerate(which[v]):
                    want[b, i] = a.reps * sizes[b]
                counts_ok = counts_ok and bool(np.array_equal(got, want))
                flip(which[v])
            ms["sha256"].append(timed(fns["sha256"], a.reps))
        med = {v: statistics.median(x) for v, x in ms.items()}
        # verify runs first in even rounds, clean in odd ones
        at = {"first": (ms["clean"][1::2], ms["verify"][0::2]), "second": (ms["clean"][0::2], ms["verify"][1::2])}
        by_pos = {pos: round(statistics.median(c) / statistics.median(v), 4) if c and v else None
                  for pos, (c, v) in at.items()}
        nb = {"verify": verify.bytes, "clean": locate.bytes, "valid": locate.bytes,
              "compared": locate.bytes, "sha256": n * total}
        assert nb["verify"] == nb["clean"] == n * total
        print(json.dumps({
            "workload": name, "k": k, "m": m, "stripes": B, "sizes": kind, "size_min": min(sizes),
            "size_max": max(sizes), "layout": "planar, 256-B aligned shards", "bytes": nb["clean"],
            "forms": {"verify": verify.forms(), "locate": locate.forms()},
            "us": {v: round(x * 1e3, 2) for v, x in med.items()},
            "us_rounds": {v: [round(y * 1e3, 2) for y in x] for v, x in ms.items()},
            "GBps": {v: round(nb[v] / (x * 1e-3) / 1e9, 1) for v, x in med.items()},
            "clean_over_verify": round(med["clean"] / med["verify"], 4),
            "clean_over_verify_by_position": by_pos,
            "valid_over_verify": round(med["valid"] / med["verify"], 3),
            "compared_over_verify": round(med["compared"] / med["verify"], 3),
            "sha256_over_valid": round(med["sha256"] / med["valid"], 3),
            "sha256_over_compared": round(med["sha256"] / med["compared"], 3),
            "counts_exact": counts_ok, "reps": a.reps, "rounds": a.rounds}), flush=True)
        verify.close()
        locate.close()
        hashes.close()
        del raw, digests
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
