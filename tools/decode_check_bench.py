"""The final decode-check launch against what the decode-idx plans offer for the same result
(DESIGN.md §5.15), timed in one process.

On a resident batch in the planar layout with 256-B aligned shards (§5.14's setup: every stripe's n
shards, shard region after shard region, and behind them the accumulators' regions), a clean
codeword per stripe, the expected set {m..n-1}, `wanted` of the other shards wanted and the next two
compared. Every expected shard but one and both compared shards have been merged into the rows
before anything is timed, so what is timed is the launch on the critical path after the last
survivor lands:
  check1   the final merge launch of the last survivor: one delivered shard, the wanted rows merged,
           the two check rows read, tested and not written: (1 + 2 * wanted + 2) * S per stripe;
  merge1   launch (a) of §5.14's table: the decode-idx merge launch of the same shard into the same
           wanted rows, (1 + 2 * wanted) * S per stripe;
  compare  the compare-only ragged plan over the ten expected and the two compared shards (present
           = expected and compared, nothing required): (k + 2) * S per stripe, with all k expected
           shards resident.
merge1 followed by compare is what a caller without decode-check plans runs for the same flag. Each
variant is warmed up, then timed over `--reps` launches with rs_plan_launch_timed events (the
kernels' own time); the median counts. The variants are interleaved over `--rounds` rounds, the
order rotated. No launch may flag a stripe (the batch is clean), which is checked before and after.
Prints one JSON line per shape: median microseconds per round and overall, GB/s of algorithmic
bytes, check1 / (merge1 + compare) and the spread between rounds.
usage: python tools/decode_check_bench.py [--shape k,m,S,stripes,wanted ...]
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

# RS(10,4) has four shards beside the expected ten: two wanted and two compared on §5.14's buffers;
# RS(10,6) holds the four wanted and two compared rows of a download that fetched two spares
SHAPES = ["10,4,1048576,256,2", "10,6,1048576,256,4"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="k,m,S,stripes,wanted")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm-ms", type=float, default=150.0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for shape in a.shape or SHAPES:
        k, m, S, B, nw = (int(x) for x in shape.split(","))
        n = k + m
        assert nw + 2 <= m
        pitch = (S + 255) // 256 * 256
        raw = torch.zeros(B * (n + 2) * pitch + 256, dtype=torch.uint8, device=dev)
        base = raw.data_ptr() + (-raw.data_ptr() % 256)
        g = torch.Generator(device=dev)
        g.manual_seed(0xCA11F5)
        raw[:B * k * pitch + 256].random_(0, 256, generator=g)
        ptr = lambda b, i: base + (i * B + b) * pitch  # noqa: E731  planar; i >= n: an accumulator
        sizes = [S] * B
        every = [ptr(b, i) for b in range(B) for i in range(n)]
        enc = Plan.ragged(k, m, sizes, every)  # a codeword per stripe
        enc.launch()
        assert not enc.corrupt()
        enc.close()
        rest = list(range(m))
        expect = list(range(m, n))
        wanted, compared = rest[:nw], rest[nw:nw + 2]
        eflags = [[i in expect for i in range(n)]] * B
        acc = {j: n + q for q, j in enumerate(compared)}

        def ptrs(which):
            return [ptr(b, i) if i in which else 0 for b in range(B) for i in range(n)]

        dst = ptrs(wanted)
        chk = [ptr(b, acc[i]) if i in compared else 0 for b in range(B) for i in range(n)]
        last = expect[0]
        # everything but the last survivor, merged from zeroed accumulators (the wanted rows hold
        # junk: the timed merges are not idempotent either way)
        feed = Plan.decode_check(k, m, sizes, eflags, ptrs(expect[1:] + compared), dst, chk)
        feed.launch()
        feed.close()
        t0 = time.perf_counter()
        check1 = Plan.decode_check(k, m, sizes, eflags, ptrs([last]), dst, chk, final=True)
        t1 = time.perf_counter()
        merge1 = Plan.decode_idx(k, m, sizes, eflags, ptrs([last]), dst)
        compare = Plan.ragged(k, m, sizes, [ptr(b, i) if i in expect or i in compared else 0
                                            for b in range(B) for i in range(n)],
                              present=[[i in expect or i in compared for i in range(n)]] * B,
                              required=[[False] * n] * B)
        plans = {"check1": check1, "merge1": merge1, "compare": compare}
        for p in (check1, compare):
            p.launch()
            assert not p.corrupt(), "the batch is a clean codeword"
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
        assert not check1.corrupt() and not compare.corrupt()
        med = {v: statistics.median(x) for v, x in ms.items()}
        nb = {v: p.bytes for v, p in plans.items()}
        assert nb["check1"] == B * S * (1 + 2 * nw + 2) and nb["merge1"] == B * S * (1 + 2 * nw)
        both = [x + y for x, y in zip(ms["merge1"], ms["compare"])]
        print(json.dumps({
            "k": k, "m": m, "S": S, "stripes": B, "wanted": nw, "compared": 2,
            "layout": "planar, 256-B aligned shards", "bytes": nb,
            "forms": {v: p.forms() for v, p in plans.items()},
            "us": {v: round(x * 1e3, 2) for v, x in med.items()},
            "us_rounds": {v: [round(y * 1e3, 2) for y in x] for v, x in ms.items()},
            "spread_pct": {v: round(100 * (max(x) - min(x)) / statistics.median(x), 2) for v, x in ms.items()},
            "GBps": {v: round(nb[v] / (x * 1e-3) / 1e9, 1) for v, x in med.items()},
            "merge1_plus_compare_us": round(statistics.median(both) * 1e3, 2),
            "check1_over_merge1_plus_compare": round(med["check1"] / statistics.median(both), 4),
            "check1_over_merge1_plus_compare_rounds": [round(x / y, 4) for x, y in zip(ms["check1"], both)],
            "check1_over_merge1": round(med["check1"] / med["merge1"], 4),
            "plan_create_ms": {"check1": round((t1 - t0) * 1e3, 2)},
            "reps": a.reps, "rounds": a.rounds}), flush=True)
        for p in plans.values():
            p.close()
        del raw
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
