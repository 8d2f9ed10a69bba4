"""The final decode-repair launch against the final decode-check launch of the same shape
(DESIGN.md §5.16), timed in one process.

§5.15's setup: a resident batch in the planar layout with 256-B aligned shards, a clean codeword
per stripe, the expected set {m..n-1}, `wanted` of the other shards wanted and the next three
compared. Every expected shard but one and the compared shards have been merged into the rows
before anything is timed, so what is timed is the launch after the last survivor lands:
  check1    the final decode-check merge launch of the last survivor (rs_check_ragged, unchanged);
  repair1   the decode-repair launch of the same shard over the same rows, on clean data: the
            clean path, which should cost what check1 costs;
  sector    repair1 on a batch in which one survivor of every stripe has one bad 4 KiB sector;
  whole     repair1 on a batch in which that survivor is wholly corrupt: every lane takes the slow
            path (no fix buffers: the columns are classified, counted and the wanted rows repaired).
Each variant is warmed up, then timed over `--reps` launches with rs_plan_launch_timed events; the
median counts. The variants are interleaved over `--rounds` rounds, the order rotated. Prints one
JSON line per shape: median microseconds per round and overall, repair1 / check1 matched by
position in the round, the spread between rounds, and the bytes a second download plus
rs_heal_batch would move for the damaged stripes ((k + 3) * S fetched again, then three passes).
usage: python tools/decode_repair_bench.py [--shape k,m,S,stripes,wanted ...]
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

SHAPES = ["10,4,1048576,256,1", "10,6,1048576,256,3"]
NCHK = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="k,m,S,stripes,wanted")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--warm-ms", type=float, default=150.0)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    for shape in a.shape or SHAPES:
        k, m, S, B, nw = (int(x) for x in shape.split(","))
        n = k + m
        assert nw + NCHK <= m
        pitch = (S + 255) // 256 * 256
        sizes = [S] * B
        rest, expect = list(range(m)), list(range(m, n))
        wanted, compared = rest[:nw], rest[nw:nw + NCHK]
        eflags = [[i in expect for i in range(n)]] * B
        acc = {j: n + q for q, j in enumerate(compared)}
        last, hurt = expect[0], expect[1]
        keep, plans = [], {}
        # one batch per kind of damage: the accumulators hold what the shards as delivered gave
        for kind in ("clean", "sector", "whole"):
            raw = torch.zeros(B * (n + NCHK) * pitch + 256, dtype=torch.uint8, device=dev)
            keep.append(raw)
            base = raw.data_ptr() + (-raw.data_ptr() % 256)
            off0 = base - raw.data_ptr()
            g = torch.Generator(device=dev)
            g.manual_seed(0xCA11F5)
            raw[:B * k * pitch + 256].random_(0, 256, generator=g)
            ptr = lambda b, i: base + (i * B + b) * pitch  # noqa: E731  planar; i >= n: an accumulator

            def ptrs(which):
                return [ptr(b, i) if i in which else 0 for b in range(B) for i in range(n)]

            enc = Plan.ragged(k, m, sizes, [ptr(b, i) for b in range(B) for i in range(n)])  # a codeword per stripe
            enc.launch()
            assert not enc.corrupt()
            enc.close()
            for b in range(B):
                at = off0 + (hurt * B + b) * pitch
                if kind == "sector":
                    raw[at + 8192:at + 8192 + min(4096, S - 8192)] ^= 0x5A
                elif kind == "whole":
                    raw[at:at + S] ^= 0x5A
            dst = ptrs(wanted)
            chk = [ptr(b, acc[i]) if i in compared else 0 for b in range(B) for i in range(n)]
            feed = Plan.decode_check(k, m, sizes, eflags, ptrs(expect[1:] + compared), dst, chk)
            feed.launch()
            feed.close()
            name = {"clean": "repair1", "sector": "sector", "whole": "whole"}[kind]
            plans[name] = Plan.decode_repair(k, m, sizes, eflags, ptrs([last]), dst, chk)
            if kind == "clean":
                plans["check1"] = Plan.decode_check(k, m, sizes, eflags, ptrs([last]), dst, chk, final=True)
        columns = {"check1": 0, "repair1": 0, "sector": B * min(4096, S - 8192), "whole": B * S}
        for v, p in plans.items():
            p.launch()
            assert p.corrupt() == (columns[v] != 0), v
            if v != "check1":
                c = p.blame()
                assert int(c[:, hurt].sum()) == columns[v] and int(c.sum()) == columns[v], (v, int(c.sum()))
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
        assert nb["repair1"] == nb["check1"] == B * S * (1 + 2 * nw + NCHK)
        ratio = [x / y for x, y in zip(ms["repair1"], ms["check1"])]
        print(json.dumps({
            "k": k, "m": m, "S": S, "stripes": B, "wanted": nw, "compared": NCHK,
            "layout": "planar, 256-B aligned shards", "bytes": nb,
            "forms": {v: p.forms() for v, p in plans.items()},
            "us": {v: round(x * 1e3, 2) for v, x in med.items()},
            "us_rounds": {v: [round(y * 1e3, 2) for y in x] for v, x in ms.items()},
            "spread_pct": {v: round(100 * (max(x) - min(x)) / statistics.median(x), 2) for v, x in ms.items()},
            "GBps": {v: round(nb[v] / (x * 1e-3) / 1e9, 1) for v, x in med.items()},
            "repair1_over_check1": round(statistics.median(ratio), 4),
            "repair1_over_check1_rounds": [round(x, 4) for x in ratio],
            "sector_over_check1": round(med["sector"] / med["check1"], 4),
            "whole_over_check1": round(med["whole"] / med["check1"], 4),
            "second_download_plus_heal_bytes": B * S * ((k + NCHK) + 3 * (k + NCHK + nw)),
            "reps": a.reps, "rounds": a.rounds}), flush=True)
        for p in plans.values():
            p.close()
        del keep, plans
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
