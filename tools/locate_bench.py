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
Pair plans (max_errors = 2), same batch, same process, same rounds:
  (b2) clean2  the pair plan on clean data;
  (c2) pair_valid   two of the k read shards of every stripe wholly corrupt (the same columns);
  (c3) pair_mixed   one read shard and one compared shard of every stripe wholly corrupt;
  (c4) single2      the pair plan over (c) valid's batch: every column has a single error.
Workloads: `rs10_4` RS(10,4), 256 stripes, sizes log-uniform in 64 KiB..4 MiB; `rs16_4`
RS(16,4), 4,096 stripes, sizes uniform in 1..16 KiB (the §5.9 workloads).
(a)-(c) are timed with rs_plan_launch_timed events over `--reps` launches, the median counts;
the variants are interleaved over `--rounds` rounds, (a), (b) and (b2) in rotating order. Which
of them runs first in a round (right after the previous round's SHA-256 pass) matters more
than which it is, so b/a, b2/a and b2/b are also reported per position: first against first
and so on (use a multiple of 3 rounds). (c2)-(c4) follow (c) in every round and are reported
against (c) valid of the same round, the median of the per-round ratios. Prints one JSON line
per workload: median microseconds, GB/s of algorithmic bytes, the ratios b/a, c/a and d/c, the
pair plan's ratios, and the counts checks of (c) and of (c2)-(c4).
Correct plans (`--correct` adds a second JSON line per workload, "section":
"correct"), same batch, same process:
  (e1) clean_correct   the correct plan on clean data, against (b) clean timed beside it: the
               two alternate, and are compared first against first and second against second;
  (e2) fix_valid       one of the k read shards of every stripe wholly corrupt, against (c) valid
               of the same round. A launch repairs the damage, so it is re-injected before
               every timed launch (the same XOR kernels that inject it for (c), then a
               synchronise); the time is the launch's own events', so the injection is not in
               it, but the launch finds the cache as the injection left it;
  (e3) fix_compared    the same with a compared shard, against (c) compared;
  (e4) heal_host / correct_host   rs_heal_batch against rs_correct_batch, wall clock, on
               `--host-stripes` host stripes of `--host-shard` bytes with one bad 4 KiB sector each
               (re-injected before every call; RS of the workload).
usage: python tools/locate_bench.py [--workload rs10_4] [--workload rs16_4] [--correct]
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


def correct_section(a, name, k, m, sizes, ptrs, flip, which, locate, stream):
    """(e1)-(e4) of the module docstring: one JSON line."""
    from callfs_amd import erasure
    n, B = k + m, len(sizes)
    correct = Plan.correct(k, m, sizes, ptrs)

    def launch(p):
        return lambda e0, e1: p.launch(stream, events=(e0, e1))

    def fix(v):
        def fn(e0, e1):
            flip(which[v])  # the launch before this one repaired it
            correct.launch(stream, events=(e0, e1))
        return fn

    def found(v):
        def fn(e0, e1):
            locate.launch(stream, events=(e0, e1))
        return fn

    w0 = time.perf_counter()
    while (time.perf_counter() - w0) * 1e3 < a.warm_ms:
        timed(launch(correct), 2)
    assert not correct.blame(stream).any() and not locate.blame(stream).any()
    ms = {v: [] for v in ("clean", "clean_correct", "valid", "fix_valid", "compared", "fix_compared")}
    pos = {"clean": ([], []), "clean_correct": ([], [])}
    counts_ok = True
    for r in range(a.rounds):
        order = ("clean", "clean_correct") if r % 2 == 0 else ("clean_correct", "clean")
        for at, v in enumerate(order):
            ms[v].append(timed(launch(locate if v == "clean" else correct), a.reps))
            pos[v][at].append(ms[v][-1])
        assert not correct.blame(stream).any() and not locate.blame(stream).any()
        for v in ("valid", "compared"):
            flip(which[v])
            timed(found(v), 2)
            ms[v].append(timed(found(v), a.reps))
            flip(which[v])
            locate.blame(stream)
            timed(fix(v), 2)
            correct.blame(stream)
            ms["fix_" + v].append(timed(fix(v), a.reps))
            got = correct.blame(stream)
            want = np.zeros_like(got)
            for b, i in enumerate(which[v]):
                want[b, i] = a.reps * sizes[b]
            counts_ok = counts_ok and bool(np.array_equal(got, want))
    assert not locate.blame(stream).any()  # every repair was exact: the batch is clean again
    med = {v: statistics.median(x) for v, x in ms.items()}

    def per_round(x, y):
        return round(statistics.median([p / q for p, q in zip(ms[x], ms[y])]), 4)

    by_pos = {nm: round(statistics.median(pos["clean_correct"][at]) / statistics.median(pos["clean"][at]), 4)
              if pos["clean_correct"][at] and pos["clean"][at] else None
              for at, nm in enumerate(("first", "second"))}
    # (e4) host stripes, one bad 4 KiB sector each
    S, HB = a.host_shard, a.host_stripes
    rng = np.random.default_rng(a.seed)
    host = []
    for _ in range(HB):
        st = [rng.integers(0, 256, S, dtype=np.uint8) for _ in range(k)] + [np.zeros(S, dtype=np.uint8) for _ in range(m)]
        erasure.encode_shards(st, k, m)
        host.append(st)
    sector = [(int(rng.integers(0, n)), 4096 * int(rng.integers(0, max(1, S // 4096)))) for _ in range(HB)]

    def hurt():
        for st, (i, o) in zip(host, sector):
            st[i][o:o + 4096] ^= 0x55

    wall = {"heal_host": [], "correct_host": []}
    host_ok = True
    for _ in range(a.host_reps + 1):  # the first pass warms both
        hurt()
        t0 = time.perf_counter()
        status, healed = erasure.heal_batch(host, k, m)
        wall["heal_host"].append((time.perf_counter() - t0) * 1e3)
        host_ok = host_ok and status == [0] * HB and healed == [[i] for i, _ in sector]
        hurt()
        t0 = time.perf_counter()
        counts, status = erasure.correct_batch(host, k, m)
        wall["correct_host"].append((time.perf_counter() - t0) * 1e3)
        host_ok = host_ok and status == [0] * HB and all(
            int(counts[b, i]) == min(4096, S - o) and int(counts[b].sum()) == int(counts[b, i])
            for b, (i, o) in enumerate(sector))
    hmed = {v: statistics.median(x[1:]) for v, x in wall.items()}
    print(json.dumps({
        "workload": name, "section": "correct", "k": k, "m": m, "stripes": B, "bytes": correct.bytes,
        "forms": {"locate": locate.forms(), "correct": correct.forms()},
        "us": {v: round(x * 1e3, 2) for v, x in med.items()},
        "us_rounds": {v: [round(y * 1e3, 2) for y in x] for v, x in ms.items()},
        "clean_correct_over_clean": round(med["clean_correct"] / med["clean"], 4),
        "clean_correct_over_clean_by_position": by_pos,
        "fix_valid_over_valid": per_round("fix_valid", "valid"),
        "fix_compared_over_compared": per_round("fix_compared", "compared"),
        "counts_exact": counts_ok,
        "host": {"stripes": HB, "shard_bytes": S, "sector": 4096,
                 "ms": {v: round(x, 2) for v, x in hmed.items()},
                 "ms_calls": {v: [round(y, 2) for y in x[1:]] for v, x in wall.items()},
                 "heal_over_correct": round(hmed["heal_host"] / hmed["correct_host"], 3), "exact": host_ok},
        "reps": a.reps, "rounds": a.rounds}), flush=True)
    correct.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", action="append", choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm-ms", type=float, default=150.0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--correct", action="store_true", help="also the correct plans' rows (e1)-(e4)")
    ap.add_argument("--host-stripes", type=int, default=16)
    ap.add_argument("--host-shard", type=int, default=1 << 20)
    ap.add_argument("--host-reps", type=int, default=5)
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
        locate2 = Plan.locate(k, m, sizes, ptrs, max_errors=2)
        hashes = HashPlan(ptrs, [S for S in sizes for _ in range(n)])
        digests = torch.empty(32 * B * n, dtype=torch.uint8, device=dev)
        rng = np.random.default_rng(a.seed)
        which = {"valid": [int(x) for x in rng.integers(0, k, B)],
                 "compared": [int(x) for x in rng.integers(k, n, B)]}
        # a second read shard, never the first one (k = 1 has none: its pair is read + compared)
        which["valid_b"] = [(i + 1 + int(x)) % k if k > 1 else k
                            for i, x in zip(which["valid"], rng.integers(0, max(k - 1, 1), B))]

        def flip(shards):
            for b, i in enumerate(shards):
                o = lead + offs[b][i]
                raw[o:o + sizes[b]] ^= 0x55
            torch.cuda.synchronize()

        def sha(e0, e1):
            e0.record(stream)
            hashes.launch(digests, stream)
            e1.record(stream)

        plans = {"verify": verify, "clean": locate, "valid": locate, "compared": locate,
                 "clean2": locate2, "pair_valid": locate2, "pair_mixed": locate2, "single2": locate2}
        fns = {v: (lambda e0, e1, p=p: p.launch(stream, events=(e0, e1))) for v, p in plans.items()}
        fns["sha256"] = sha
        for v in ("verify", "clean", "clean2", "sha256"):  # warm-up by time
            w0 = time.perf_counter()
            while (time.perf_counter() - w0) * 1e3 < a.warm_ms:
                timed(fns[v], 2)
        assert not locate.blame(stream).any() and not verify.corrupt(stream)
        assert not locate2.blame(stream).any()
        ms = {v: [] for v in fns}
        counts_ok = counts2_ok = True
        trio = ("verify", "clean", "clean2")
        pos = {v: {0: [], 1: [], 2: []} for v in trio}
        # what (c2)-(c4) corrupt, and on which plan's bins the columns land
        pairs = {"pair_valid": ("valid", "valid_b"), "pair_mixed": ("valid", "compared"),
                 "single2": ("valid",)}
        for r in range(a.rounds):
            for at, v in enumerate(trio[r % 3:] + trio[:r % 3]):
                ms[v].append(timed(fns[v], a.reps))
                pos[v][at].append(ms[v][-1])
            assert not locate.blame(stream).any() and not locate2.blame(stream).any()
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
            for v, sets in pairs.items():
                for w in sets:
                    flip(which[w])
                timed(fns[v], 2)
                locate2.blame(stream)
                ms[v].append(timed(fns[v], a.reps))
                got = locate2.blame(stream)
                want = np.zeros_like(got)
                for w in sets:
                    for b, i in enumerate(which[w]):
                        want[b, i] = a.reps * sizes[b]
                counts2_ok = counts2_ok and bool(np.array_equal(got, want))
                for w in sets:
                    flip(which[w])
            ms["sha256"].append(timed(fns["sha256"], a.reps))
        med = {v: statistics.median(x) for v, x in ms.items()}
        # round r runs verify, clean, clean2 rotated by r: each is first in every third round
        def by_position(x, y):
            return {name: round(statistics.median(pos[x][at]) / statistics.median(pos[y][at]), 4)
                    if pos[x][at] and pos[y][at] else None
                    for at, name in enumerate(("first", "second", "third"))}

        def per_round(x, y):
            return round(statistics.median([p / q for p, q in zip(ms[x], ms[y])]), 3)

        by_pos = by_position("clean", "verify")
        nb = {v: (verify.bytes if v == "verify" else n * total if v == "sha256" else plans[v].bytes) for v in fns}
        assert nb["verify"] == nb["clean"] == nb["clean2"] == n * total
        print(json.dumps({
            "workload": name, "k": k, "m": m, "stripes": B, "sizes": kind, "size_min": min(sizes),
            "size_max": max(sizes), "layout": "planar, 256-B aligned shards", "bytes": nb["clean"],
            "forms": {"verify": verify.forms(), "locate": locate.forms(), "locate2": locate2.forms()},
            "us": {v: round(x * 1e3, 2) for v, x in med.items()},
            "us_rounds": {v: [round(y * 1e3, 2) for y in x] for v, x in ms.items()},
            "GBps": {v: round(nb[v] / (x * 1e-3) / 1e9, 1) for v, x in med.items()},
            "clean_over_verify": round(med["clean"] / med["verify"], 4),
            "clean_over_verify_by_position": by_pos,
            "valid_over_verify": round(med["valid"] / med["verify"], 3),
            "compared_over_verify": round(med["compared"] / med["verify"], 3),
            "sha256_over_valid": round(med["sha256"] / med["valid"], 3),
            "sha256_over_compared": round(med["sha256"] / med["compared"], 3),
            "counts_exact": counts_ok,
            "clean2_over_verify": round(med["clean2"] / med["verify"], 4),
            "clean2_over_verify_by_position": by_position("clean2", "verify"),
            "clean2_over_clean_by_position": by_position("clean2", "clean"),
            "pair_valid_over_valid": per_round("pair_valid", "valid"),
            "pair_mixed_over_valid": per_round("pair_mixed", "valid"),
            "single2_over_valid": per_round("single2", "valid"),
            "pair_valid_over_verify": round(med["pair_valid"] / med["verify"], 3),
            "pair_mixed_over_verify": round(med["pair_mixed"] / med["verify"], 3),
            "pair_counts_exact": counts2_ok, "reps": a.reps, "rounds": a.rounds}), flush=True)
        if a.correct:
            correct_section(a, name, k, m, sizes, ptrs, flip, which, locate, stream)
        verify.close()
        locate.close()
        locate2.close()
        hashes.close()
        del raw, digests
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
