"""Feed launches and decode sessions against what they replace, timed in one
process, RS(10,4) with the expected set {4..13}.

  (a) feed     rs_feed_launch of one expected shard into 4 resident rows (4 wanted), merge mode,
      plan     against the decode-idx plan launch (rs_plan_create_decode_idx, one shard delivered)
               over the same buffers: (1 + 2*4) * S bytes each. Both are timed the same way: two
               events around `--reps` back-to-back launches on one stream, divided by reps.
  (b) inplace  rs_session_feed of one arrival (1 wanted + 3 compared rows) on the in-place route,
      staged   on the staged route (CALLFS_RS_SESSION_INPLACE_MAX forces either),
      hostcall against rs_decode_check for the same arrival: the delivered shard and the four rows
               in host memory, merge mode. Wall time per arrival; a session's feeds are timed over
               a whole session (13 arrivals, the stream drained at the end) and divided.
  (c) last     the last arrival's feed plus rs_session_finish, wall time until the wanted shard is
               in host memory, on either route,
      oneshot  against one rs_codec_decode of the same shards (one data shard missing).
Variants are interleaved over `--rounds` rounds; the median of the rounds counts and the spread
between rounds is printed. One JSON line per section and size.
usage: python tools/session_bench.py [--sizes 65536,1048576,...] [--section a|b|c ...]
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

from callfs_amd import _native as N  # noqa: E402
from callfs_amd import erasure as E  # noqa: E402
from callfs_amd.device import Feed, Plan  # noqa: E402

K, M, NN = 10, 4, 14
EXPECT = list(range(4, 14))


def rounds_of(variants, rounds):
    """{name: [seconds per round]} with the variants rotated from round to round."""
    out = {v: [] for v in variants}
    names = list(variants)
    for r in range(rounds):
        rot = r % len(names)
        for v in names[rot:] + names[:rot]:
            out[v].append(variants[v]())
    return out


def report(section, S, t, extra=None):
    med = {v: statistics.median(x) for v, x in t.items()}
    line = {"section": section, "S": S,
            "us": {v: round(x * 1e6, 2) for v, x in med.items()},
            "us_rounds": {v: [round(y * 1e6, 2) for y in x] for v, x in t.items()},
            "spread_pct": {v: round(100 * (max(x) - min(x)) / statistics.median(x), 1) for v, x in t.items()}}
    line.update(extra or {})
    print(json.dumps(line), flush=True)


def section_a(S, reps, rounds):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    pitch = (S + 255) // 256 * 256
    raw = torch.randint(0, 256, (5 * pitch + 256,), dtype=torch.uint8, device=dev)
    base = raw.data_ptr() + (-raw.data_ptr() % 256)
    src, rows = base, [base + (1 + r) * pitch for r in range(4)]
    eflags = [i in EXPECT for i in range(NN)]
    dst = [rows[i] if i < 4 else 0 for i in range(NN)]
    feed = Feed(K, M, S, eflags, dst, [0] * NN)
    plan = Plan.decode_idx(K, M, [S], [eflags], [src if i == EXPECT[0] else 0 for i in range(NN)], dst)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        def run():
            for _ in range(10):
                fn()
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps
        return run

    t = rounds_of({"feed": timed(lambda: feed.launch(EXPECT[0], src, stream=stream)),
                   "plan": timed(lambda: plan.launch(stream))}, rounds)
    med = {v: statistics.median(x) for v, x in t.items()}
    report("a", S, t, {"bytes": 9 * S, "GBps": {v: round(9 * S / x / 1e9, 1) for v, x in med.items()},
                       "feed_over_plan": round(med["feed"] / med["plan"], 4),
                       "feed_over_plan_rounds": [round(x / y, 4) for x, y in zip(t["feed"], t["plan"])],
                       "reps": reps, "rounds": rounds})
    feed.close()
    plan.close()


def _codeword(S):
    rng = np.random.default_rng(S)
    data = rng.integers(0, 256, K * S, dtype=np.uint8).tobytes()
    return data, [bytes(s) for s in E.Codec().encode(data, E.ErasureProfile(K, M))]


def _session(S, route):
    os.environ["CALLFS_RS_SESSION_INPLACE_MAX"] = str(1 << 40) if route == "inplace" else "0"
    flags = lambda idx: [i in idx for i in range(NN)]  # noqa: E731
    return E.DecodeSession(K, M, S, flags(EXPECT), flags([0]), flags([1, 2, 3]))


def section_b(S, reps, rounds):
    _, shards = _codeword(S)
    order = EXPECT + [1, 2, 3]

    def session(route):
        def run():
            total = 0.0
            for _ in range(reps):
                s = _session(S, route)
                t0 = time.perf_counter()
                for i in order:
                    s.feed(i, shards[i])
                s.peek(0, 0)  # drains the stream
                total += time.perf_counter() - t0
                s.close()
            return total / (reps * len(order))
        return run

    dst = [bytearray(S) if i == 0 else None for i in range(NN)]
    chk = [bytearray(S) if i in (1, 2, 3) else None for i in range(NN)]
    eflags = [i in EXPECT for i in range(NN)]

    def hostcall():
        total = 0.0
        for r in range(reps * 2):
            i = order[r % len(order)]
            inputs = [shards[j] if j == i else None for j in range(NN)]
            t0 = time.perf_counter()
            E.decode_check(dst, chk, eflags, inputs, K, M)
            total += time.perf_counter() - t0
        return total / (reps * 2)

    for fn in (session("inplace"), session("staged"), hostcall):
        fn()
    t = rounds_of({"inplace": session("inplace"), "staged": session("staged"), "hostcall": hostcall}, rounds)
    med = {v: statistics.median(x) for v, x in t.items()}
    report("b", S, t, {"inplace_over_staged": round(med["inplace"] / med["staged"], 4),
                       "hostcall_over_best": round(med["hostcall"] / min(med["inplace"], med["staged"]), 2),
                       "reps": reps, "rounds": rounds})


def section_c(S, reps, rounds):
    data, shards = _codeword(S)
    order = EXPECT + [1, 2, 3]
    codec, prof = E.Codec(), E.ErasureProfile(K, M)

    def last(route):
        def run():
            total = 0.0
            for _ in range(reps):
                s = _session(S, route)
                for i in order[:-1]:
                    s.feed(i, shards[i])
                s.peek(0, 0)
                out = [bytearray(S) if i == 0 else None for i in range(NN)]
                t0 = time.perf_counter()
                s.feed(order[-1], shards[order[-1]])
                s.finish(out)
                total += time.perf_counter() - t0
                assert bytes(out[0]) == shards[0]
                s.close()
            return total / reps
        return run

    def oneshot():
        total = 0.0
        for _ in range(reps):
            have = [None] + list(shards[1:])
            t0 = time.perf_counter()
            got = codec.decode(have, prof, K * S)
            total += time.perf_counter() - t0
            assert bytes(got[:S]) == shards[0]
        return total / reps

    for fn in (last("inplace"), last("staged"), oneshot):
        fn()
    t = rounds_of({"last_inplace": last("inplace"), "last_staged": last("staged"), "oneshot": oneshot}, rounds)
    report("c", S, t, {"reps": reps, "rounds": rounds})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=None, help="comma-separated shard sizes (default: per section)")
    ap.add_argument("--section", action="append", choices=("a", "b", "c"))
    ap.add_argument("--reps", type=int, default=200, help="launches per round in (a); (b), (c): reps / 10 sessions")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")] if a.sizes else None
    N.default_context()
    for sec in a.section or ("a", "b", "c"):
        if sec == "a":
            for S in sizes or (64 << 10, 1 << 20, 4 << 20):
                section_a(S, a.reps, a.rounds)
        elif sec == "b":
            for S in sizes or (4 << 10, 64 << 10, 256 << 10, 1 << 20, 4 << 20):
                section_b(S, max(2, a.reps // 10), a.rounds)
        else:
            for S in sizes or (64 << 10, 1 << 20, 4 << 20):
                section_c(S, max(2, a.reps // 10), a.rounds)


if __name__ == "__main__":
    main()
