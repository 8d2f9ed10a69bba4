"""Absorb launches and encode sessions against what they replace, timed in one
process, RS(10,4).

  (a) absorb   rs_absorb_launch of one piece that covers q = 1, 4, 10 whole shards of S bytes into
               the 4 resident rows: q * S bytes read, 4 * S read and written. Timed as two events
               around `--reps` back-to-back launches on one stream, divided by reps.
      plan     for q = k, the uniform encode plan launch over the same k * S input bytes (it reads
               k * S and writes 4 * S; it does not read the rows).
               The buffers are (q + 4) * S to (k + 4) * S bytes and are launched over again and
               again: up to S = 1 MiB they fit the 256 MiB last-level cache, so the figures are
               cache-resident ones (stated in the line as "resident").
  (b) inplace  rs_encode_session_feed per piece of `piece` bytes on the in-place route,
      direct   on the direct route (the body inside an rs_host_alloc buffer),
      staged   on the staged route (CALLFS_RS_SESSION_INPLACE_MAX forces it),
      idx      against rs_encode_idx for the same bytes at S = 1 MiB (one call per whole shard,
               parity in host memory). Sessions are timed over a whole body of 10 MiB, the stream
               drained at the end; the figure is bytes fed per second.
  (c) last     from the last body byte to the parity in host memory: the last feed (one piece of
               min(L, 1 MiB)) plus rs_encode_session_finish, on the in-place and the staged route,
      oneshot  against one rs_codec_encode of the whole body.
Variants are interleaved over `--rounds` rounds; the median of the rounds counts and the spread
between rounds is printed. One JSON line per section and size.
usage: python tools/encode_session_bench.py [--section a|b|c ...] [--reps N] [--rounds N]
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
from callfs_amd import erasure as E  # noqa: E402
from callfs_amd.device import Absorb, Plan  # noqa: E402

K, M = 10, 4


def rounds_of(variants, rounds):
    """{name: [seconds per round]} with the variants rotated from round to round."""
    out = {v: [] for v in variants}
    names = list(variants)
    for r in range(rounds):
        rot = r % len(names)
        for v in names[rot:] + names[:rot]:
            out[v].append(variants[v]())
    return out


def report(section, key, t, extra=None):
    med = {v: statistics.median(x) for v, x in t.items()}
    line = {"section": section}
    line.update(key)
    line.update({"us": {v: round(x * 1e6, 2) for v, x in med.items()},
                 "us_rounds": {v: [round(y * 1e6, 2) for y in x] for v, x in t.items()},
                 "spread_pct": {v: round(100 * (max(x) - min(x)) / statistics.median(x), 1) for v, x in t.items()}})
    line.update(extra or {})
    print(json.dumps(line), flush=True)


def section_a(S, reps, rounds):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    pitch = (S + 255) // 256 * 256
    raw = torch.randint(0, 256, ((K + M) * pitch + 256,), dtype=torch.uint8, device=dev)
    base = raw.data_ptr() + (-raw.data_ptr() % 256)
    rows = [base + (K + j) * pitch for j in range(M)]
    # the absorb source is the body, shards back to back at pitch S; the plan reads the same bytes
    body = torch.randint(0, 256, (K * S,), dtype=torch.uint8, device=dev)
    absorb = Absorb(K, M, S, rows)
    plan = Plan(K, M, S, 1, [body.data_ptr() + i * S for i in range(K)] + rows)
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

    variants = {"absorb_q%d" % q: timed(lambda q=q: absorb.launch(0, q * S, body.data_ptr(), stream=stream))
                for q in (1, 4, 10)}
    variants["plan"] = timed(lambda: plan.launch(stream))
    t = rounds_of(variants, rounds)
    med = {v: statistics.median(x) for v, x in t.items()}
    moved = {"absorb_q1": (1 + 2 * M) * S, "absorb_q4": (4 + 2 * M) * S, "absorb_q10": (K + 2 * M) * S,
             "plan": (K + M) * S}
    report("a", {"S": S}, t, {"bytes": moved, "GBps": {v: round(moved[v] / x / 1e9, 1) for v, x in med.items()},
                              "absorb_q10_over_plan": round(med["absorb_q10"] / med["plan"], 4),
                              "absorb_q10_over_plan_rounds": [round(x / y, 4) for x, y in
                                                              zip(t["absorb_q10"], t["plan"])],
                              "resident": (K + M) * S <= (256 << 20), "reps": reps, "rounds": rounds})
    absorb.close()
    plan.close()


def _route_env(route):
    os.environ["CALLFS_RS_SESSION_INPLACE_MAX"] = "0" if route == "staged" else str(1 << 40)


def section_b(piece, reps, rounds):
    S = 1 << 20
    L = K * S
    ctx = N.default_context()
    plain = np.random.default_rng(piece).integers(0, 256, L, dtype=np.uint8)
    pinned = N.PinnedBuffer(L, ctx)
    pinned.array[:] = plain

    def session(route):
        body = pinned.array if route == "direct" else plain

        def run():
            total = 0.0
            for _ in range(reps):
                _route_env(route)
                s = E.EncodeSession(K, M, L)
                t0 = time.perf_counter()
                for at in range(0, L, piece):
                    s.feed(at, body[at:at + piece])
                s.peek(0, 0)  # drains the stream
                total += time.perf_counter() - t0
                s.close()
            return total / reps
        return run

    parity = [bytearray(S) for _ in range(M)]

    def idx():
        total = 0.0
        for _ in range(reps):
            t0 = time.perf_counter()
            for i in range(K):
                E.encode_idx(plain[i * S:(i + 1) * S], i, parity, K, M)
            total += time.perf_counter() - t0
        return total / reps

    variants = {"inplace": session("inplace"), "direct": session("direct"), "staged": session("staged"), "idx": idx}
    for fn in variants.values():
        fn()
    t = rounds_of(variants, rounds)
    med = {v: statistics.median(x) for v, x in t.items()}
    report("b", {"piece": piece, "L": L}, t,
           {"GBps_fed": {v: round(L / x / 1e9, 2) for v, x in med.items()},
            "us_per_piece": {v: round(x * 1e6 / (L // piece), 2) for v, x in med.items() if v != "idx"},
            "idx_over_best": round(med["idx"] / min(med["inplace"], med["direct"], med["staged"]), 2),
            "reps": reps, "rounds": rounds})
    pinned.close()


def section_c(L, reps, rounds):
    ctx = N.default_context()
    body = np.random.default_rng(L).integers(0, 256, L, dtype=np.uint8)
    S = -(-L // K)
    last = min(L, 1 << 20)
    out = np.zeros((K + M) * S, dtype=np.uint8)
    ss = ctypes.c_size_t(0)

    def oneshot():
        total = 0.0
        for _ in range(reps):
            t0 = time.perf_counter()
            N.check(N.lib.rs_codec_encode(ctx.handle, K, M, ctypes.c_void_p(body.ctypes.data), L,
                                          ctypes.c_void_p(out.ctypes.data), out.size, ctypes.byref(ss)))
            total += time.perf_counter() - t0
        return total / reps

    oneshot()
    ref = out.reshape(K + M, S)[K:].copy()

    def close(route):
        def run():
            total = 0.0
            for _ in range(reps):
                _route_env(route)
                s = E.EncodeSession(K, M, L)
                for at in range(0, L - last, 1 << 20):
                    s.feed(at, body[at:min(at + (1 << 20), L - last)])
                s.peek(0, 0)
                parity = [bytearray(S) for _ in range(M)]
                t0 = time.perf_counter()
                s.feed(L - last, body[L - last:])
                s.finish(parity)
                total += time.perf_counter() - t0
                assert bytes(parity[M - 1]) == ref[M - 1].tobytes()
                s.close()
            return total / reps
        return run

    variants = {"last_inplace": close("inplace"), "last_staged": close("staged"), "oneshot": oneshot}
    for fn in variants.values():
        fn()
    t = rounds_of(variants, rounds)
    med = {v: statistics.median(x) for v, x in t.items()}
    report("c", {"L": L}, t, {"oneshot_over_best": round(med["oneshot"] / min(med["last_inplace"], med["last_staged"]), 2),
                              "reps": reps, "rounds": rounds})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", action="append", choices=("a", "b", "c"))
    ap.add_argument("--reps", type=int, default=200, help="launches per round in (a); (b), (c): reps / 20 bodies")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    N.default_context()
    for sec in a.section or ("a", "b", "c"):
        if sec == "a":
            for S in (16 << 10, 256 << 10, 1 << 20):
                section_a(S, a.reps, a.rounds)
        elif sec == "b":
            for piece in (64 << 10, 1 << 20):
                section_b(piece, max(2, a.reps // 20), a.rounds)
        else:
            for L in (640 << 10, 10 << 20, 40 << 20):
                section_c(L, max(2, a.reps // 20), a.rounds)


if __name__ == "__main__":
    main()
