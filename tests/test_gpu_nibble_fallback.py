"""The ahead-of-time nibble-table kernels on the launches the bit-sliced rule
(csrc/bitslice_rule.hpp) has taken over: with CALLFS_RS_BITSLICE=0, which is also what a box
where hiprtc cannot build runs, and what every host-memory call runs until a background compile
lands. Every case is bit-exact against the C oracle (oracle/rs_oracle.c via oracle.cref):

  wide-ring        rs_apply_lds's wide ring (R 9..16; 16-byte table entries, a 5-slot input
                   ring) pinned to its consecutive and its Q8 instance, over K on every edge of
                   the ring's prefill and loop (K < 4, K = 5, 6, K not a multiple of 5); rows
                   all written, written and compared, all compared; flipped bytes flagged
  wide-rule        the wide rule's order on both sides of 256 tiles per stripe, two launch
                   groups, and the Split layout's unaligned 16-B accesses
  wide-lds-opt-in  K > 128: more than 64 KiB of tables, before and after a launch without them
  narrow-verify    R <= 8 launches the rule gives the bit-sliced kernel: read-only and
                   one-erasure plans (kLdsVerify, the all-compared triples, the v_perm kernel),
                   R 5..8 rings at K >= 20, R <= 4 at K = 24, the io.ReadAll layout
  host-path        the host-memory entry points, staged over several chunks, and the batch calls

CALLFS_RS_BITSLICE is read once per process, so each group runs in a fresh child, which prints
one line per case; the test counts them, so a child that skipped cases fails.
tests/test_native_launch_record.py (--wide) shows on the CPU that the wide ring's 16 pins
dispatch 16 different kernels, which no byte comparison can."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import sys
import time
import numpy as np
import torch
from oracle import cref
from callfs_amd import Codec, ErasureProfile, erasure as E, _native as N
from callfs_amd.device import Plan, StripeBatch, _aligned_empty

GROUP = sys.argv[1]
DEV = torch.device("cuda:0")
T0 = time.time()
N.lib.rs_tune_table_reset(None)  # the forms below are the rule's, not a tuner's
state = {"ok": 0, "fail": 0}
seen = set()


def fail(case, form, what, stripe="-", shard="-"):
    state["fail"] += 1
    print("FAIL %s form=%s stripe=%s shard=%s: %s" % (case, form, stripe, shard, what), flush=True)


def consistent(k, m, S, batch, seed, layout="planar"):
    # a resident batch whose parity the oracle computed, and its host image [batch][n][S]
    sb = StripeBatch(k, m, S, batch, DEV, layout=layout)
    sb.fill_random(seed)
    host = sb.gather().cpu().numpy()
    for b in range(batch):
        want = cref.encode([host[b, i] for i in range(k)], k, m)
        for j in range(m):
            host[b, k + j] = want[j]
            sb.shard(b, k + j).copy_(torch.from_numpy(want[j]))
    return sb, host


def lose(k, m, e):
    # e lost shards: data first, then parity
    d = min(k, e)
    return list(range(d)) + list(range(k, k + e - d))


def differing(got, host):
    if np.array_equal(got, host):
        return []
    return [(b, i) for b in range(host.shape[0]) for i in range(host.shape[1])
            if not np.array_equal(got[b, i], host[b, i])]


def run_case(case, plan, S, prepare, image, host, pin=None, want_forms=None, flip=None):
    # One case: pin (or keep the rule), require a nibble-table form, launch over the zeroed
    # outputs and compare every shard of every stripe; flip(b, pos) toggles a byte of a
    # compared shard of stripe b.
    before = state["fail"]
    groups = int(N.lib.rs_plan_groups(plan.handle))
    if pin is not None:
        plan.set_orders([pin] * groups)
        want_forms = [pin] * groups
    forms = plan.forms()
    form = ",".join(forms)
    seen.update(forms)
    if want_forms is not None and forms != want_forms:
        fail(case, form, "forms() is not %s" % want_forms)
    if any(f.startswith("bs") for f in forms):
        fail(case, form, "a bit-sliced form with CALLFS_RS_BITSLICE=0")
    try:
        plan.set_orders(["bs"] * groups)
        fail(case, form, "set_orders(['bs']) was accepted")
    except N.NativeError as e:
        if e.code != N.RS_E_ARG:
            fail(case, form, "set_orders(['bs']) failed with %d, not RS_E_ARG" % e.code)
    if plan.forms() != forms:
        fail(case, form, "a refused set_orders changed the plan: %s" % plan.forms())

    def launch_and_compare(want_flagged, what):
        plan.launch()
        flagged = plan.corrupt_stripes()
        if flagged != want_flagged:
            fail(case, form, "%s: corrupt_stripes() = %s, not %s" % (what, flagged, want_flagged))
        for b, i in differing(image(), host):
            fail(case, form, what + ": bytes differ from the oracle's", b, i)

    prepare()
    launch_and_compare([], "launch")
    if flip is not None:
        for b, pos in ((1, 100), (2, S - 3)):
            flip(b, pos)
            plan.launch()
            flagged = plan.corrupt_stripes()
            if flagged != [b]:
                fail(case, form, "byte %d of stripe %d flipped: corrupt_stripes() = %s" % (pos, b, flagged))
            flip(b, pos)
        launch_and_compare([], "after flipping back")
    if state["fail"] == before:
        state["ok"] += 1
        print("ok %s form=%s" % (case, form), flush=True)


def batch_case(sb, host, kind, lost, present, tag="", **kw):
    # a launch over a StripeBatch that rebuilds `lost` in place
    n = sb.k + sb.m
    plan = Plan.for_batch(sb, present=present)
    compared = present is not None and len(lost) < sb.m

    def prepare():
        for i in lost:
            sb.zero_shard(i)

    def flip(b, pos):
        sb.shard(b, n - 1)[pos] ^= 0x21  # the last compared shard

    case = "RS(%d,%d) S=%d %s%s" % (sb.k, sb.m, sb.S, kind, tag)
    pins = kw.pop("pins", [None])
    for pin in pins:
        run_case(case + (" pin=" + pin if pin else ""), plan, sb.S, prepare,
                 lambda: sb.gather().cpu().numpy(), host, pin=pin,
                 flip=flip if compared and sb.batch >= 3 else None, **kw)
    plan.close()


def launches(sb, host, kinds, **kw):
    k, m, n = sb.k, sb.m, sb.k + sb.m
    for kind in kinds:
        if kind == "enc":
            batch_case(sb, host, kind, list(range(k, n)), None, **kw)
            continue
        e = {"dec-m": m, "dec-part": max(1, m // 2), "dec-9": 9, "read-only": 0}.get(kind)
        lost = [1 if k > 1 else 0] if kind == "dec-1" else lose(k, m, e)
        batch_case(sb, host, kind, lost, [i not in lost for i in range(n)], **kw)


WIDE = ["enc", "dec-m", "dec-part", "read-only"]
PINS = ["consecutive", "q8"]


def wide_ring():
    S = 2 * 8192 + 16 * 37 + 9  # two full tiles, a partial wave and a 9-byte tail
    for m in range(9, 17):
        for k in (1, 2, 4, 5, 6, 11, 33):
            sb, host = consistent(k, m, S, 3, seed=k * 131 + m)
            launches(sb, host, WIDE, pins=PINS)
    S = 40 * 8192 + 16 * 5 + 3  # Q8 permutes tiles from 8 tiles per segment
    for k, m in ((5, 9), (11, 16)):
        sb, host = consistent(k, m, S, 3, seed=k + m)
        launches(sb, host, WIDE, pins=["q8"])


def split_case(k, m, S, off):
    # upstream Split of a contiguous object: every shard at its own byte offset
    n, batch = k + m, 2
    total = batch * n * S
    buf = torch.randint(0, 256, (total + 64,), dtype=torch.uint8, device=DEV)
    base = buf.data_ptr() + off
    ptrs = [base + (b * n + i) * S for b in range(batch) for i in range(n)]
    host = buf.cpu().numpy()[off:off + total].copy().reshape(batch, n, S)
    for b in range(batch):
        want = cref.encode([host[b, i] for i in range(k)], k, m)
        for j in range(m):
            host[b, k + j] = want[j]
    good = torch.from_numpy(host.reshape(-1)).to(DEV)
    plan = Plan(k, m, S, batch, ptrs)

    def prepare():
        buf[off:off + total].copy_(good)
        for b in range(batch):
            s0 = off + (b * n + k) * S
            buf[s0:s0 + m * S].zero_()

    run_case("RS(%d,%d) S=%d split off=%d enc" % (k, m, S, off), plan, S, prepare,
             lambda: buf[off:off + total].cpu().numpy().reshape(batch, n, S), host)
    plan.close()


def wide_rule():
    for S, form in (((2 << 20) + 3 * 8192 + 16 * 5 + 3, "q8"), (65_536 + 45, "consecutive")):
        sb, host = consistent(4, 9, S, 2, seed=S % 1000)
        launches(sb, host, WIDE, want_forms=[form])
        del sb
    for k, m in ((10, 20), (6, 17)):  # two launch groups: 16 rows, then 4 and 1
        sb, host = consistent(k, m, 40_013, 2, seed=k + m)
        if int(N.lib.rs_plan_groups(Plan.for_batch(sb).handle)) != 2:
            fail("RS(%d,%d)" % (k, m), "-", "not two launch groups")
        launches(sb, host, ["enc", "dec-9"])
    split_case(12, 9, 65_539, 5)
    split_case(20, 10, 65_539, 5)


def wide_lds_opt_in():
    S = 8192 + 16 * 5 + 3
    # RS(20,16) needs no opt-in and runs before RS(240,16), which does, with the same R
    for k, m in ((129, 9), (140, 13), (247, 9), (20, 16), (240, 16)):
        sb, host = consistent(k, m, S, 2, seed=k)
        launches(sb, host, ["enc", "dec-m"], pins=PINS)


def readall_case(k, m, S, batch, tag):
    # CallFS's io.ReadAll layout: survivors at odd offsets, the lost shards rebuilt into
    # buffers of their own, the remaining parity compared
    n = k + m
    sb, host = consistent(k, m, S, batch, seed=S + k, layout="readall")
    fp = -(-S // 64) * 64
    for erase in ([1], [0, k]):
        fresh = _aligned_empty((batch, len(erase), fp), 256, DEV)
        ptrs = list(sb.pointers())
        for b in range(batch):
            for j, i in enumerate(erase):
                ptrs[b * n + i] = fresh[b, j].data_ptr()
        plan = Plan(k, m, S, batch, ptrs, present=[i not in erase for i in range(n)])

        def image():
            got = sb.gather().cpu().numpy()
            new = fresh.cpu().numpy()
            for j, i in enumerate(erase):
                got[:, i] = new[:, j, :S]
            return got

        def flip(b, pos):
            sb.shard(b, n - 1)[pos] ^= 0x21

        run_case("RS(%d,%d) S=%d readall%s lost=%s" % (k, m, S, tag, erase), plan, S,
                 lambda: fresh.fill_(0xA5), image, host, flip=flip)
        plan.close()


def narrow_verify():
    S = 3 * 8192 + 1024 + 16 * 37 + 9
    for k, m in ((5, 1), (5, 2), (5, 3), (5, 4), (10, 5), (10, 6), (10, 7), (10, 8)):
        sb, host = consistent(k, m, S, 3, seed=k * 131 + m)
        launches(sb, host, ["read-only", "dec-1"])
    for k, m in ((3, 2), (2, 4), (1, 3)):  # k <= 3 and R <= 4: the v_perm kernel
        sb, host = consistent(k, m, S, 3, seed=k * 131 + m)
        launches(sb, host, ["read-only"])
    for k, m in ((20, 5), (24, 8), (32, 8)):
        sb, host = consistent(k, m, S, 3, seed=k * 131 + m)
        launches(sb, host, ["enc", "dec-m", "dec-1"])
    sb, host = consistent(24, 4, 600_000, 3, seed=24)  # 74 tiles per stripe
    launches(sb, host, ["enc"])
    del sb
    for k, m, batch in ((10, 8, 3), (10, 8, 4), (8, 8, 3), (16, 8, 3)):
        readall_case(k, m, 122_190, batch, " batch=%d" % batch)


def host_case(case, check):
    before = state["fail"]
    check(case)
    if state["fail"] == before:
        state["ok"] += 1
        print("ok %s form=host" % case, flush=True)


def as_u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def host_path():
    rng = np.random.default_rng(21)
    c = Codec()
    for k, m, L in ((20, 12, 5 * (1 << 20) + 13), (6, 9, 70_001)):
        prof = ErasureProfile(k, m)
        data = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        sh = c.encode(data, prof)

        def encoded(case):
            want = cref.encode([as_u8(sh[i]) for i in range(k)], k, m)
            for j in range(m):
                if not np.array_equal(as_u8(sh[k + j]), want[j]):
                    fail(case, "host", "parity differs from the oracle's", 0, k + j)

        def decoded(case):
            lost = list(sh)
            for i in list(range(0, k, 3))[: m // 2] + list(range(k, k + m - m // 2)):
                lost[i] = None
            if c.decode(lost, prof, L) != data:
                fail(case, "host", "decode does not return the object")

        host_case("RS(%d,%d) L=%d Codec.encode" % (k, m, L), encoded)
        host_case("RS(%d,%d) L=%d Codec.decode" % (k, m, L), decoded)
    k, m = 20, 12
    st = [[rng.integers(0, 256, 65_536 + 7 * b, dtype=np.uint8).tobytes() for _ in range(k)]
          for b in range(5)]
    par, status = E.encode_batch(st, k, m)

    def batch_encoded(case):
        if list(status) != [0] * 5:
            fail(case, "host", "status %s" % list(status))
        for b in range(5):
            want = cref.encode([as_u8(s) for s in st[b]], k, m)
            for j in range(m):
                if not np.array_equal(as_u8(par[b][j]), want[j]):
                    fail(case, "host", "parity differs from the oracle's", b, k + j)

    def batch_rebuilt(case):
        full = [list(st[b]) + [bytes(p) for p in par[b]] for b in range(5)]
        gone = (0, 5, 9, 20, 21, 22, 23, 24, 25, 26)
        dmg = [[None if i in gone else s for i, s in enumerate(f)] for f in full]
        got = E.reconstruct_batch(dmg, k, m)
        if list(got) != [0] * 5:
            fail(case, "host", "status %s" % list(got))
        for b in range(5):
            for i in range(k + m):
                if bytes(dmg[b][i]) != full[b][i]:
                    fail(case, "host", "shard differs from the oracle's", b, i)

    host_case("RS(20,12) five stripes encode_batch", batch_encoded)
    host_case("RS(20,12) five stripes reconstruct_batch", batch_rebuilt)


{"wide-ring": wide_ring, "wide-rule": wide_rule, "wide-lds-opt-in": wide_lds_opt_in,
 "narrow-verify": narrow_verify, "host-path": host_path}[GROUP]()
torch.cuda.synchronize()
print("forms seen: %s" % " ".join(sorted(seen)))
print("%.1f s after the imports" % (time.time() - T0))
print("nibble fallback %s: %d ok, %d failed" % (GROUP, state["ok"], state["fail"]), flush=True)
sys.exit(1 if state["fail"] else 0)
"""

# The number of cases (`ok` lines) each group's child must report:
#   wide-ring        8 m x 7 K x 4 launches x 2 pins, and 2 profiles x 4 launches in Q8 at 41 tiles
#   wide-rule        RS(4,9) at 2 sizes x 4 launches, 2 two-group profiles x 2 launches, 2 Split
#   wide-lds-opt-in  5 profiles x 2 launches x 2 pins
#   narrow-verify    8 x 2, 3 read-only, 3 x 3, RS(24,4), 4 io.ReadAll shapes x 2 erasure sets
#   host-path        2 objects x (encode, decode), encode_batch, reconstruct_batch
GROUPS = {"wide-ring": 8 * 7 * 4 * 2 + 2 * 4, "wide-rule": 2 * 4 + 2 * 2 + 2,
          "wide-lds-opt-in": 5 * 2 * 2, "narrow-verify": 8 * 2 + 3 + 3 * 3 + 1 + 4 * 2,
          "host-path": 2 * 2 + 2}


@pytest.mark.parametrize("group", list(GROUPS))
def test_nibble_kernels_vs_oracle(native_lib, group):
    """One fresh child per group with CALLFS_RS_BITSLICE=0: every case `ok`, none skipped. A
    fault, an abort or the time limit in the child fails the test with its output."""
    path = os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p])
    env = dict(os.environ, CALLFS_RS_BITSLICE="0", PYTHONPATH=path)
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD, group], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        pytest.fail("the %s child ran into its time limit\n%s\n%s" % (group, e.stdout, e.stderr))
    out = r.stdout[-6000:] + r.stderr[-4000:]
    assert r.returncode == 0, out
    lines = r.stdout.splitlines()
    oks = sum(ln.startswith("ok ") for ln in lines)
    print("\n".join(lines[-3:]))
    assert lines[-1] == "nibble fallback %s: %d ok, 0 failed" % (group, GROUPS[group]), out
    assert oks == GROUPS[group] and not any(ln.startswith("FAIL") for ln in lines), out
