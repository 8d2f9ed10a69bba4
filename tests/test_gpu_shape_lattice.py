"""Every tile-map kernel kind (mixed, ragged, required, update pair and single, decode-idx merge
and store, final decode-check merge and store, decode-repair merge and store, locate, locate2,
correct) over one lattice of source
counts and row counts, so that every instance (RT 4 for R <= 4, RT 8 for R 5..8, RT 16 for R 9..16)
of every kind runs at the edges of its input ring (3 slots for RT <= 8, 5 for RT 16), of the early
compare point (4 sources before the end) and of its row loops, in first and in second launch
groups, and so that the > 64 KiB dynamic-LDS opt-in is exercised for every kind.

Expected bytes come from oracle.cref alone (tests/shape_lattice.py holds the arena and one runner
per kind), exact. Every plan lives in a sentinel-guarded allocation in the packed, odd-offset layout
and the whole allocation is compared after every launch; before a launch the runner asserts on the
CPU that every written row's expected bytes differ from its starting bytes. Stripes cycle through
the sizes 5 (tail only), 16 (one vector), 40 (two vectors and a tail) and 8211 (a full tile, one
lane of a second, a 3-byte tail). Every case asserts the plan's kernel forms and launch groups."""
import json
import os
import subprocess
import sys

import pytest

import shape_lattice as SL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# both sides of the ring depths 3 and 5 and of the early-compare distance 4; not all multiples of 5
INPUTS = (1, 2, 3, 4, 5, 6, 7, 9, 11)
# per instance class: its widest row count, and the row counts of the row axis: the lower edge,
# the upper edge and counts that are no multiple of 4
CLASS_ROWS = {"rt4": 4, "rt8": 8, "rt16": 16}
ROW_AXIS = {"rt4": (1, 2, 3, 4), "rt8": (5, 6, 7, 8), "rt16": (9, 10, 13, 16)}
SECOND_GROUPS = (17, 21, 25, 32)  # at k = 5: second groups of 1, 5, 9 and 16 rows
REBUILD = ("mixed", "ragged", "required")
COUNTED = ("update-pair", "update-single", "merge", "merge-store", "check", "check-store", "repair", "repair-store")
REPAIR = ("repair", "repair-store")
LOCATE = ("locate", "locate2", "correct")
KINDS = REBUILD + COUNTED + LOCATE


@pytest.fixture(autouse=True)
def _no_tuned_forms(native_lib):
    """Forms compared below are the rule's: forget what other tests' tuners recorded."""
    native_lib.lib.rs_tune_table_reset(None)
    yield
    native_lib.lib.rs_tune_table_reset(None)


def _narrow(m):
    """Row counts below m for the stripes that run in a wider instance than they need: 1 and 9
    beside 16, 5 beside 8."""
    return SL.narrow_rows(m)


def _idx_sets(k, m, counts):
    """Decode-idx stripes, one per source count: its own expected set; stripe 0 wants every other
    shard (m rows), the rest fewer, from either end of the row list."""
    widths = [m] + _narrow(m)
    expect, wanted = [], []
    for b in range(len(counts)):
        e = SL.expected_set(k, m, b)
        rest = [i for i in range(k + m) if i not in e]
        w = widths[b % len(widths)]
        expect.append(e)
        wanted.append(tuple(rest[:w] if b % 2 == 0 else rest[-w:]))
    return expect, wanted


def _check_sets(k, m, counts, store, seed):
    """Final decode-check stripes, one per source count C (store: C counts the delivered compared
    shards too). Stripe 0 has m rows, the rest fewer; one or two check rows at the front, at the
    back or in the middle of the row list; every third stripe damaged, in the vector body and in the
    tail in turn. A stripe with no expected source has no wanted row: it only scans."""
    widths = [m] + _narrow(m)
    expect, wanted, compared, nfeed, damage = [], [], [], [], []
    for b, C in enumerate(counts):
        e = SL.expected_set(k, m, b)
        rest = [i for i in range(k + m) if i not in e]
        w = widths[b % len(widths)]
        rows = rest[:w] if b % 2 == 0 else rest[-w:]
        ncmp = min(1 + b % 2, w, max(C, 1) if store else w)
        if w > 16 and C >= 3:  # two launch groups: check rows on both sides of row 16
            cmp_ = sorted({rows[1], rows[16], rows[-1]})
        elif b % 3 == 0:
            cmp_ = rows[:ncmp]
        elif b % 3 == 1:
            cmp_ = rows[-ncmp:]
        else:
            cmp_ = sorted({rows[len(rows) // 2], rows[0]} if ncmp > 1 else {rows[len(rows) // 2]})
        nf = max(0, C - (len(cmp_) if store else 0))
        expect.append(e)
        compared.append(tuple(cmp_))
        wanted.append(tuple(i for i in rows if i not in cmp_) if nf else ())
        nfeed.append(nf)
        damage.append((b // 3) % 2 if b % 3 == 1 else None)
    feeds = SL.pick_sets(k, nfeed, seed)
    return expect, wanted, compared, feeds, damage


def _run_counted(kind, k, m, counts, seed):
    """One plan of a kind whose input axis is the per-stripe source count."""
    sizes = SL.cycle_sizes(len(counts), first=seed)
    if kind.startswith("update"):
        SL.run_update(k, m, sizes, SL.pick_sets(k, counts, seed), pair=kind == "update-pair", seed=seed)
    elif kind.startswith("merge"):
        expect, wanted = _idx_sets(k, m, counts)
        assert max(len(w) for w in wanted) == m
        SL.run_decode_idx(k, m, sizes, expect, wanted, SL.pick_sets(k, counts, seed),
                          store=kind == "merge-store", seed=seed)
    elif kind in REPAIR:
        store = kind == "repair-store"
        md = SL.run_decode_repair(k, m, SL.repair_counted(k, m, counts, store, seed), store, seed=seed)
        SL.check_repair_counted(md, k, m, counts, store)
    else:
        store = kind == "check-store"
        # the widest stripe, stripe 0, has the most sources; the last has none: its accumulators
        # are only scanned (merge) or nothing of it is read (store)
        counts = tuple(counts)[::-1] + (0,)
        sizes = SL.cycle_sizes(len(counts), first=seed)
        expect, wanted, compared, feeds, damage = _check_sets(k, m, counts, store, seed)
        if store:
            damage[-1] = None
        assert len(wanted[0]) + len(compared[0]) == m and not feeds[-1] and compared[-1]
        assert any(d is not None for d in damage) and any(d is None for d in damage)
        SL.run_decode_check(k, m, sizes, expect, wanted, compared, feeds, store, damage, seed=seed,
                            scan_only=(len(counts) - 1,))


def _run_profile(kind, k, m, seed):
    """One profile of a kind whose input axis is k."""
    if kind == "mixed":
        for S in (8211, 40, 5):  # 5: the byte kernel, <8> up to 8 rows and <16> above
            SL.run_rebuild("mixed", k, m, [S] * 5, SL.lattice_masks(k, m, 5, seed), seed=seed + S)
    elif kind == "ragged":
        SL.run_rebuild("ragged", k, m, SL.cycle_sizes(5, first=seed), SL.lattice_masks(k, m, 5, seed), seed=seed)
    elif kind == "required":
        masks, wanted = SL.required_sets(k, m, seed, narrow=_narrow(m)[:3])
        SL.run_rebuild("required", k, m, SL.cycle_sizes(len(masks), first=seed), masks, wanted, seed=seed)
    else:
        SL.run_locate_profile(kind, k, m, seed=seed)


@pytest.mark.parametrize("cls", list(CLASS_ROWS))
@pytest.mark.parametrize("kind", KINDS)
def test_input_axis(native_lib, kind, cls):
    """Source counts 1..11 on both sides of the ring depths and of the early-compare distance, at
    the widest row count of each instance class. For the kinds that stage every input it is k, one
    plan per profile; for the others one RS(11, m) plan has a stripe per source count."""
    m = CLASS_ROWS[cls]
    if kind in COUNTED:
        _run_counted(kind, 11, m, INPUTS, seed=m)
    else:
        for k in INPUTS:
            _run_profile(kind, k, m, seed=10 * k + m)


@pytest.mark.parametrize("cls", list(CLASS_ROWS))
@pytest.mark.parametrize("kind", KINDS)
def test_row_axis(native_lib, kind, cls):
    """Every instance at its lower edge, its upper edge and row counts that are no multiple of 4,
    at k = 3 and k = 6; the kinds whose patterns have their own row counts put narrower stripes into
    the same plan."""
    for k in (3, 6):
        for m in ROW_AXIS[cls]:
            if kind in COUNTED:
                _run_counted(kind, k, m, sorted({1, 2, k}), seed=100 * k + m)
            else:
                _run_profile(kind, k, m, seed=100 * k + m)


@pytest.mark.parametrize("kind", [kind for kind in REBUILD + COUNTED if kind not in REPAIR])
def test_second_launch_groups(native_lib, kind):
    """RS(5, m) with m = 17, 21, 25, 32: a second launch group of 1, 5, 9 and 16 rows, so of every
    instance class. The mixed masks hold an encode and decode patterns; the decode-check stripes
    have check rows on both sides of row 16. (A decode-repair stripe has at most 16 rows and one
    group: test_gpu_decode_repair.py holds the 17-row refusal.)"""
    for m in SECOND_GROUPS:
        if kind in COUNTED:
            _run_counted(kind, 5, m, (1, 3, 5, 4), seed=m)
        else:
            _run_profile(kind, 5, m, seed=m)


@pytest.mark.parametrize("kind", LOCATE)
def test_locate_kinds_have_one_group(native_lib, kind):
    """RS(5,17) with everything present: 16 of the 17 compared shards are examined, in one group
    (run_locate asserts the groups)."""
    exp = SL.run_locate_profile(kind, 5, 17, seed=3)
    assert exp[0].any() and not exp[-1].any()


@pytest.mark.parametrize("mode", ["merge", "store"])
def test_decode_check_five_to_eight_rows(native_lib, mode):
    """The RT 8 instances of the final decode-check kernel: RS(10,8) stripes with 5, 6, 7 and 8
    rows, the check rows among the first four rows, among the rest, and on both sides; per shape a
    clean stripe, one damaged in the vector body and one damaged in the tail. The flagged stripes
    are exactly the damaged ones (run_decode_check asserts it against the rule and the launch)."""
    k, m = 10, 8
    store = mode == "store"
    expect, wanted, compared, nfeed, damage = [], [], [], [], []
    for rows in (5, 6, 7, 8):
        for place in ("front", "back", "both"):
            for dmg in (None, 0, 1):
                b = len(expect)
                e = SL.expected_set(k, m, b)
                rest = [i for i in range(k + m) if i not in e]
                lst = rest[:rows] if b % 2 else rest[-rows:]
                cmp_ = {"front": lst[1:3], "back": lst[-2:], "both": [lst[0], lst[4], lst[-1]]}[place]
                assert (place == "front") == all(lst.index(j) < 4 for j in cmp_)
                assert (place == "back") == all(lst.index(j) >= 4 for j in cmp_) or rows == 5
                expect.append(e)
                compared.append(tuple(sorted(set(cmp_))))
                wanted.append(tuple(i for i in lst if i not in cmp_))
                nfeed.append(k if b % 4 else 7)
                damage.append(dmg)
    sizes = [(40, 8211)[b % 2] for b in range(len(expect))]
    hit = {(sizes[b], damage[b]) for b in range(len(expect)) if damage[b] is not None}
    assert hit == {(40, 0), (40, 1), (8211, 0), (8211, 1)}  # body and tail, at both sizes
    assert {len(w) + len(c) for w, c in zip(wanted, compared)} == {5, 6, 7, 8}
    feeds = SL.pick_sets(k, nfeed, seed=58)
    SL.run_decode_check(k, m, sizes, expect, wanted, compared, feeds, store, damage, seed=58)


# ---- decode-repair: its two row axes, and runs inside one 16-byte vector ------------------------

@pytest.mark.parametrize("mode", ["merge", "store"])
@pytest.mark.parametrize("shape", [s for cls in SL.REPAIR_ROWS.values() for s in cls], ids=lambda s: "%d+%d" % s)
def test_repair_row_axes(native_lib, shape, mode):
    """(check rows, wanted rows) at the edges of every instance class -- 5 and 9 rows, 16 check rows
    and no wanted row -- at check-row counts that straddle a 4-row group and reach words 2 and 3 of
    the packed accumulator, at k = 3 and k = 6: a clean stripe, an expected shard's byte in the
    vector body, the last check row's compared shard (syndrome byte r' - 1) in the tail, the first
    check row's compared shard."""
    nchk, nwant = shape
    for k in (3, 6):
        seed = 100 * k + 16 * nchk + nwant
        stripes = SL.repair_row_stripes(k, nchk, nwant, mode == "store", seed)
        md = SL.run_decode_repair(k, nchk + nwant, stripes, mode == "store", seed=seed)
        SL.check_repair_rows(md, nchk, nwant)


@pytest.mark.parametrize("fix", ["zero", "mixed"])
@pytest.mark.parametrize("mode", ["merge", "store"])
@pytest.mark.parametrize("shape", SL.RUN_SHAPES, ids=lambda s: "%d+%d" % s)
def test_repair_runs_within_a_vector(native_lib, shape, mode, fix):
    """Several verdicts inside one 16-byte vector (SL.repair_run_stripes): the gathered error vector
    is applied when the verdict changes, twice into one fix vector, after an unexplained column, in
    every column in turn, at positions k - 1 and k, with the flush flags and run lengths differing
    from lane to lane; in vector 0, lanes 63 and 64, the first vector of tile 1 and the last vector
    before the tail. With A's fix pointer null the wanted rows and the counts are the same."""
    store = mode == "store"
    stripes, names = SL.repair_run_stripes(*shape, store, fix)
    md = SL.run_decode_repair(10, sum(shape), stripes, store, seed=7 * shape[0] + shape[1])
    SL.check_repair_runs(md, names, shape, fix)


# ---- the > 64 KiB dynamic-LDS opt-in ---------------------------------------------------------

@pytest.fixture(scope="module")
def wide_results():
    """The opt-in is set once per process, device and kind, so the order of launches is the test:
    a fresh child runs, per kind, RS(20,16), RS(128,16) (exactly 64 KiB of tables), RS(129,9)
    (66,048 B: the first shape that needs the opt-in), RS(240,16) and RS(20,16) again, each checked
    against the oracle at the sizes 40 and 8211."""
    env = dict(os.environ)
    paths = [ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else [])
    env["PYTHONPATH"] = os.pathsep.join(paths)
    r = subprocess.run([sys.executable, "-c", "import sys, shape_lattice; sys.exit(shape_lattice.wide_child())"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("WIDE_LDS_RESULT ")]
    assert lines, "no result line (exit %d): %s" % (r.returncode, r.stdout[-2000:] + r.stderr[-4000:])
    return r.returncode, json.loads(lines[-1][len("WIDE_LDS_RESULT "):])


@pytest.mark.parametrize("kind", SL.WIDE_KINDS)
def test_wide_lds(native_lib, wide_results, kind):
    """k * 512 B of tables with 16-byte entries: no opt-in at k = 20 and k = 128, the opt-in at
    k = 129 and k = 240, and the small profile again afterwards. RS(240,16) with everything present
    examines 256 shards: the locate kinds hit shards 0, 127, 128, 239, 240 and 255, locate2 also the
    pair (239, 255), correct repairs shards 255 and 200."""
    code, results = wide_results
    res = results[kind]
    assert res["error"] is None, res["error"]
    assert [tuple(p) for p in res["passed"]] == list(SL.WIDE_PROFILES)
    assert code == 0
    assert 128 * 512 == 64 << 10 < 129 * 512 == 66_048
