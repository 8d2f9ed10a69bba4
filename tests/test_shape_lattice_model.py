"""The decode-repair case tables of tests/test_gpu_shape_lattice.py, walked without a device: every
parametrised case builds its RepairModel (tests/shape_lattice.py), which asserts that every damaged
column is blamed or unexplained by the rule, that every row the launch rewrites differs from its
starting bytes and that every other row stays; the checks of the GPU tests that need only the model
-- the source and row counts, a damaged and a clean stripe, the counts the sequences give -- run
here too. Expected bytes come from oracle.cref alone."""
import numpy as np
import pytest

import shape_lattice as SL
import test_gpu_shape_lattice as TL


@pytest.mark.parametrize("store", [False, True], ids=["merge", "store"])
@pytest.mark.parametrize("cls", list(TL.CLASS_ROWS))
def test_input_axis_tables(cls, store):
    m = TL.CLASS_ROWS[cls]
    md = SL.RepairModel(11, m, SL.repair_counted(11, m, TL.INPUTS, store, m), store, seed=m)
    SL.check_repair_counted(md, 11, m, TL.INPUTS, store)
    assert len(md.stripes) == 10 and set(md.srcs) == set(TL.INPUTS) | {0}
    assert {1, m} <= set(md.nrows)


@pytest.mark.parametrize("store", [False, True], ids=["merge", "store"])
@pytest.mark.parametrize("cls", list(TL.ROW_AXIS))
def test_row_axis_tables(cls, store):
    for k in (3, 6):
        for m in TL.ROW_AXIS[cls]:
            counts, seed = sorted({1, 2, k}), 100 * k + m
            md = SL.RepairModel(k, m, SL.repair_counted(k, m, counts, store, seed), store, seed=seed)
            SL.check_repair_counted(md, k, m, counts, store)


@pytest.mark.parametrize("store", [False, True], ids=["merge", "store"])
@pytest.mark.parametrize("cls", list(SL.REPAIR_ROWS))
def test_repair_row_tables(cls, store):
    lo, hi = {"rt4": (1, 4), "rt8": (5, 8), "rt16": (9, 16)}[cls]
    for nchk, nwant in SL.REPAIR_ROWS[cls]:
        assert lo <= nchk + nwant <= hi
        for k in (3, 6):
            seed = 100 * k + 16 * nchk + nwant
            stripes = SL.repair_row_stripes(k, nchk, nwant, store, seed)
            md = SL.RepairModel(k, nchk + nwant, stripes, store, seed=seed)
            SL.check_repair_rows(md, nchk, nwant)
            assert store == (set(md.srcs) == {k + nchk})
    rows = {c + w for c, w in SL.REPAIR_ROWS[cls]}
    # both edges of the instance class (the 1- and 2-row stripes are the narrow ones of the axes)
    assert {max(lo, 3), hi} <= rows


@pytest.mark.parametrize("fix", ["zero", "mixed"])
@pytest.mark.parametrize("store", [False, True], ids=["merge", "store"])
@pytest.mark.parametrize("shape", SL.RUN_SHAPES, ids=lambda s: "%d+%d" % s)
def test_repair_run_tables(shape, store, fix):
    stripes, names = SL.repair_run_stripes(*shape, store, fix)
    md = SL.RepairModel(10, sum(shape), stripes, store, seed=7 * shape[0] + shape[1])
    SL.check_repair_runs(md, names, shape, fix)
    # every sequence sits once in each of the chosen vectors over stripes 0 and 1
    for b in (0, 1):
        vecs = {c // 16 for _, c, _ in stripes[b]["damage"]}
        assert set(SL.RUN_VECTORS) < vecs and len(vecs) == 6
    assert {c // 16 for _, c, _ in stripes[2]["damage"]} == {138, 139, 141}
    # a null fix pointer changes neither the wanted rows nor the counts
    other = SL.RepairModel(10, sum(shape), SL.repair_run_stripes(*shape, store, "zero")[0], store,
                           seed=7 * shape[0] + shape[1])
    assert np.array_equal(other.counts, md.counts)
    for b, st in enumerate(stripes):
        for w in st["wanted"]:
            assert np.array_equal(SL.get(other.want, other.off[b][w], SL.RUN_S), SL.get(md.want, md.off[b][w], SL.RUN_S))


@pytest.mark.parametrize("store", [False, True], ids=["merge", "store"])
def test_wide_tables(store):
    for k, m in sorted(set(SL.WIDE_PROFILES)):
        md = SL.RepairModel(k, m, SL.repair_wide_stripes(k, m, store), store, seed=k)
        assert md.rows == m > 8 and set(md.srcs) == {k} and md.nchk == [3] * 3 and md.flagged == [0, 1]
        assert not md.counts[:, k + m].any() and md.counts.sum() > 0
        if k + m == 256:
            assert md.stripes[0]["compared"] == (253, 254, 255) and md.counts[0, 255] == 1
            assert {st["expect"].index(s) for st in md.stripes[:1] for s, _, _ in st["damage"] if s < k} == {0, 127, 128, 239}
