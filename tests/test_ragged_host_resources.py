"""Register report of the kernels behind heterogeneous host batches (CPU, no GPU needed):
the sixteen rs_apply_small_ragged instances are recorded in callfs_amd/kernel_resources.json
with no scratch and no VGPR spills, and the mixed and ragged LDS instances the staged and
direct transports launch keep the VGPRs and waves per SIMD they had before the host path
used them."""
import json
import os
import re

import pytest

from callfs_amd import build as nb


@pytest.fixture(scope="module")
def kernels():
    if nb._stale() or not os.path.exists(nb.RESOURCES):
        nb.build()
    with open(nb.RESOURCES) as fh:
        return json.load(fh)["kernels"]


def test_sixteen_small_ragged_instances_are_clean(kernels):
    small = {int(re.search(r"rs_apply_small_ragged<(\d+)>", k["name"]).group(1)): k
             for k in kernels if "rs_apply_small_ragged<" in k["name"]}
    assert sorted(small) == list(range(1, 17))
    for r, k in small.items():
        assert k.get("scratch", 0) == 0, k["name"]
        assert k.get("vgpr_spill", 0) == 0, k["name"]
        assert k["vgprs"] + k.get("agprs", 0) <= 256, k["name"]


# (rows of the instance) -> (vgprs, waves_per_simd), as recorded before this feature
MIXED = {4: (58, 8), 8: (64, 8), 16: (120, 4)}
RAGGED = {4: (58, 8), 8: (62, 8), 16: (120, 4)}


@pytest.mark.parametrize("kernel,want", [("rs_apply_mixed", MIXED), ("rs_apply_ragged", RAGGED)])
def test_mixed_and_ragged_instances_unmoved(kernels, kernel, want):
    got = {}
    for k in kernels:
        mt = re.search(kernel + r"<(\d+),", k["name"])
        if mt:
            got[int(mt.group(1))] = (k["vgprs"], k["waves_per_simd"])
    assert got == want
