"""No GPU needed: the code objects of the probe-gather kernels (kernels_probe.hip), cross-compiled for gfx950 as the Makefile builds the unit.
Each kernel is there once, uses no scratch, spills nothing and declares no static LDS (the gather's walk stack is the launch's dynamic
LDS, sized from the tree); each is held to the register count it compiles to."""
import os

import pytest

from test_kernel_resources import HIPCC, kernel_table, uncontracted_units
from test_refit_resources import named

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# vgpr_count of the code objects' metadata (hipcc -S --cuda-device-only --offload-arch=gfx950 -O3 -ffp-contract=off, ROCm's clang), read off
# this very table when the kernels were written: 80 for the gather -- the occlusion walk with the probe and 28 accumulators held across it;
# six waves per SIMD, the launch bound it declares, leave exactly 80 -- and 66 for the reduce (28 sums and the loads in flight).
VGPRS = {"probe_gather_kernel": 80, "probe_reduce_kernel": 66}


@pytest.fixture(scope="module")
def table():
    return kernel_table("kernels_probe.hip")


def test_the_unit_is_built_without_contraction():
    assert "kernels_probe.hip" in uncontracted_units()


@pytest.mark.parametrize("name", sorted(VGPRS))
def test_each_kernel_is_there_once_without_scratch_or_spills_at_its_register_count(table, name):
    hits = named(table, name)
    assert len(hits) == 1, (name, sorted(k for k in table if "evplp" in k))
    t = table[hits[0]]
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (name, t)
    assert t["group_segment_fixed_size"] == 0, (name, t)
    assert t["vgpr_count"] <= VGPRS[name], (name, t)
