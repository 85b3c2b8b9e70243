"""No GPU needed: the code objects of the progressive surface gather's kernels (kernels_surface_prog.hip), cross-compiled for gfx950 as the
Makefile builds the unit.  The unit is uncontracted; each kernel is there once, uses no scratch, spills nothing and declares no static LDS
-- the state goes through surface_state.h's update as a struct, which must stay in registers -- and each is held to the register count it
compiles to."""
import os

import pytest

from test_kernel_resources import HIPCC, kernel_table, uncontracted_units
from test_refit_resources import named

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# vgpr_count of the code objects' metadata (hipcc -S --cuda-device-only --offload-arch=gfx950 -O3 -ffp-contract=off, ROCm's clang), read off
# this very table when the kernels were written: 64 for the query -- what surface_photon_kernel holds (60) and the state's words that wait
# for the update across the walk.
VGPRS = {"surface_prog_compact_kernel": 8, "surface_prog_fold_kernel": 16, "surface_prog_photon_kernel": 64, "surface_prog_resolve_kernel": 22,
         "lightmap_prog_resolve_kernel": 37}


@pytest.fixture(scope="module")
def table():
    return kernel_table("kernels_surface_prog.hip")


def test_the_unit_is_built_without_contraction():
    assert "kernels_surface_prog.hip" in uncontracted_units()


@pytest.mark.parametrize("name", sorted(VGPRS))
def test_each_kernel_is_there_once_without_scratch_or_spills_at_its_register_count(table, name):
    hits = named(table, name)
    assert len(hits) == 1, (name, sorted(k for k in table if "evplp" in k))
    t = table[hits[0]]
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (name, t)
    assert t["group_segment_fixed_size"] == 0, (name, t)
    assert t["vgpr_count"] <= VGPRS[name], (name, t)
