"""No GPU needed: the code objects of the k-nearest start radius' kernels (kernels_surface_knn.hip), cross-compiled for gfx950 as the Makefile
builds the unit.  The unit is uncontracted; each kernel is there once, uses no scratch and spills nothing -- the select's 16 counters per
lane live in LDS exactly so that they do not go to scratch, and the 16 words read back for knn_select.h's ks_step must stay in registers
--; the select declares its uint32 hist[16][64] and nothing more (4096 bytes), the photon kernel no LDS; and each is held to the register
count it compiles to."""
import os

import pytest

from test_kernel_resources import HIPCC, kernel_table, uncontracted_units
from test_refit_resources import named

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# vgpr_count of the code objects' metadata (hipcc -S --cuda-device-only --offload-arch=gfx950 -O3 -ffp-contract=off, ROCm's clang), read off
# this very table when the kernels were written.  The photon kernel is surface_prog_photon_kernel's walk (64 there).
VGPRS = {"surface_knn_select_kernel": 34, "surface_knn_photon_kernel": 64}
LDS = {"surface_knn_select_kernel": 4096, "surface_knn_photon_kernel": 0}


@pytest.fixture(scope="module")
def table():
    return kernel_table("kernels_surface_knn.hip")


def test_the_unit_is_built_without_contraction():
    assert "kernels_surface_knn.hip" in uncontracted_units()


@pytest.mark.parametrize("name", sorted(VGPRS))
def test_each_kernel_is_there_once_without_scratch_or_spills_at_its_register_count(table, name):
    hits = named(table, name)
    assert len(hits) == 1, (name, sorted(k for k in table if "evplp" in k))
    t = table[hits[0]]
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (name, t)
    assert t["group_segment_fixed_size"] <= LDS[name], (name, t)
    assert t["vgpr_count"] <= VGPRS[name], (name, t)


def test_the_selects_counters_are_the_only_lds(table):
    t = table[named(table, "surface_knn_select_kernel")[0]]
    assert t["group_segment_fixed_size"] == 4096, t
