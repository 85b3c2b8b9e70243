"""No GPU needed: the code objects of the surface-gather kernels (kernels_surface.hip), cross-compiled for gfx950 as the Makefile builds the
unit.  Each kernel is there once, uses no scratch and spills nothing; the two walking kernels -- the VPL half, whose shadow-ray stack is the
launch's dynamic LDS, and the photon query -- declare no static LDS (nor does any other); each is held to the register count it compiles to."""
import os

import pytest

from test_kernel_resources import HIPCC, kernel_table, uncontracted_units
from test_refit_resources import named

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# vgpr_count of the code objects' metadata (hipcc -S --cuda-device-only --offload-arch=gfx950 -O3 -ffp-contract=off, ROCm's clang), read off
# this very table when the kernels were written: 71 for the VPL half -- the occlusion walk with the receiver's sixteen floats, its view
# direction and four accumulators held across it; seven waves per SIMD, the launch bound it declares, leave 72 -- and 60 for the photon
# query (the receiver, the range's six cell indices, the compact photon in flight).
VGPRS = {"surface_vpl_kernel": 71, "surface_photon_kernel": 60, "surface_cell_kernel": 11, "surface_bucket_kernel": 8, "surface_compact_kernel": 39,
         "surface_reduce_kernel": 17}
WALKING = ("surface_vpl_kernel", "surface_photon_kernel")


@pytest.fixture(scope="module")
def table():
    return kernel_table("kernels_surface.hip")


def test_the_unit_is_built_without_contraction():
    assert "kernels_surface.hip" in uncontracted_units()


@pytest.mark.parametrize("name", sorted(VGPRS))
def test_each_kernel_is_there_once_without_scratch_or_spills_at_its_register_count(table, name):
    hits = named(table, name)
    assert len(hits) == 1, (name, sorted(k for k in table if "evplp" in k))
    t = table[hits[0]]
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (name, t)
    assert t["group_segment_fixed_size"] == 0, (name, t)
    assert t["vgpr_count"] <= VGPRS[name], (name, t)


def test_the_walking_kernels_are_among_them():
    assert set(WALKING) <= set(VGPRS)
