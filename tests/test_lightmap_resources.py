"""No GPU needed: the code objects of the lightmap kernels (kernels_lightmap.hip), cross-compiled for gfx950 as the Makefile builds the unit.
Each kernel is there once -- the raster kernel once per sample count, 1, 2 and 4 per axis -- uses no scratch and spills nothing; the unit is
built without contraction (a hit's surface point carries the G-buffer's bits); only the raster kernel declares static LDS: the 64 staged
triangles of a tile's list, 56 bytes each; each kernel is held to the register count it compiles to."""
import os

import pytest

from test_kernel_resources import HIPCC, kernel_table, uncontracted_units
from test_refit_resources import named

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# vgpr_count of the code objects' metadata (hipcc -S --cuda-device-only --offload-arch=gfx950 -O3 -ffp-contract=off, ROCm's clang), read off
# this very table when the kernels were written: 50 for the points (three vertices, the hit point, the normal, four bilinear texels in flight),
# 42 / 44 for the count and the fill (three edge functions in 64 bits and the tile walk), and 34 / 44 / 56 for the raster kernel at 1 / 2 / 4
# samples per axis: three 64-bit edge values with their two steps each, and S x S winners.
VGPRS = {"lightmap_points_kernel": 50, "lightmap_setup_kernel": 19, "lightmap_count_kernel": 42, "lightmap_fill_kernel": 44, "lightmap_resolve_kernel": 23,
         "lightmap_gutter_kernel": 37}
RASTER_VGPRS = {1: 34, 2: 44, 4: 56}
RASTER_LDS = 64 * 56


@pytest.fixture(scope="module")
def table():
    return kernel_table("kernels_lightmap.hip")


def clean(t):
    return t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0


def test_the_unit_is_built_without_contraction():
    assert "kernels_lightmap.hip" in uncontracted_units()


@pytest.mark.parametrize("name", sorted(VGPRS))
def test_each_kernel_is_there_once_without_scratch_spills_or_lds_at_its_register_count(table, name):
    hits = named(table, name)
    assert len(hits) == 1, (name, sorted(k for k in table if "evplp" in k))
    t = table[hits[0]]
    assert clean(t), (name, t)
    assert t["group_segment_fixed_size"] == 0, (name, t)
    assert t["vgpr_count"] <= VGPRS[name], (name, t)


def test_the_raster_kernel_is_there_once_per_sample_count_and_alone_declares_lds(table):
    hits = named(table, "lightmap_raster_kernel")
    assert len(hits) == 3, sorted(k for k in table if "evplp" in k)
    for S, bound in RASTER_VGPRS.items():
        mine = [k for k in hits if f"ILi{S}E" in k]
        assert len(mine) == 1, (S, hits)
        t = table[mine[0]]
        assert clean(t), (S, t)
        assert t["group_segment_fixed_size"] == RASTER_LDS, (S, t)
        assert t["vgpr_count"] <= bound, (S, t)
    ours = [k for k in table if "evplp" in k and "lightmap" in k]
    assert len(ours) == len(VGPRS) + 3, ours
