"""No GPU needed: the code objects of the PLOC builder's kernels (EVPLP_BVH_PLOC_GPU).  They live in bvh_gpu.hip beside the radix-tree builder's
and the refit's: zero scratch, no spills, the nearest-neighbour kernel's staged window in exactly 7 680 bytes of LDS and no LDS in the others,
and nothing in their text that is atomic or fences -- an iteration's steps hand over at the end of a launch alone."""
import os
import re

import pytest

from test_gather_budget_resources import function_text
from test_kernel_resources import HIPCC, ROOT, kernel_table

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# search, merge flags, compaction + nodes, placement, and the launch that makes the first clusters
PLOC = ("ploc_nn_kernel", "ploc_merge_kernel", "ploc_scatter_kernel", "ploc_place_kernel", "ploc_init_kernel")
OLD = ("tri_setup_kernel", "morton_kernel", "hierarchy_kernel", "refit_kernel", "collapse_kernel", "flag_kernel", "emit_nodes_kernel", "emit_leaves_kernel", "node4_kernel",
       "refit_scatter_kernel", "refit_leaves_kernel", "refit_level_kernel", "accel_cost_kernel")
SRC = os.path.join(ROOT, "evplp_amd", "csrc", "bvh_gpu.hip")
NN_LDS = (256 + 2 * 32) * 24


@pytest.fixture(scope="module")
def table():
    return kernel_table("bvh_gpu.hip")


def named(table, n):
    return [k for k in table if f"{len(n)}{n}" in k]


def test_the_ploc_kernels_use_no_scratch_spill_nothing_and_only_the_search_uses_lds(table):
    assert NN_LDS == 7680
    for n in PLOC:
        hits = named(table, n)
        assert len(hits) == 1, (n, sorted(table))
        t = table[hits[0]]
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (n, t)
        assert t["group_segment_fixed_size"] == (NN_LDS if n == "ploc_nn_kernel" else 0), (n, t)
        assert t["vgpr_count"] <= 64, (n, t)


def test_the_existing_kernels_of_the_unit_are_still_there_one_each(table):
    for n in OLD:
        assert len(named(table, n)) == 1, (n, sorted(table))


def test_the_ploc_kernels_neither_fence_nor_use_atomics():
    src = open(SRC).read()
    for n in PLOC:
        text = function_text(src, "void " + n + "(")
        assert "atomic" not in text and "__threadfence" not in text, n
        assert ("__syncthreads" in text) == (n == "ploc_nn_kernel"), n
    nn = function_text(src, "void ploc_nn_kernel(")
    assert nn.count("__syncthreads()") == 1 and "#pragma clang fp contract(off)" in nn and nn.count("ploc_distance(") == 1
    # the distance is stated once, for the kernel and for the host twin
    types = open(os.path.join(ROOT, "evplp_amd", "csrc", "evplp_types.h")).read()
    assert len(re.findall(r"inline float ploc_distance\(", types)) == 1 and "#pragma clang fp contract(off)" in function_text(types, "inline float ploc_distance(")
    assert open(os.path.join(ROOT, "evplp_amd", "csrc", "host", "ploc.cpp")).read().count("ploc_distance(") == 1
