"""No GPU needed: the code object of accel_cost_kernel (evplp_accel_quality).  It lives in bvh_gpu.hip beside the refit's kernels and is held
to zero scratch, no spills and at most 64 VGPRs; its only hand-over is the end of the launch -- nothing in it is atomic and nothing fences --;
and the twelve kernels the unit had are still there."""
import os

import pytest

from test_gather_budget_resources import function_text
from test_kernel_resources import HIPCC, ROOT, kernel_table

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

NEW = "accel_cost_kernel"
OLD = ("tri_setup_kernel", "morton_kernel", "hierarchy_kernel", "refit_kernel", "collapse_kernel", "flag_kernel", "emit_nodes_kernel", "emit_leaves_kernel", "node4_kernel",
       "refit_scatter_kernel", "refit_leaves_kernel", "refit_level_kernel")
SRC = os.path.join(ROOT, "evplp_amd", "csrc", "bvh_gpu.hip")
TYPES = os.path.join(ROOT, "evplp_amd", "csrc", "evplp_types.h")


@pytest.fixture(scope="module")
def table():
    return kernel_table("bvh_gpu.hip")


def named(table, n):
    """the unit's own kernel called n (the mangled name carries its length; hipCUB's kernels are in the table too)"""
    return [k for k in table if f"{len(n)}{n}" in k]


def test_the_cost_kernel_uses_no_scratch_and_spills_nothing(table):
    hits = named(table, NEW)
    assert len(hits) == 1, sorted(table)
    t = table[hits[0]]
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, t
    assert t["vgpr_count"] <= 64, t
    assert t["group_segment_fixed_size"] == 4 * 3 * 8, t                      # lane 0 of four waves, three doubles


def test_the_twelve_existing_kernels_of_the_unit_are_still_there(table):
    assert len(OLD) == 12
    for n in OLD:
        assert len(named(table, n)) == 1, (n, sorted(table))


def test_the_cost_kernel_neither_fences_nor_uses_atomics():
    src = open(SRC).read()
    text = function_text(src, "void " + NEW + "(")
    assert "atomic" not in text and "__threadfence" not in text
    assert text.count("__shfl_down(") == 1 and text.count("__syncthreads()") == 1
    # the terms come from the functions the host reference calls, and those are as plain
    assert text.count("accel_cost_terms(") == 1 and text.count("accel_root_area(") == 1
    types = open(TYPES).read()
    for f in ("void accel_cost_terms(", "double accel_root_area(", "bool cost_box_present("):
        body = function_text(types, f)
        assert "atomic" not in body and "__threadfence" not in body, f
