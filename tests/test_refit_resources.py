"""No GPU needed: the code objects of the refit (evplp_refit_accel).  Its three kernels live in bvh_gpu.hip beside the device builder's and
are held to zero scratch and no spills; the builder's kernels are the ones they were; and the refit hands boxes from one height of the tree
to the next through the end of a kernel launch alone -- nothing in the new kernels is atomic and nothing fences."""
import os

import pytest

from test_gather_budget_resources import function_text
from test_kernel_resources import HIPCC, ROOT, kernel_table

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

NEW = ("refit_scatter_kernel", "refit_leaves_kernel", "refit_level_kernel")
OLD = ("tri_setup_kernel", "morton_kernel", "hierarchy_kernel", "refit_kernel", "collapse_kernel", "flag_kernel", "emit_nodes_kernel", "emit_leaves_kernel", "node4_kernel")
SRC = os.path.join(ROOT, "evplp_amd", "csrc", "bvh_gpu.hip")


@pytest.fixture(scope="module")
def table():
    return kernel_table("bvh_gpu.hip")


def named(table, n):
    """the unit's own kernel called n (the mangled name carries its length; hipCUB's kernels are in the table too)"""
    return [k for k in table if f"{len(n)}{n}" in k]


def test_the_new_kernels_use_no_scratch_and_spill_nothing(table):
    for n in NEW:
        hits = named(table, n)
        assert len(hits) == 1, (n, sorted(table))
        t = table[hits[0]]
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (n, t)
        assert t["group_segment_fixed_size"] == 0 and t["vgpr_count"] <= 64, (n, t)


def test_the_existing_kernels_of_the_unit_are_still_there(table):
    for n in OLD:
        assert len(named(table, n)) == 1, (n, sorted(table))


def test_the_new_kernels_neither_fence_nor_use_atomics():
    src = open(SRC).read()
    for n in NEW + ("store_operands",):
        text = function_text(src, "void " + n + "(")
        assert "atomic" not in text and "__threadfence" not in text and "__syncthreads" not in text, n
    # the operands of a leaf slot are computed in one place, for the builder and for the refit
    assert src.count("e1[1] * e0[2] - e1[2] * e0[1]") == 1
    assert function_text(src, "void emit_leaves_kernel(").count("store_operands(") == 1
    assert function_text(src, "void refit_leaves_kernel(").count("store_operands(") == 1
    # ... and a box is padded in one place
    assert src.count("fabsf(h) * 1e-6f") == 1 and function_text(src, "void refit_level_kernel(").count("set_box(") == 1
