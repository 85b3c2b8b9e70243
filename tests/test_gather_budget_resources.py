"""No GPU needed: the code objects of gather budget mode (evplp_adaptive_enable(ctx, 2)).  Its three kernels live in kernels_gather.hip -- the
per-call mask, the mode's reduce and the n_t step -- and are held to zero scratch and no spills; the reduce shares the balanced tree
(reduce_tree) and the counter shards (reduce_counters) with gather_reduce_kernel as functions, so the existing reduce kernels stay two and
keep their names."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, ROOT, kernel_table

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

NEW = ("gather_budget_mask_kernel", "gather_reduce_budget_kernel", "gather_budget_step_kernel")


@pytest.fixture(scope="module")
def table():
    return kernel_table("kernels_gather.hip")


def test_the_new_kernels_keep_their_budgets(table):
    for n in NEW:
        hits = [k for k in table if n in k]
        assert len(hits) == 1, (n, sorted(table))
        t = table[hits[0]]
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (n, t)
    # the reduce's tree needs the plain reduce's registers, not more than a 256-thread workgroup gets at full occupancy
    assert table[[k for k in table if "gather_reduce_budget_kernel" in k][0]]["vgpr_count"] <= 64


def test_the_existing_gather_kernels_are_the_ones_they_were(table):
    """no template parameter added or changed: 18 kernels before, the same 18 names now, plus the three"""
    old = [k for k in table if not any(n in k for n in NEW)]
    assert len(old) == 18 and len(table) == 21, sorted(table)
    assert sorted(k for k in old if "gather_reduce_kernel" in k) == sorted(
        ["_ZN5evplp20gather_reduce_kernelILb0EEEvNS_10GatherArgsEiNS_9AdaptArgsE", "_ZN5evplp20gather_reduce_kernelILb1EEEvNS_10GatherArgsEiNS_9AdaptArgsE"])


def function_text(src, head):
    """the text of the function whose definition starts with `head`, up to its closing brace in column 0"""
    k = src[src.index(head):]
    return k[:k.index("\n}\n")]


def test_the_tree_and_the_counters_are_shared_functions_and_nothing_new_is_atomic():
    csrc = os.path.join(ROOT, "evplp_amd", "csrc")
    assert not os.path.exists(os.path.join(csrc, "reduce_tree_body.hpp"))
    src = open(os.path.join(csrc, "kernels_gather.hip")).read()
    assert src.count("#define EV_MERGE") == 1                             # the tree's text lives in one place
    # the reduce's existing counter shards and nothing else: two LDS adds per wave, two global adds per workgroup
    assert len(re.findall(r"\batomic\w*\(", function_text(src, "EV_DEV void reduce_counters("))) == 4
    for n in ("void gather_reduce_kernel(", "void gather_reduce_budget_kernel("):
        k = function_text(src, n)
        assert k.count("reduce_tree(") == 1 and k.count("reduce_counters(") == 1, n
        assert "atomic" not in k, n
    for n in ("gather_budget_mask_kernel", "gather_budget_step_kernel"):
        assert "atomic" not in function_text(src, "void " + n + "("), n
