"""No GPU needed: the code objects of gather budget mode (evplp_adaptive_enable(ctx, 2)).  Its three kernels live in kernels_gather.hip -- the
per-call mask, the mode's reduce and the n_t step -- and are held to zero scratch and no spills; the reduce shares the balanced tree with
gather_reduce_kernel as text (reduce_tree_body.hpp), so the existing reduce kernels stay two and keep their names."""
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


def test_the_tree_is_shared_as_text_and_nothing_new_is_atomic():
    src = open(os.path.join(ROOT, "evplp_amd", "csrc", "kernels_gather.hip")).read()
    assert src.count('#include "reduce_tree_body.hpp"') == 2              # gather_reduce_kernel and gather_reduce_budget_kernel
    assert "EV_MERGE" not in src                                          # the tree's text lives in one place
    body = src[src.index("void gather_reduce_budget_kernel("):src.index("light-subpath windows")]
    # the reduce's existing counter shards and nothing else: two LDS adds per wave, two global adds per workgroup
    assert len(re.findall(r"\batomic\w*\(", body)) == 4
    for n in ("gather_budget_mask_kernel", "gather_budget_step_kernel"):
        k = src[src.index("void " + n + "("):]
        assert "atomic" not in k[:k.index("\n}\n")], n
