"""No GPU needed: the three kernels of the temporal accumulation have zero scratch and no spills, and the previous-pose walk -- the primary
walk without its material fetch -- needs no more registers than primary_kernel in the same build."""
import os

import pytest

from test_kernel_resources import HIPCC, kernel_table


def _one(table, want):
    hits = [k for k in table if want in k]
    assert len(hits) == 1, (want, sorted(table))
    return hits[0], table[hits[0]]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_temporal_kernels_have_no_scratch_and_no_spills_and_the_walk_fits_the_primary_budget():
    table = kernel_table("kernels_temporal.hip")
    for want in ("temporal_accumulate_kernel", "pose_snapshot_kernel", "prev_pose_kernel"):
        name, t = _one(table, want)
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (name, t)
    _, walk = _one(table, "prev_pose_kernel")
    _, primary = _one(kernel_table("kernels_trace.hip"), "primary_kernel")
    print(f"\nvgprs: prev_pose_kernel {walk['vgpr_count']}, primary_kernel {primary['vgpr_count']}")
    assert walk["vgpr_count"] <= primary["vgpr_count"], (walk, primary)
