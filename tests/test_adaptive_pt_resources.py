"""No GPU needed: the adaptive variant of the path-tracing kernel is in the code object, exactly once, beside the default, and keeps the
default's code-object properties -- zero scratch, no VGPR spills, at most 128 registers (four waves per SIMD), no more SGPRs parked in VGPR
lanes than the default parks.  The rescale of retired pixels lives inside the variant: there is no kernel of its own for it."""
import os

import pytest

from test_kernel_resources import HIPCC, kernel_table

VARIANT, DEFAULT = "path_trace_kernelILb1E", "path_trace_kernelILb0E"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_adaptive_path_trace_variant_keeps_the_budget():
    table = kernel_table("kernels_pt.hip")
    hits = [k for k in table if VARIANT in k]
    default = [k for k in table if DEFAULT in k]
    assert len(hits) == 1 and len(default) == 1, sorted(table)
    assert sorted(table) == sorted(hits + default), sorted(table)          # one kernel each, and nothing else (no rescale kernel)
    t, d = table[hits[0]], table[default[0]]
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0, t
    assert t["vgpr_count"] <= 128, t
    assert t["sgpr_spill_count"] <= d["sgpr_spill_count"], (t, d)
