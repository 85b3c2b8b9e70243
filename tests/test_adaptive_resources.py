"""No GPU needed: the adaptive variants of the gather kernels (VPL gather, VSL walk and estimators, reduce), of the cut kernel and of the
noise kernels, and the retirement kernel, keep the code-object properties of the defaults they stand beside -- zero scratch, no VGPR spills,
no more SGPRs parked in VGPR lanes than the default variant parks (the walks park some by design), and the walks within 64 registers (eight
waves per SIMD)."""
import os

import pytest

from test_kernel_resources import HIPCC, kernel_table


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src, kinds, budgets", [
    ("kernels_gather.hip", ["gather_vpl_kernelILb1ELb0ELb1E", "gather_vpl_kernelILb0ELb0ELb1E", "gather_vsl_walk_kernelILb1ELb0ELb1E",
                            "gather_vsl_walk_kernelILb0ELb0ELb1E", "gather_vsl_shade_kernelILb0ELb1E", "gather_reduce_kernelILb1E"],
     {"gather_vpl_kernelILb1ELb0ELb1E": 64, "gather_vpl_kernelILb0ELb0ELb1E": 64, "gather_vsl_walk_kernelILb1ELb0ELb1E": 64,
      "gather_vsl_walk_kernelILb0ELb0ELb1E": 64, "gather_vsl_shade_kernelILb0ELb1E": 128}),
    ("kernels_cut.hip", ["gather_cut_kernelILb1E"], {"gather_cut_kernelILb1E": 64}),
    ("kernels_stats.hip", ["noise_fold_frozen_kernel", "noise_rows_frozen_kernel", "noise_variance_frozen_kernel", "adaptive_retire_kernel"], {}),
])
def test_adaptive_variants_keep_their_budgets(src, kinds, budgets):
    table = kernel_table(src)
    for want in kinds:
        hits = [k for k in table if want in k]
        assert len(hits) == 1, (want, sorted(table))
        t = table[hits[0]]
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0, (hits[0], t)
        # the default it stands beside: the same name with the last template argument false (none: a kernel of its own, held to zero)
        default = [k for k in table if want.endswith("1E") and want[:-2] + "0E" in k]
        limit = table[default[0]]["sgpr_spill_count"] if default else 0
        assert t["sgpr_spill_count"] <= limit, (hits[0], t, default)
    for want, limit in budgets.items():
        for k in [k for k in table if want in k]:
            assert table[k]["vgpr_count"] <= limit, (k, table[k])
