"""No GPU needed: the three kernels of the denoiser (prepare, a-trous level, finish) have zero scratch and no VGPR spills."""
import os

import pytest

from test_kernel_resources import HIPCC, kernel_table


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_denoise_kernels_have_no_scratch_and_no_spills():
    table = kernel_table("kernels_denoise.hip")
    for want in ("denoise_prepare_kernel", "denoise_level_kernel", "denoise_finish_kernel"):
        hits = [k for k in table if want in k]
        assert len(hits) == 1, (want, sorted(table))
        t = table[hits[0]]
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (hits[0], t)
