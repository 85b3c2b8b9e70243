"""EVPLP_PARTITION_ITERATIONS without a GPU: the additive ABI (enum value, two entry points, their argument checks) and the code object of
the reduction that sums the ranks' accumulators (zero scratch: it is an HBM-bound stream and must stay one)."""
import ctypes as C
import os
import subprocess

import pytest

from test_kernel_resources import HIPCC, kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_partition_values_without_bands_in_header_and_binding(evplp, tmp_path):
    src = tmp_path / "partition.c"
    src.write_text('''#include <stdio.h>
#include "evplp.h"
int main(void) {
    evplp_group_partition p = EVPLP_PARTITION_ITERATIONS;
    printf("%d %d\\n", (int)EVPLP_PARTITION_STRIPS, (int)p);
    return 0;
}
''')
    exe = tmp_path / "partition"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [evplp.PARTITION_STRIPS, evplp.PARTITION_ITERATIONS] == [0, 2]
    assert evplp.PARTITIONS["iterations"] == 2


def test_new_entry_points_are_exported_and_refuse_a_null_group(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    for name in ("evplp_group_select_rank", "evplp_group_synchronize_rank"):
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
    assert evplp.lib().evplp_group_select_rank(None, 0) == evplp.ERR_INVALID
    assert evplp.lib().evplp_group_synchronize_rank(None, 0) == evplp.ERR_INVALID


def test_unknown_partition_name_is_refused_before_any_device_call(evplp):
    with pytest.raises(ValueError):
        evplp.Group(16, 16, 4, 4, 2, 2, devices=[0, 0], partition="rows")
    with pytest.raises(ValueError):
        evplp.Group(16, 16, 4, 4, 2, 2, devices=[0, 0], partition="bands")      # (removed in ABI version 5)
    cfg, gc, h = evplp.Config(), evplp.GroupConfig(), C.c_void_p()
    cfg.abi_version = evplp.ABI_VERSION; cfg.res_x = cfg.res_y = 16; cfg.num_light_paths = cfg.num_vpl_light_paths = 4; cfg.photons_per_path = 2
    gc.n_ranks = 2; gc.partition = 1
    assert evplp.lib().evplp_group_create(C.byref(cfg), C.cast(C.byref(gc), C.c_void_p), C.byref(h)) == evplp.ERR_INVALID and not h.value
    assert b"partition 1 unknown" in evplp.lib().evplp_group_last_error(None)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_reduce_shards_kernel_has_no_scratch_and_no_spills():
    table = kernel_table("kernels_splat.hip")
    hits = [k for k in table if "reduce_shards_kernel" in k]
    assert len(hits) == 2, sorted(table)            # the sum and the first-non-zero variant
    for k in hits:
        t = table[k]
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (k, t)
