"""No GPU needed: the code objects hipcc produces for gfx950 must keep the properties the design relies on -- zero scratch in every
gather / cut / splat / path-tracing kernel (a count-indexed local array in the cut kernel once put 20 bytes per lane into scratch and cost
30 % of its time) and the register budgets that give the walks their eight waves per SIMD (64 registers: the pixel's reflectances wait in LDS)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-fno-slp-vectorize", "-S", "--cuda-device-only", "-w"]


def uncontracted_units():
    """the units the Makefile builds with -ffp-contract=off: its `$(BUILD)/X.o: HIPFLAGS += -ffp-contract=off ...` lines"""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    return [x + ".hip" for x in re.findall(r"^\$\(BUILD\)/(\w+)\.o: HIPFLAGS \+= -ffp-contract=off\b", mk, re.M)]


def kernel_table(src):
    extra = ["-ffp-contract=off"] if src in uncontracted_units() else []      # (as the Makefile builds it)
    out = subprocess.run([HIPCC] + FLAGS + extra + ["-o", "-", os.path.join(ROOT, "evplp_amd", "csrc", src)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    table, cur = {}, {}
    for line in out.stdout.splitlines():
        m = re.match(r"\s+\.(name|private_segment_fixed_size|vgpr_count|vgpr_spill_count|sgpr_spill_count|group_segment_fixed_size):\s+(\S+)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1) == "vgpr_spill_count":      # the last of the fields of one kernel's metadata block
            table[cur.get("name", "?")] = {k: int(v) for k, v in cur.items() if k != "name"}
            cur = {}
    return table


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src, zero_scratch, budgets", [
    # (second template argument Lb0: the product kernels; Lb1 = the self-clocking calibration variants, evplp_calibrate_blocks, run for one frame
    # before a deal by cost -- held to their register budgets, not to zero scratch: the VPL one parks its start clock in 8 bytes of it)
    ("kernels_gather.hip", ["gather_vpl_kernelILb1ELb0", "gather_vpl_kernelILb0ELb0", "gather_vsl_walk_kernelILb1ELb0", "gather_vsl_walk_kernelILb0ELb0", "gather_vsl_shade_kernelILb0", "gather_reduce_kernel"],
     {"gather_vpl_kernelILb1": 64, "gather_vpl_kernelILb0": 64, "gather_vsl_walk_kernelILb1": 64, "gather_vsl_walk_kernelILb0": 64, "gather_vsl_shade_kernel": 128}),
    ("kernels_cut.hip", ["gather_cut_kernel", "primary_cut_kernel"], {"gather_cut_kernel": 64}),
    # (the proxy-footprint variants of the tile kernel, ILb1, are held to seven / six waves per SIMD below)
    # (ILi0E: the MIXED launch -- heavy tiles with four waves, the others with one; its proxy variant runs at six waves like the four-wave one)
    ("kernels_splat.hip", ["splat_bin_kernel", "splat_scatter_kernel", "splat_heavy_kernel", "splat_tiles_kernelILi1ELb0", "splat_tiles_kernelILi4ELb0", "splat_tiles_kernelILi0ELb0",
                           "splat_tiles_kernelILi4ELb1", "splat_tiles_kernelILi0ELb1", "resolve_kernel"],
     {"splat_tiles_kernelILi1ELb0": 64, "splat_tiles_kernelILi4ELb0": 64, "splat_tiles_kernelILi0ELb0": 64, "splat_tiles_kernelILi1ELb1": 72, "splat_tiles_kernelILi4ELb1": 80,
      "splat_tiles_kernelILi0ELb1": 80}),
    ("kernels_pt.hip", ["path_trace_kernel"], {}),
    ("kernels_trace.hip", ["light_trace_kernel", "primary_kernel"], {"light_trace_kernel": 128, "primary_kernel": 64}),
])
def test_code_objects_keep_their_budgets(src, zero_scratch, budgets):
    table = kernel_table(src)
    for want in zero_scratch:
        hits = [k for k in table if want in k]
        assert hits, (want, sorted(table))
        for k in hits:
            assert table[k]["private_segment_fixed_size"] == 0 and table[k]["vgpr_spill_count"] == 0, (k, table[k])
    for want, limit in budgets.items():
        for k in [k for k in table if want in k]:
            assert table[k]["vgpr_count"] <= limit, (k, table[k])
    if src == "kernels_splat.hip":
        # splat_tiles_kernel<1, true> at seven waves per SIMD (72 registers; it wants 78): two values wait in scratch -- the pixel's address
        # for the final store (written before the batch loop, read after it) and one 16-byte value re-read once per 64-photon batch;
        # none inside the radius-test, slab or shading loops (measured: seven waves with these beat six without, 96.6 vs 102 us at config #4)
        for k in [k for k in table if "splat_tiles_kernelILi1ELb1" in k]:
            assert table[k]["private_segment_fixed_size"] <= 32 and table[k]["vgpr_spill_count"] <= 8, (k, table[k])
