"""No GPU needed: the code objects of the batched path tracer (evplp_path_trace_batch), one item-table pipeline for adaptivity off, mode 1 and
budget mode.  Its kernels live in three translation units -- kernels_ptbatch_primary.hip, built like kernels_trace.hip with -ffp-contract=off for
the whole unit (the batched primary, nothing else), kernels_stats.hip, built likewise (budget mode's per-tile fold and per-tile noise figure,
beside the other statistics kernels), and kernels_ptbatch.hip with the path tracer's default flags (the item table, the trace, the
accumulation, the closing kernel) -- and are held to zero scratch, no VGPR spills, 64 registers for the batched primary (eight waves per SIMD,
as primary_kernel) and 128 for the batched trace (four, as path_trace_kernel).  kernels_pt.hip, kernels_trace.hip and kernels_stats.hip keep
exactly their kernels.  tests/test_pt_batch_same_arithmetic.py holds the trace to path_trace_kernel's operand shapes."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, ROOT, kernel_table

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

BUDGET_STATS = ("noise_fold_budget_kernel", "tile_noise_kernel")
TABLE_UNIT = ("pt_batch_scan_kernel", "pt_batch_fill_kernel", "pt_batch_trace_kernel", "pt_batch_accumulate_kernel", "pt_batch_close_kernel")


def only(table, want):
    hits = [k for k in table if want in k]
    assert len(hits) == 1, (want, sorted(table))
    return table[hits[0]]


def test_the_makefile_builds_the_batched_primary_without_contraction():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(BUILD\)/kernels_ptbatch_primary\.o: HIPFLAGS \+= -ffp-contract=off\s*$", mk, re.M)
    assert re.search(r"^\$\(BUILD\)/kernels_stats\.o: HIPFLAGS \+= -ffp-contract=off\s*$", mk, re.M)
    assert not re.search(r"^\$\(BUILD\)/kernels_ptbatch\.o:.*-ffp-contract=off", mk, re.M)       # the trace keeps path_trace_kernel's flags
    for src in ("kernels_ptbatch.hip", "kernels_ptbatch_primary.hip", "kernels_stats.hip"):
        assert "$(CSRC)/" + src in mk, src


def test_batched_primary_keeps_the_budget():
    """the unit without contraction: the batched primary, nothing else"""
    table = kernel_table("kernels_ptbatch_primary.hip")
    assert len(table) == 1, sorted(table)
    t = only(table, "pt_batch_primary_kernel")
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0, t
    assert t["vgpr_count"] <= 64, t


def test_budget_fold_and_tile_noise_keep_their_budgets():
    table = kernel_table("kernels_stats.hip")
    for n in BUDGET_STATS:
        t = only(table, n)
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0, (n, t)


def test_batched_table_accumulate_and_close_keep_their_budgets():
    table = kernel_table("kernels_ptbatch.hip")
    assert len(table) == len(TABLE_UNIT), sorted(table)
    for n in TABLE_UNIT:
        if n != "pt_batch_trace_kernel":
            t = only(table, n)
            assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0, (n, t)
    assert only(table, "pt_batch_scan_kernel")["group_segment_fixed_size"] <= 128              # (the scan's wave totals: no atomics, no big LDS)


def test_batched_trace_keeps_its_budget():
    t = only(kernel_table("kernels_ptbatch.hip"), "pt_batch_trace_kernel")
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0, t
    assert t["vgpr_count"] <= 128, t


def test_the_batched_kernels_use_no_atomics_but_the_pass_counters():
    """Nothing that reaches an image or a noise figure goes through an atomic: the only ones are the trace's rays and paths, one per wave."""
    for src, want in (("kernels_ptbatch.hip", 2), ("kernels_ptbatch_primary.hip", 0), ("kernels_stats.hip", 0)):
        text = open(os.path.join(ROOT, "evplp_amd", "csrc", src)).read()
        assert len(re.findall(r"\batomic\w*\(", text)) == want, src


def test_the_existing_units_keep_exactly_their_kernels():
    pt = kernel_table("kernels_pt.hip")
    assert len(pt) == 2 and all("path_trace_kernelILb" in k for k in pt), sorted(pt)
    trace = kernel_table("kernels_trace.hip")
    assert len(trace) == 3 and all(sum(1 for k in trace if re.search(r"\d" + n, k)) == 1 for n in ("primary_kernel", "light_trace_kernel", "compact_vpl_kernel")), sorted(trace)
    stats = kernel_table("kernels_stats.hip")
    want = ["frame_error_kernel", "noise_fold_frozen_kernel", "noise_pool_kernel", "noise_rows_kernel", "noise_rows_frozen_kernel", "noise_variance_kernel",
            "noise_variance_frozen_kernel", "adaptive_retire_kernel", "noise_fold_kernelILb1E", "noise_fold_kernelILb0E", "noise_fold_budget_kernel", "tile_noise_kernel"]
    assert len(stats) == len(want), sorted(stats)
    for n in want:
        assert sum(1 for k in stats if re.search(r"\d" + n, k)) == 1, (n, sorted(stats))
    assert not [k for k in list(pt) + list(trace) + list(stats) if "pt_batch" in k]
    p, lt = only(trace, "14primary_kernel"), only(trace, "light_trace_kernel")
    assert p["private_segment_fixed_size"] == 0 and p["vgpr_spill_count"] == 0 and p["vgpr_count"] <= 64, p
    assert lt["private_segment_fixed_size"] == 0 and lt["vgpr_spill_count"] == 0 and lt["vgpr_count"] <= 128, lt
