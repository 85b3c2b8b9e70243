"""No GPU needed: the code objects of the path tracer's budget mode (evplp_adaptive_enable_pt(ctx, 2)).  Its kernels live in two translation
units of their own -- kernels_ptbudget_exact.hip, built like kernels_trace.hip with -ffp-contract=off for the whole unit (the batched primary
of the mode, the per-tile fold, the per-tile noise figure), and kernels_ptbudget.hip with the path tracer's default flags (the item table, the
trace, the accumulation into the raw sums) -- so kernels_ptbatch*.hip, kernels_pt.hip and kernels_trace.hip keep exactly their kernels
(tests/test_pt_batch_resources.py).  Every kernel is held to zero scratch and no spills, the primary to 64 registers and the trace to 128, and
the trace to path_trace_kernel's operand shapes, as tests/test_pt_batch_same_arithmetic.py holds pt_batch_trace_kernel."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, ROOT
from test_pt_batch_resources import only, table_of
from test_pt_batch_same_arithmetic import body_of, optimised_ir, shapes

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_the_makefile_builds_the_exact_unit_without_contraction():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert re.search(r"^\$\(BUILD\)/kernels_ptbudget_exact\.o: HIPFLAGS \+= -ffp-contract=off\s*$", mk, re.M)
    assert not re.search(r"^\$\(BUILD\)/kernels_ptbudget\.o:.*-ffp-contract=off", mk, re.M)       # the trace keeps path_trace_kernel's flags
    for src in ("kernels_ptbudget.hip", "kernels_ptbudget_exact.hip"):
        assert "$(CSRC)/" + src in mk, src


def test_budget_primary_fold_and_tile_noise_keep_their_budgets():
    table = table_of("kernels_ptbudget_exact.hip", ["-ffp-contract=off"])
    names = ("pt_budget_primary_kernel", "noise_fold_budget_kernel", "tile_noise_kernel")
    assert len(table) == len(names), sorted(table)
    for n in names:
        t = only(table, n)
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0, (n, t)
    assert only(table, "pt_budget_primary_kernel")["vgpr_count"] <= 64


def test_budget_table_trace_accumulate_and_finish_keep_their_budgets():
    table = table_of("kernels_ptbudget.hip")
    names = ("pt_budget_scan_kernel", "pt_budget_fill_kernel", "pt_budget_trace_kernel", "pt_budget_accumulate_kernel", "pt_budget_finish_kernel")
    assert len(table) == len(names), sorted(table)
    for n in names:
        t = only(table, n)
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0, (n, t)
    assert only(table, "pt_budget_trace_kernel")["vgpr_count"] <= 128
    assert only(table, "pt_budget_scan_kernel")["group_segment_fixed_size"] <= 128             # (the scan's wave totals: no atomics, no big LDS)


def test_the_budget_kernels_use_no_atomics_but_the_pass_counters():
    """Nothing that reaches an image or a noise figure goes through an atomic: the only ones are the trace's rays and paths, one per wave."""
    for src, want in (("kernels_ptbudget.hip", 2), ("kernels_ptbudget_exact.hip", 0)):
        text = open(os.path.join(ROOT, "evplp_amd", "csrc", src)).read()
        assert len(re.findall(r"\batomic\w*\(", text)) == want, src


def test_the_budget_trace_contracts_as_path_trace_kernel_does():
    pt = shapes(body_of(optimised_ir("kernels_pt.hip"), "path_trace_kernelILb0E"))
    budget = shapes(body_of(optimised_ir("kernels_ptbudget.hip"), "pt_budget_trace_kernel"))
    fused = sum(1 for s in pt if s.startswith(("fadd contract", "fsub contract")) and "fmul=" in s)
    print(f"{len(pt)} floating-point operations in path_trace_kernel, {len(budget)} in pt_budget_trace_kernel; {fused} adds with a product to fuse")
    assert len(pt) > 1000 and fused > 100
    differ = [(i, a, b) for i, (a, b) in enumerate(zip(pt, budget)) if a != b]
    assert len(pt) == len(budget) and not differ, (len(pt), len(budget), differ[:6])
