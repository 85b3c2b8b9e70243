"""No GPU needed: the code object of refit_rotate_level_kernel (evplp_optimize_accel, evplp_set_refit_rotations).  It lives in bvh_gpu.hip
beside refit_level_kernel, whose work it does with the rotation rule on top, and is held to zero scratch, no spills, no LDS and 128 VGPRs
(the compiler gives it 90: the exact boxes of two children and four grandchildren are live across the rule, 36 floats, beside the node's own
64 bytes).  The end of a launch is its only hand-over: nothing in it is atomic, nothing fences, nothing is shared.  The kernels the unit had
are still there, and the plain refit's kernel is still the only one evplp_refit_accel launches by default."""
import os
import re

import pytest

from test_gather_budget_resources import function_text
from test_kernel_resources import HIPCC, ROOT
from test_refit_resources import NEW as REFIT, OLD, named, table  # noqa: F401  (table: the module's fixture, compiled once per module here)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

CSRC = os.path.join(ROOT, "evplp_amd", "csrc")
SRC = os.path.join(CSRC, "bvh_gpu.hip")
KERNEL = "refit_rotate_level_kernel"
VGPR_BUDGET = 128


def test_the_kernel_is_there_once_and_uses_no_scratch_no_lds_and_spills_nothing(table):
    hits = named(table, KERNEL)
    assert len(hits) == 1, sorted(table)
    t = table[hits[0]]
    print(f"{KERNEL}: {t}")
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, t
    assert t["group_segment_fixed_size"] == 0 and t["vgpr_count"] <= VGPR_BUDGET, t
    # its name does not shadow the plain kernel's in the tests that look kernels up by a length-prefixed name
    assert len(named(table, "refit_level_kernel")) == 1


def test_the_kernels_of_the_unit_are_still_there(table):
    for n in OLD + REFIT + ("refit_transform_kernel", "refit_rest_kernel", "accel_cost_kernel", "ploc_nn_kernel", "ploc_merge_kernel", "ploc_scatter_kernel", "ploc_place_kernel"):
        assert len(named(table, n)) == 1, (n, sorted(table))


def test_it_neither_fences_nor_uses_atomics_and_calls_the_shared_functions():
    src = open(SRC).read()
    for n in ("void " + KERNEL + "(", "void rotate_ref_box(", "void rotate_set_box(", "void rotate_kids("):
        text = function_text(src, n)
        assert "atomic" not in text and "__threadfence" not in text and "__syncthreads" not in text and "__shared__" not in text, n
    text = function_text(src, "void " + KERNEL + "(")
    assert text.count("rotate_choice(") == 1 and text.count("rotate_need(") == 2 and "ploc_distance" not in text
    # boxes are padded by the one set_box, leaf boxes use the one tri_has_area
    assert src.count("fabsf(h) * 1e-6f") == 1 and function_text(src, "void rotate_set_box(").count("set_box(") == 2      # (its own name and the call)
    assert function_text(src, "void rotate_ref_box(").count("tri_has_area(") == 1
    types = open(os.path.join(CSRC, "evplp_types.h")).read()
    for f in ("inline int rotate_choice(", "inline void rotate_union(", "inline int32_t rotate_need(", "inline bool rotate_box_empty("):
        assert types.count(f) == 1, f
        body = function_text(types, f)
        assert "atomic" not in body and "__threadfence" not in body and not re.search(r"\bfmaf?\(|__fm", body), f
    # the plain refit is untouched: its kernel is launched from one place, the rotating one from another, and only when asked
    assert src.count("hipLaunchKernelGGL(refit_level_kernel") == 1 and src.count("hipLaunchKernelGGL(" + KERNEL) == 1
    refit = function_text(open(os.path.join(CSRC, "scene_motion.cpp")).read(), "static int refit_tree(")       # evplp_refit_accel's tree stage
    assert re.search(r"if \(rot > 0\) rotate_enqueue\(", refit) and re.search(r"else for \(int32_t l = 0; l < c->refit_levels; l\+\+\)\n\s+refit_level\(", refit)
    assert "rotate_passes = 0" in open(os.path.join(CSRC, "context.hpp")).read()
