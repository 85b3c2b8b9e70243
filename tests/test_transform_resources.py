"""No GPU needed: the code object of refit_transform_kernel (evplp_transform_mesh + evplp_refit_accel).  It lives in bvh_gpu.hip beside the
refit's other kernels, is launched once per refit whatever moved, and is held to zero scratch, no spills, no LDS; it neither fences nor
uses atomics; and transform_point is the only arithmetic it does on positions -- the function the host copy of a mesh goes through."""
import os
import re

import pytest

from test_gather_budget_resources import function_text
from test_kernel_resources import HIPCC, ROOT
from test_refit_resources import NEW, OLD, named, table  # noqa: F401  (table: the module's fixture, compiled once per module here)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

CSRC = os.path.join(ROOT, "evplp_amd", "csrc")
SRC = os.path.join(CSRC, "bvh_gpu.hip")


def test_the_kernel_is_there_once_and_uses_no_scratch_no_lds_and_spills_nothing(table):
    for n in ("refit_transform_kernel", "refit_rest_kernel"):
        hits = named(table, n)
        assert len(hits) == 1, (n, sorted(table))
        t = table[hits[0]]
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (n, t)
        assert t["group_segment_fixed_size"] == 0 and t["vgpr_count"] <= 64, (n, t)


def test_the_kernels_of_the_unit_are_still_there(table):
    for n in OLD + NEW:
        assert len(named(table, n)) == 1, (n, sorted(table))


def test_it_neither_fences_nor_uses_atomics_and_transform_point_is_its_only_arithmetic_on_positions():
    src = open(SRC).read()
    for n in ("refit_transform_kernel", "refit_rest_kernel"):
        text = function_text(src, "void " + n + "(")
        assert "atomic" not in text and "__threadfence" not in text and "__syncthreads" not in text and "__shared__" not in text, n
    text = function_text(src, "void refit_transform_kernel(")
    body = text[text.index("{"):]
    assert body.count("transform_point(") == 1
    # what else the body computes is integers: no float is declared, no fused operation is spelt, and the attributes are written by the call alone
    assert not re.search(r"\bfloat\b|fmaf?\(|__fm", body), body
    assert len(re.findall(r"attrs\[", body)) == 1 and "rest[" not in body
    # one launch per refit: the host launches it from one place, outside the loop over the meshes
    assert src.count("hipLaunchKernelGGL(refit_transform_kernel") == 1
    ctx, motion = open(os.path.join(CSRC, "context.cpp")).read(), open(os.path.join(CSRC, "scene_motion.cpp")).read()
    refit = function_text(motion, "static int refit_deform(")          # evplp_refit_accel's stage of the three deformer launches
    assert (motion + ctx).count("refit_transform(") == 1 and refit.count("refit_transform(") == 1
    assert re.search(r"\n    if \(nx\) \{\n[^\n]*\n        refit_transform\(", refit), "the launch sits at the function's own level, behind the loop over the meshes"
    # the function itself: stated once, uncontracted, without a fused operation
    types = open(os.path.join(CSRC, "evplp_types.h")).read()
    assert types.count("inline void transform_point(") == 1
    fn = types[types.index("inline void transform_point("):]
    fn = fn[:fn.index("\n}\n")]
    assert "#pragma clang fp contract(off)" in fn and "fma" not in fn
    # ... and the host moves its copy through it, nowhere else is a matrix applied
    assert motion.count("transform_point(") == 3 and ctx.count("transform_point(") == 0       # evplp_transform_points, evplp_transform_mesh, its finiteness check
