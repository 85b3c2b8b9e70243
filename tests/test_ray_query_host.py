"""Ray queries without a GPU: the seven entry points of evplp_trace_closest / evplp_trace_occluded (exported, bound, declared, refusing null
handles; the ABI version unchanged), the two structs' sizes against the header, the chunk constant stated once, and where the code lives."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evplp_amd", "csrc")
NEW = ("evplp_trace_closest", "evplp_trace_occluded", "evplp_trace_closest_device", "evplp_trace_occluded_device", "evplp_triangle_info",
       "evplp_group_trace_closest", "evplp_group_trace_occluded")


def test_new_entry_points_are_exported_bound_declared_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    rays = np.zeros((1, 8), np.float32)
    hits = np.zeros(1, evplp.HIT_DTYPE)
    out = np.zeros(1, np.uint8)
    m, i = C.c_int32(), C.c_int32()
    assert L.evplp_trace_closest(None, rays.ctypes.data, 1, 0, 0, hits.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_trace_occluded(None, rays.ctypes.data, 1, 0, out.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_trace_closest_device(None, None, 0, 0, 0, None) == evplp.ERR_INVALID
    assert L.evplp_trace_occluded_device(None, None, 0, 0, None) == evplp.ERR_INVALID
    assert L.evplp_triangle_info(None, 0, C.byref(m), C.byref(i)) == evplp.ERR_INVALID
    assert L.evplp_group_trace_closest(None, rays.ctypes.data, 1, 0, 0, hits.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_group_trace_occluded(None, rays.ctypes.data, 1, 0, out.ctypes.data) == evplp.ERR_INVALID
    assert hits["triangle"][0] == 0 and out[0] == 0, "a refused call writes nothing"
    assert L.evplp_abi_version() == 5
    assert "#define EVPLP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", hdr)
    for meth in ("trace_closest", "trace_occluded"):
        assert callable(getattr(evplp.Context, meth)) and callable(getattr(evplp.Group, meth)), meth
    assert callable(evplp.Context.triangle_info)


def test_the_structs_and_the_constants_match_the_header(evplp, tmp_path):
    assert evplp.HIT_DTYPE.itemsize == 16 and evplp.HIT_DTYPE.names == ("t", "beta", "gamma", "triangle")
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "evplp.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(evplp_ray), sizeof(evplp_hit), '
                   'offsetof(evplp_ray, tmin), offsetof(evplp_ray, direction), offsetof(evplp_ray, tmax), offsetof(evplp_hit, triangle), EVPLP_QUERY_CHUNK_RAYS, EVPLP_QUERY_ORDER); return 0; }\n')
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    assert got == [32, 16, 12, 16, 28, 12, evplp.QUERY_CHUNK_RAYS, evplp.QUERY_ORDER]
    # the chunk is stated once, in the header; the library's units take it from there
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    assert len(re.findall(r"#define EVPLP_QUERY_CHUNK_RAYS \d+", hdr)) == 1
    assert "constexpr int32_t kQueryChunk = EVPLP_QUERY_CHUNK_RAYS;" in open(os.path.join(CSRC, "ray_query.hpp")).read()


def test_the_binding_refuses_arrays_that_are_no_ray_batches(evplp):
    for bad in (np.zeros((3, 7), np.float32), np.zeros(8, np.float32), np.zeros((2, 2, 8), np.float32)):
        with pytest.raises(ValueError):
            evplp._host_rays(bad)
    assert evplp._host_rays(np.zeros((0, 8))).shape == (0, 8)
    assert evplp._device_rays(np.zeros((1, 8), np.float32)) is None, "a numpy array takes the host form"
    assert evplp.QUERY_ORDER_DEFAULT in (False, True)


def test_where_the_code_lives():
    """new units only: the walks are called, not restated; the existing kernel units and context.cpp hold none of it"""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(CSRC)/kernels_query.hip" in mk and "$(CSRC)/ray_query.cpp" in mk
    assert re.search(r"^\$\(BUILD\)/kernels_query\.o: HIPFLAGS \+= -ffp-contract=off\b", mk, re.M), "t, beta and gamma are the oracle's bits"
    q = open(os.path.join(CSRC, "kernels_query.hip")).read()
    assert q.count("closest_lane4<") == 1 and q.count("occluded_lane4<") == 1
    for needle in ("tri_test", "node4_slabs", "safe_rcp", "sc.nodes4", "asm"):
        assert needle not in q, needle
    assert q.count("hipcub::DeviceRadixSort::SortPairs(") == 2, "the size query and the sort"
    for f in os.listdir(CSRC):
        if f.endswith(".hip") and f != "kernels_query.hip":
            text = open(os.path.join(CSRC, f)).read()
            assert "ray_closest_kernel" not in text and "QueryArgs" not in text, f
    ctx = open(os.path.join(CSRC, "context.cpp")).read()
    assert "evplp_trace_closest" not in ctx and "evplp_trace_occluded" not in ctx and ctx.count("grow_scratch_of(") == 1 and ctx.count("release_ray_query(") == 1
    host = open(os.path.join(CSRC, "ray_query.cpp")).read()
    assert "hipMalloc(" not in host and host.count("grow_scratch_of(") == 2, "device memory of the queries is grow-only scratch of the context"
    grp = open(os.path.join(CSRC, "group.cpp")).read()
    assert grp.count('extern "C" int evplp_group_trace_closest(') == 1 and grp.count('extern "C" int evplp_group_trace_occluded(') == 1 and grp.count("static Task trace_share(") == 1
    assert grp.count("ray_query_check(") == 2, "refused on the caller's thread, with the context's own check"
