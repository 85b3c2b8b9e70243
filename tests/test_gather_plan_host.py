"""No GPU needed: how a VPL / VSL gather cuts a frame into launches (csrc/host/gather_plan.cpp) -- splits per wavefront, item deal, tile blocks,
cut groups, bands under the cut-scratch bound, group ranges under the VSL mask bound -- is a pure function of a few integers.  A stand-alone
program checks hand-derived answers and the plan's invariants over a seeded sweep; the rest of this file is about where the rules are stated."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "evplp_amd", "csrc")


def _read(*parts):
    return open(os.path.join(CSRC, *parts)).read()


def _sources():
    for d, _, files in os.walk(CSRC):
        for f in files:
            if f.endswith((".cpp", ".hpp", ".h", ".hip")):
                yield os.path.relpath(os.path.join(d, f), CSRC), open(os.path.join(d, f)).read()


def test_the_plan_under_asan_and_ubsan(tmp_path):
    """tools/host_fuzz/gather_plan_check.cpp: the known answers (1024^2 and 2048^2 under the default bounds, a small frame, strips of 8 and 16
    rows, the frame and byte overrides of test_gpu_parity.py's band x group-range test, the VSL limit), then 400 000 seeded inputs"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "gather_plan_check")
    host = os.path.join(CSRC, "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + host, "-o", exe,
           os.path.join(ROOT, "tools", "host_fuzz", "gather_plan_check.cpp"), os.path.join(host, "gather_plan.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.match(r"plans (\d+) refused (\d+) banded (\d+) ranged (\d+) both (\d+) rootwalks (\d+)", r.stdout)
    assert m, r.stdout
    plans, refused, banded, ranged, both, rootwalks = map(int, m.groups())
    # the sweep reaches every path of the plan, each many times
    assert plans > 100000 and refused > 10000 and banded > 5000 and ranged > 20000 and both > 1000 and rootwalks > 50000, r.stdout


def test_the_plan_is_host_only_and_not_exported(evplp):
    for f in ("gather_plan.cpp", "gather_plan.hpp"):
        text = _read("host", f)
        assert not re.search(r"hip/|hip_runtime|\bhip[A-Z]\w*|__global__|__device__", text), f + " names no HIP header and no HIP call"
        assert "evplp_context" not in text and "context.hpp" not in text and "kernels.h\"" not in text, f
        assert set(re.findall(r"#include [<\"]([^>\"]+)[>\"]", text)) <= {"gather_plan.hpp", "algorithm", "cstddef", "cstdint"}, f
    hdr = _read("host", "gather_plan.hpp")
    assert hdr.index("#pragma GCC visibility push(hidden)") < hdr.index("plan_gather(") < hdr.index("#pragma GCC visibility pop")
    for name in ("plan_gather", "gather_band", "gather_group_range"):
        assert name not in evplp._SIGNATURES and not any(name in s for s in evplp._SIGNATURES)
    if shutil.which("nm") is not None:
        exported = subprocess.run(["nm", "-D", "--defined-only", evplp.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert "evplp_create" in exported
        for name in ("plan_gather", "gather_band", "gather_group_range", "tile_rows_are_neighbours"):
            assert name not in exported, name
    assert evplp.lib().evplp_abi_version() == 5


def test_each_shared_rule_is_stated_once():
    """the neighbour-rows predicate (the gather's and the eye's cut-group shape), the small-launch threshold, the slot count and a launch's
    tile count: one definition each, in host/gather_plan.hpp, and the places that follow them call it"""
    hdr = _read("host", "gather_plan.hpp")
    counts = {"strip_rows >= 16": 0, "<= 8192": 0, "num_vpl_light_paths * photons_per_path": 0, "num_vpl_light_paths * cfg->photons_per_path": 0,
              "num_vpl_light_paths * c->cfg.photons_per_path": 0, "* 8 * sh": 0}
    for _, text in _sources():
        for k in counts:
            counts[k] += text.count(k)
    assert counts == {"strip_rows >= 16": 1, "<= 8192": 1, "num_vpl_light_paths * photons_per_path": 1, "num_vpl_light_paths * cfg->photons_per_path": 0,
                      "num_vpl_light_paths * c->cfg.photons_per_path": 0, "* 8 * sh": 1}, counts
    for needle in ("strip_rows >= 16", "<= 8192", "num_vpl_light_paths * photons_per_path", "* 8 * sh"):
        assert needle in hdr, needle
    ctx, gather = _read("context.cpp"), _read("kernels_gather.hip")
    assert ctx.count("tile_rows_are_neighbours(") == 1 and _read("host", "gather_plan.cpp").count("tile_rows_are_neighbours(") == 1     # the eye's cuts; the gather's
    assert ctx.count("nvpl_slot_count(") == 2, "evplp_create's arrays and the gather's plan"
    assert "small_gather_launch" not in ctx
    assert re.search(r"int gather_launch_tiles\(const GatherArgs &a\) \{ return gather_band_tiles\(", gather)


def test_run_gather_follows_the_plan_and_no_pass_reads_the_environment():
    ctx = _read("context.cpp")
    create = ctx.index('extern "C" int evplp_create(')
    end_of_create = ctx.index("\n}\n", create)
    assert ctx.count("getenv") > 10 and "getenv" not in ctx[end_of_create:], "overrides are read once, by evplp_create"
    assert "EVPLP_MASK_BYTES" in ctx[create:end_of_create] and "EVPLP_CUT_BYTES" in ctx[create:end_of_create]
    body = ctx[ctx.index("static int run_gather("):ctx.index('extern "C" int evplp_gather_vpl(')]
    # the sequence: refusals, plan, workspaces (a failed cut scratch plans again), pass_begin, then band by band cuts before walks inside the events
    order = ["pass_ready(", "plan_gather(pin)", "plan.refused", "grow_scratch(c, c->partial", "grow_scratch(c, c->cuts", "pin.cuts_available = false; plan = plan_gather(pin)",
             "grow_scratch(c, c->vsl_masks", "pass_begin(", "launch_compact_vpl(", "launch_tile_boxes(", "ev_dom_begin", "gather_band(plan, i)", "launch_gather_cuts(",
             "gather_group_range(plan, j)", "launch_gather_vsl(", "launch_gather_vpl_items(", "ev_dom_end", "launch_gather_reduce(", "pass_end("]
    at = [body.index(s) for s in order]
    assert at == sorted(at), [s for s, a, b in zip(order[1:], at, at[1:]) if b < a]
    # no arithmetic on tile, group or band counts is left in it
    for needle in ("hipMalloc", "hipFree", "tiles_y +", "kVplSplit /", ">> ", "<< ", "std::min", "std::max"):
        assert needle not in body, needle
    # one grow idiom on the pass path
    assert ctx.count("static hipError_t grow_scratch(") == 1 and ctx.count("grow_scratch(c, ") == 6
    assert "denoise_alloc" not in ctx and "temporal_alloc" not in ctx and ctx.count('alloc_once(c, "evplp_denoise"') == 3 and ctx.count('alloc_once(c, "evplp_denoise_temporal"') == 4
