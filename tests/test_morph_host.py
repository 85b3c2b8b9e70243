"""No GPU needed: the arithmetic and the surface of evplp_set_mesh_morph / evplp_morph_mesh.  morph_point (evplp_types.h) is the one function
that morphs a point -- on the host copy of a mesh and in evplp_morph_points (both through host/morph.cpp), and in refit_morph_kernel.  It is
restated here in numpy fp32: per target one product and one sum per coordinate, each rounded on its own, in index order."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_transform_host import EYE, _anim, _render, _technique_file, scene_file  # noqa: F401  (scene_file: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evplp_set_mesh_morph", "evplp_morph_mesh", "evplp_morph_points", "evplp_group_set_mesh_morph", "evplp_group_morph_mesh")
F = np.float32


def test_new_entry_points_are_exported_bound_declared_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    d, w = np.zeros((1, 1, 3), F), np.ones(1, F)
    assert L.evplp_set_mesh_morph(None, 0, 1, d.ctypes.data, 1) == evplp.ERR_INVALID
    assert L.evplp_morph_mesh(None, 0, w.ctypes.data, 1) == evplp.ERR_INVALID
    assert L.evplp_group_set_mesh_morph(None, 0, 1, d.ctypes.data, 1) == evplp.ERR_INVALID
    assert L.evplp_group_morph_mesh(None, 0, w.ctypes.data, 1) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5
    for f in ("set_mesh_morph", "morph_mesh"):
        assert callable(getattr(evplp.Context, f)) and callable(getattr(evplp.Group, f)), f
    assert callable(evplp.morph_points)


def test_the_function_is_stated_once_and_is_what_every_side_calls():
    csrc = os.path.join(ROOT, "evplp_amd", "csrc")
    types = open(os.path.join(csrc, "evplp_types.h")).read()
    assert types.count("inline void morph_point(") == 1
    fn = types[types.index("inline void morph_point("):]
    fn = fn[:fn.index("\n}\n")]
    assert "__host__ __device__ inline void morph_point(const float *p, const float *delta, size_t stride, const float *w, int32_t T, float *out)" in types
    assert "#pragma clang fp contract(off)" in fn and "fma" not in fn and " if " not in fn and "?" not in fn, "uncontracted, unfused, no shortcut for any weight"
    for f, n in (("bvh_gpu.hip", 1), (os.path.join("host", "morph.cpp"), 1), ("context.cpp", 0), ("scene_motion.cpp", 0), ("group.cpp", 0)):     # scene_motion.cpp moves its copy through morph.cpp's loops
        assert open(os.path.join(csrc, f)).read().count("morph_point(") == n, f
    host = open(os.path.join(csrc, "host", "morph.cpp")).read()
    assert "hip/" not in host and "hipMalloc" not in host, "host/morph.cpp names no HIP header and no HIP call"
    assert "static_assert(sizeof(MorphDesc) == 32" in types and "kMaxMorphTargets = 64" in types


# ---- the arithmetic
def restate_morph(p, deltas, w):
    """out = (((p + w0 d0) + w1 d1) + ...) + w_{T-1} d_{T-1}: every operation an np.float32 one, in index order"""
    p, deltas, w = np.asarray(p, F), np.asarray(deltas, F), np.asarray(w, F)
    assert deltas.shape == (len(w),) + p.shape
    out = p.copy()
    for k in range(len(w)):
        t = w[k] * deltas[k]
        assert t.dtype == F
        out = out + t
        assert out.dtype == F
    return out


def weight_set(rng, T):
    """0, 1, negatives and values > 1 among them (as far as T allows)"""
    w = rng.uniform(-1.5, 2.5, T).astype(F)
    for k, v in zip(rng.permutation(T), (0.0, 1.0, -0.75, 1.75)):
        w[k] = v
    return w


@pytest.mark.parametrize("T", [1, 3, 64])
def test_morph_points_is_the_fp32_restatement_bit_for_bit(evplp, T):
    rng = np.random.default_rng(200 + T)
    n = 1001
    p = rng.uniform(-10, 10, (n, 3)).astype(F)
    d = rng.uniform(-1, 1, (T, n, 3)).astype(F)
    sets = [weight_set(rng, T)]
    if T == 1:
        sets += [np.array([v], F) for v in (0.0, 1.0, -0.75, 1.75)]
    else:
        assert {0.0, 1.0}.issubset(set(sets[0].tolist()[:T])) or T < 4
    for w in sets:
        got = evplp.morph_points(p, d, w)
        want = restate_morph(p, d, w)
        assert got.dtype == F and got.tobytes() == want.tobytes(), f"{T} targets, weights {w[:4]}: {int((got != want).any(1).sum())} of {n} points differ"
        # in place
        q = p.copy()
        assert evplp.lib().evplp_morph_points(q.ctypes.data, d.ctypes.data, w.ctypes.data, T, n, q.ctypes.data) == evplp.OK
        assert q.tobytes() == want.tobytes()
    # a restatement that rounds once per coordinate (fp64, then fp32) must differ, or the comparison could not see a contraction
    w = sets[0] if T > 1 else np.array([1.75], F)
    once = (p.astype(np.float64) + np.einsum("k,knr->nr", w.astype(np.float64), d.astype(np.float64))).astype(F)
    assert (once != restate_morph(p, d, w)).any()


def test_zero_weights_return_the_input_and_a_unit_weight_adds_the_delta(evplp):
    rng = np.random.default_rng(9)
    n = 1001
    p = rng.uniform(-10, 10, (n, 3)).astype(F)
    p[:60] = rng.choice([0.0, -0.0, 1.0, -1.0], (60, 3)).astype(F)
    for T in (1, 3, 64):
        d = rng.uniform(-5, 5, (T, n, 3)).astype(F)
        got = evplp.morph_points(p, d, np.zeros(T, F))
        assert np.array_equal(got, p), T                                      # (value for value: -0.0 may have become +0.0)
        nz = p != 0
        assert got[nz].tobytes() == p[nz].tobytes()
    # exactly representable data: small integers and quarters -- p + d is exact, so one weight of 1 gives it exactly
    p = (rng.integers(-64, 64, (n, 3)) / 4.0).astype(F)
    d = (rng.integers(-64, 64, (3, n, 3)) / 4.0).astype(F)
    for k in range(3):
        w = np.zeros(3, F); w[k] = 1
        assert np.array_equal(evplp.morph_points(p, d, w), (p.astype(np.float64) + d[k].astype(np.float64)).astype(F)), k
        assert np.array_equal((p.astype(np.float64) + d[k]).astype(F).astype(np.float64), p.astype(np.float64) + d[k]), "the sum is exact in fp32"


def test_every_refusal_returns_invalid_and_writes_nothing(evplp):
    L = evplp.lib()
    rng = np.random.default_rng(3)
    n, T = 65, 5
    p = rng.uniform(-10, 10, (n, 3)).astype(F)
    d = rng.uniform(-1, 1, (T, n, 3)).astype(F)
    w = weight_set(rng, T)
    SENTINEL = F(-123.25)

    def call(p=p, d=d, w=w, T=T, n=n, null=()):
        out = np.full((max(n, 1), 3), SENTINEL, F)
        args = dict(p=p.ctypes.data, d=d.ctypes.data, w=w.ctypes.data, out=out.ctypes.data)
        for k in null:
            args[k] = None
        rc = L.evplp_morph_points(args["p"], args["d"], args["w"], T, n, args["out"])
        return rc, bool((out == SENTINEL).all())
    rc, untouched = call()
    assert rc == evplp.OK and not untouched
    assert call(n=0)[0] == evplp.OK

    def edit(a, at, v):
        a = a.copy(); a[at] = v
        return a
    big_d, big_w = edit(d, (2, 7, 1), 3e38), edit(w, 2, 3e38)                     # finite, but the product overflows
    assert np.isfinite(big_d).all() and np.isfinite(big_w).all()
    cases = {"null in": dict(null=("p",)), "null deltas": dict(null=("d",)), "null weights": dict(null=("w",)), "null out": dict(null=("out",)), "n < 0": dict(n=-1),
             "no targets": dict(T=0), "65 targets": dict(T=65, d=np.zeros((65, n, 3), F), w=np.zeros(65, F)), "T < 0": dict(T=-1),
             "delta nan": dict(d=edit(d, (4, n - 1, 2), np.nan)), "delta inf": dict(d=edit(d, (0, 0, 0), np.inf)),
             "weight nan": dict(w=edit(w, T - 1, np.nan)), "weight inf": dict(w=edit(w, 0, -np.inf)), "point nan": dict(p=edit(p, (n - 1, 2), np.nan)),
             "a result that is not finite": dict(d=big_d, w=big_w)}
    for name, kw in cases.items():
        rc, untouched = call(**kw)
        assert rc == evplp.ERR_INVALID and untouched, name
    assert call(w=np.array([-3.0, 0.0, 7.5, 1.0, -0.0], F))[0] == evplp.OK, "the weights are used as given: any finite value"


# ---- a stand-alone program under the sanitizers: nothing is preloaded, nothing is loaded into Python
def test_morph_host_code_under_asan_and_ubsan(tmp_path):
    """tools/host_fuzz/morph_fuzz.cpp against host/morph.cpp (and host/skin.cpp, whose loop it calls): seeded random valid and invalid argument sets"""
    from test_kernel_resources import HIPCC
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "include")
    if shutil.which("g++") is None or not os.path.isdir(rocm_include):
        pytest.skip("no g++ or no HIP headers")
    exe = str(tmp_path / "morph_fuzz")
    host = os.path.join(ROOT, "evplp_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
           "-I" + host, "-isystem", rocm_include, "-o", exe, os.path.join(ROOT, "tools", "host_fuzz", "morph_fuzz.cpp"), os.path.join(host, "morph.cpp"), os.path.join(host, "skin.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.match(r"morphed (\d+) refused (\d+) composed (\d+)", r.stdout)
    assert m and int(m.group(1)) > 2000 and int(m.group(2)) > 2000 and int(m.group(3)) > 500, r.stdout


# ---- the "morph" + "weights" keys of a track of the "animation" block: refused by key name before any group exists
@pytest.mark.parametrize("technique", ["photonfam", "pt"])
def test_bad_morph_tracks_are_refused_before_any_gpu_work(evplp, scene_file, tmp_path, technique):
    jp, _ = _technique_file(scene_file, tmp_path, technique)
    t0 = "animation.tracks[0]"
    # the vertex count of mesh 0, from the refusal of a target of one vertex
    rc, msg = _render(evplp, jp, _anim(tracks=[{"mesh": 0, "morph": {"targets": [[[0, 0, 0]]]}, "weights": [[0], [0]]}]))
    assert rc == evplp.ERR_PARSE and t0 + ".morph.targets[0]" in msg, msg
    nv = int(re.search(r"\((\d+) vertices\)", msg).group(1))
    assert nv > 3

    def tg(T=2, n=nv):
        return {"targets": [[[0.0, 0.0, 0.01 * (k + 1)]] * n for k in range(T)]}
    ws = [[0.5, 0.25], [1.0, -1.0]]
    one = [[0.0, 0.0, 0.0]] * nv
    cases = [
        ([{"mesh": 0, "morph": tg()}], [t0 + ".weights", "morph"]),                                                # morph without weights
        ([{"mesh": 0, "weights": ws}], [t0 + ".morph", "weights"]),                                                # weights without morph
        ([{"mesh": 0, "matrices": [EYE] * 2, "weights": ws}], [t0 + ".morph"]),
        ([{"mesh": 0}], [t0 + ".matrices", "poses"]),                                                              # (the old message keeps its wording)
        ([{"object": 0, "morph": tg(), "weights": ws}], [t0 + ".morph", "object", "mesh"]),
        ([{"object": "arealight", "morph": tg(), "weights": ws}], [t0 + ".morph", "object", "mesh"]),
        ([{"mesh": 0, "morph": tg(), "weights": ws[:1]}], [t0 + ".weights"]),                                       # wrong counts
        ([{"mesh": 0, "morph": tg(), "weights": ws + ws[:1]}], [t0 + ".weights"]),
        ([{"mesh": 0, "morph": tg(), "weights": [ws[0], [1.0]]}], [t0 + ".weights[1]"]),
        ([{"mesh": 0, "morph": tg(), "weights": [ws[0], [1.0, 2.0, 3.0]]}], [t0 + ".weights[1]"]),
        ([{"mesh": 0, "morph": tg(), "weights": 5}], [t0 + ".weights"]),
        ([{"mesh": 0, "morph": tg(), "weights": [ws[0], [1.0, "x"]]}], [t0 + ".weights[1]"]),
        ([{"mesh": 0, "morph": tg(), "weights": [ws[0], [1.0, 1e300]]}], [t0 + ".weights[1]", "finite"]),           # (no fp32 number; JSON has no NaN)
        ([{"mesh": 0, "morph": {"targets": []}, "weights": [[], []]}], [t0 + ".morph.targets", "1 .. 64"]),
        ([{"mesh": 0, "morph": {"targets": [one] * 65}, "weights": [[0.0] * 65] * 2}], [t0 + ".morph.targets", "1 .. 64"]),
        ([{"mesh": 0, "morph": tg(n=nv - 1), "weights": ws}], [t0 + ".morph.targets[0]", f"{nv} vertices"]),
        ([{"mesh": 0, "morph": {"targets": [one, one + one[:1]]}, "weights": ws}], [t0 + ".morph.targets[1]", f"{nv} vertices"]),
        ([{"mesh": 0, "morph": {"targets": [one, one[:-1] + [[0.0, 0.0]]]}, "weights": ws}], [t0 + f".morph.targets[1][{nv - 1}]", "three"]),
        ([{"mesh": 0, "morph": {"targets": [one, one[:-1] + [[0.0, 0.0, 1e300]]]}, "weights": ws}], [t0 + f".morph.targets[1][{nv - 1}]", "finite"]),
        ([{"mesh": 0, "morph": {"targets": [one, one[:-1] + [[0.0, "x", 0.0]]]}, "weights": ws}], [t0 + f".morph.targets[1][{nv - 1}]"]),
        ([{"mesh": 0, "morph": {"targets": 5}, "weights": ws}], [t0 + ".morph.targets"]),
        ([{"mesh": 0, "morph": 5, "weights": ws}], [t0 + ".morph.targets"]),
        ([{"mesh": 0, "morph": {}, "weights": ws}], [t0 + ".morph.targets"]),
        # beside the other keys the other keys' refusals stay
        ([{"mesh": 0, "morph": tg(), "weights": ws, "matrices": [EYE]}], [t0 + ".matrices"]),
        ([{"mesh": 0, "morph": tg(), "weights": ws, "poses": [[EYE], [EYE]]}], [t0 + ".skin"]),
        ([{"mesh": 0, "morph": tg(), "weights": ws, "skin": {"bones": 1, "indices": [[0, 0, 0, 0]], "weights": [[1, 0, 0, 0]]}}], [t0 + ".skin", "poses"]),
        ([{"mesh": 1, "matrices": [EYE] * 2}, {"mesh": 1, "morph": tg(), "weights": ws}], ["animation.tracks[1]", "two of the animation.tracks"]),
    ]
    for tracks, needles in cases:
        overrides = _anim(tracks=tracks)
        rc, msg = _render(evplp, jp, overrides)
        assert rc == evplp.ERR_PARSE, (overrides[:300], rc, msg)
        for n in needles:
            assert n in msg, (overrides[:300], msg)
    written = sorted(p.name for p in tmp_path.iterdir() if p.suffix in (".pfm", ".ppm", ".png", ".exr"))
    assert not written, written


def test_the_documents_state_the_contract():
    hdr = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "evplp.h")).read())
    for needle in ("weights do NOT compose", "All targets are always evaluated", "morphed first, then moved", "ntargets = 0 removes the targets",
                   "a final coordinate that is not finite", "Weights that collapse triangles are legal", "take them away first", "morph targets (after a call)",
                   "never morphs allocates none"):
        assert needle in re.sub(r"\s+", " ", hdr), needle
    integ = re.sub(r"\s+", " ", open(os.path.join(ROOT, "INTEGRATION.md")).read())
    for needle in ("Moving by morph targets", "weights do NOT compose", "All targets are always evaluated", "morphed first, then moved", '"morph"', '"weights"', "morph_times.txt"):
        assert needle in integ, needle
    design = re.sub(r"\s+", " ", open(os.path.join(ROOT, "DESIGN.md")).read())
    assert "refit_morph_kernel" in design and "morphed first, then moved" in design
    assert "evplp_morph_mesh" in open(os.path.join(ROOT, "README.md")).read()


# ---- the code object of refit_morph_kernel: no scratch, no spills, no LDS, no fences, morph_point its only arithmetic, one launch per refit
def test_the_kernel_uses_no_scratch_and_is_launched_once_per_refit():
    from test_gather_budget_resources import function_text
    from test_kernel_resources import HIPCC, ROOT, kernel_table
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    table = kernel_table("bvh_gpu.hip")
    hits = [k for k in table if "18refit_morph_kernel" in k]
    assert len(hits) == 1
    t = table[hits[0]]
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0 and t["group_segment_fixed_size"] == 0 and t["vgpr_count"] <= 64, t
    src = open(os.path.join(ROOT, "evplp_amd", "csrc", "bvh_gpu.hip")).read()
    text = function_text(src, "void refit_morph_kernel(")
    assert "__launch_bounds__(256) void refit_morph_kernel(" in src
    body = text[text.index("{"):]
    assert "atomic" not in body and "__threadfence" not in body and "__syncthreads" not in body and "__shared__" not in body
    assert body.count("morph_point(") == 1 and "#pragma clang fp contract(off)" in body and not re.search(r"fmaf?\(|__fm", body)
    assert len(re.findall(r"attrs\[", body)) == 1 and "rest[" not in body and "tri >= ntri" in body and "d.count" in body
    assert src.count("hipLaunchKernelGGL(refit_morph_kernel") == 1
    ctx, motion = (open(os.path.join(ROOT, "evplp_amd", "csrc", f)).read() for f in ("context.cpp", "scene_motion.cpp"))
    refit = function_text(motion, "static int refit_deform(")          # evplp_refit_accel's stage of the three deformer launches
    assert (motion + ctx).count("refit_morph(") == 1 and refit.count("refit_morph(") == 1 and re.search(r"\n    if \(nmo\) \{\n[^\n]*\n[^\n]*\n        refit_morph\(", refit), "the launch sits at the function's own level, behind the loop over the meshes"
    assert refit.index("refit_morph(") < refit.index("refit_transform(") < refit.index("refit_skin("), "morphed first, then moved"
