"""No GPU needed: the arithmetic and the surface of evplp_set_mesh_skin / evplp_pose_mesh.  skin_point (evplp_types.h) is the one function
that skins a point -- on the host copy of a mesh, in refit_skin_kernel, and in evplp_skin_points (host/skin.cpp), which hands it to callers
and to this test.  It is restated here in numpy fp32: four transform_points, four products and three sums per coordinate, each rounded on
its own, in the header's order."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_transform_host import EYE, _anim, _render, _technique_file, restate_fp32, scene_file  # noqa: F401  (scene_file: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evplp_set_mesh_skin", "evplp_pose_mesh", "evplp_skin_points", "evplp_mesh_count", "evplp_mesh_info", "evplp_mesh_vertices",
       "evplp_group_set_mesh_skin", "evplp_group_pose_mesh")
F = np.float32


def test_new_entry_points_are_exported_bound_declared_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    m = np.eye(3, 4, dtype=F)
    b, w = np.zeros((1, 4), np.int32), np.array([[1, 0, 0, 0]], F)
    assert L.evplp_set_mesh_skin(None, 0, 1, b.ctypes.data, w.ctypes.data, 1) == evplp.ERR_INVALID
    assert L.evplp_pose_mesh(None, 0, m.ctypes.data, 1) == evplp.ERR_INVALID
    assert L.evplp_group_set_mesh_skin(None, 0, 1, b.ctypes.data, w.ctypes.data, 1) == evplp.ERR_INVALID
    assert L.evplp_group_pose_mesh(None, 0, m.ctypes.data, 1) == evplp.ERR_INVALID
    assert L.evplp_mesh_count(None) == evplp.ERR_INVALID and L.evplp_mesh_info(None, 0, None, None, None) == evplp.ERR_INVALID
    assert L.evplp_mesh_vertices(None, 0, 0, m.ctypes.data, 4) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5
    for f in ("set_mesh_skin", "pose_mesh", "mesh_info", "mesh_vertices"):
        assert callable(getattr(evplp.Context, f)), f
    assert callable(evplp.Group.set_mesh_skin) and callable(evplp.Group.pose_mesh) and callable(evplp.skin_points)


def test_the_function_is_stated_once_and_is_what_every_side_calls():
    csrc = os.path.join(ROOT, "evplp_amd", "csrc")
    types = open(os.path.join(csrc, "evplp_types.h")).read()
    assert types.count("inline void skin_point(") == 1
    fn = types[types.index("inline void skin_point("):]
    fn = fn[:fn.index("\n}\n")]
    assert "__host__ __device__ inline void skin_point(" in types and "#pragma clang fp contract(off)" in fn and "fma" not in fn
    assert fn.count("transform_point(") == 1, "the four influences go through the existing function"
    for f, n in (("bvh_gpu.hip", 1), (os.path.join("host", "skin.cpp"), 1), ("context.cpp", 0), ("scene_motion.cpp", 0)):      # scene_motion.cpp moves its copy through skin.cpp's loop
        assert open(os.path.join(csrc, f)).read().count("skin_point(") == n, f
    host = open(os.path.join(csrc, "host", "skin.cpp")).read()
    assert "hip/" not in host and "hipMalloc" not in host, "host/skin.cpp names no HIP header and no HIP call"


# ---- the arithmetic
def restate_skin(bones, idx, w, p):
    """q_k = transform_point(bones[b_k], p); out[r] = ((w0 q0[r] + w1 q1[r]) + w2 q2[r]) + w3 q3[r]: every operation an np.float32 one"""
    bones = np.asarray(bones, F).reshape(-1, 12)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    q = []
    for k in range(4):
        m = bones[idx[:, k]]
        qk = np.empty_like(p)
        for r in range(3):
            a, b, c = m[:, 4 * r] * x, m[:, 4 * r + 1] * y, m[:, 4 * r + 2] * z
            assert a.dtype == F and b.dtype == F and c.dtype == F
            qk[:, r] = ((a + b) + c) + m[:, 4 * r + 3]
        q.append(qk)
    t = [w[:, k:k + 1] * q[k] for k in range(4)]
    assert all(v.dtype == F for v in t)
    return ((t[0] + t[1]) + t[2]) + t[3]


def palette(rng, n):
    """n different finite matrices: rotations with shear and a translation, none the identity"""
    m = rng.uniform(-1.5, 1.5, (n, 12)).astype(F)
    m[:, 3::4] = rng.uniform(-4, 4, (n, 3)).astype(F)
    return m


def skins(rng, n, nbones):
    """n vertices in four equal parts: four distinct bones (where the palette has four), repeated bones, zero weights, weights (1, 0, 0, 0)"""
    idx = rng.integers(0, nbones, (n, 4)).astype(np.int32)
    w = rng.uniform(0.05, 1.0, (n, 4))
    q = n // 4
    if nbones >= 4:
        for v in range(q):
            idx[v] = rng.choice(nbones, 4, replace=False)
    idx[q:2 * q, 1] = idx[q:2 * q, 0]; idx[q:2 * q, 3] = idx[q:2 * q, 2]          # repeated bones
    w[2 * q:3 * q, rng.integers(0, 4)] = 0.0; w[2 * q:3 * q, 3] = 0.0             # zero weights (their indices stay anywhere in range)
    w[3 * q:] = [1.0, 0.0, 0.0, 0.0]
    w = (w / w.sum(1, keepdims=True)).astype(F)
    idx[0, 0] = nbones - 1; idx[3 * q, 0] = nbones - 1; idx[-1, 0] = 0            # the last bone is used, with a full weight too
    return idx, w


@pytest.mark.parametrize("nbones", [1, 3, 1024])
def test_skin_points_is_the_fp32_restatement_bit_for_bit(evplp, nbones):
    rng = np.random.default_rng(100 + nbones)
    n = 10000
    p = rng.uniform(-10, 10, (n, 3)).astype(F)
    bones = palette(rng, nbones)
    idx, w = skins(rng, n, nbones)
    assert (idx == nbones - 1).any() and (w == 0).any() and (w[:, 0] == 1).any() and np.abs(w.astype(np.float64).sum(1) - 1).max() < 1e-3
    if nbones >= 4:
        assert any(len(set(r)) == 4 for r in idx[:n // 4].tolist())
    got = evplp.skin_points(bones, idx, w, p)
    want = restate_skin(bones, idx, w, p)
    assert got.dtype == F and got.tobytes() == want.tobytes(), f"{nbones} bones: {int((got != want).any(1).sum())} of {n} points differ"
    # a restatement that rounds once per coordinate (fp64, then fp32) must differ, or the comparison could not see a contraction
    b64, p64, w64 = bones.astype(np.float64).reshape(-1, 3, 4), p.astype(np.float64), w.astype(np.float64)
    once = sum(w64[:, k:k + 1] * (np.einsum("nrc,nc->nr", b64[idx[:, k]][:, :, :3], p64) + b64[idx[:, k]][:, :, 3]) for k in range(4)).astype(F)
    assert (once != want).any()
    # in place
    q = p.copy()
    assert evplp.lib().evplp_skin_points(bones.ctypes.data, nbones, idx.ctypes.data, w.ctypes.data, q.ctypes.data, q.ctypes.data, n) == evplp.OK
    assert q.tobytes() == want.tobytes()


def test_a_full_weight_is_transform_points_of_that_bone(evplp):
    rng = np.random.default_rng(7)
    nbones, n = 9, 4000
    bones = palette(rng, nbones)
    assert len({b.tobytes() for b in bones}) == nbones, "every unused palette entry is a different finite matrix"
    p = rng.uniform(-10, 10, (n, 3)).astype(F)
    p[:50] = rng.choice([0.0, -0.0, 1.0, -1.0], (50, 3)).astype(F)
    w = np.tile(np.array([1, 0, 0, 0], F), (n, 1))
    for bone in (0, 4, nbones - 1):
        idx = rng.integers(0, nbones, (n, 4)).astype(np.int32)
        idx[:, 0] = bone
        got = evplp.skin_points(bones, idx, w, p)
        want = evplp.transform_points(bones[bone], p)
        assert np.array_equal(got, want), bone                                    # (value for value: the sign of a zero may differ)
        assert np.array_equal(want, restate_fp32(bones[bone], p))


def test_every_refusal_returns_invalid_and_writes_nothing(evplp):
    L = evplp.lib()
    rng = np.random.default_rng(3)
    n, nbones = 64, 5
    bones = palette(rng, nbones)
    p = rng.uniform(-10, 10, (n, 3)).astype(F)
    idx, w = skins(rng, n, nbones)
    SENTINEL = F(-123.25)

    def call(bones=bones, nb=nbones, idx=idx, w=w, p=p, n=n, null=()):
        out = np.full((max(n, 1), 3), SENTINEL, F)
        args = dict(bones=bones.ctypes.data, idx=idx.ctypes.data, w=w.ctypes.data, p=p.ctypes.data, out=out.ctypes.data)
        for k in null:
            args[k] = None
        rc = L.evplp_skin_points(args["bones"], nb, args["idx"], args["w"], args["p"], args["out"], n)
        return rc, bool((out == SENTINEL).all())
    rc, untouched = call()
    assert rc == evplp.OK and not untouched
    assert call(n=0)[0] == evplp.OK

    def edit(a, at, v):
        a = a.copy(); a[at] = v
        return a
    zero_w = np.argwhere(w == 0)[0]
    big = edit(bones, (2, 0), 3e38)                                                 # finite, but 3e38 x overflows
    assert np.isfinite(big).all() and (idx == 2).any()
    off = w.copy(); off[5] = off[5] * F(1.002)                                      # the four weights add up to 1.002
    near = w.copy(); near[5] = near[5] * F(1.0005)                                  # ... to 1.0005: inside the bound
    cases = {"null bone_matrices": dict(null=("bones",)), "null bone_index": dict(null=("idx",)), "null weight": dict(null=("w",)), "null in": dict(null=("p",)),
             "null out": dict(null=("out",)), "n < 0": dict(n=-1), "no bones": dict(nb=0), "1025 bones": dict(nb=1025, bones=palette(rng, 1025)),
             "index = nbones": dict(idx=edit(idx, (7, 2), nbones)), "index < 0": dict(idx=edit(idx, (7, 2), -1)),
             "index out of range under a zero weight": dict(idx=edit(idx, tuple(zero_w), nbones)),
             "fewer bones than the indices name": dict(nb=nbones - 1),
             "weight nan": dict(w=edit(w, (3, 1), np.nan)), "weight inf": dict(w=edit(w, (3, 1), np.inf)), "weight < 0": dict(w=edit(edit(w, (3, 1), -0.25), (3, 0), w[3, 0] + w[3, 1] + F(0.25))),
             "weights add up to 1.002": dict(w=off), "matrix nan": dict(bones=edit(bones, (4, 11), np.nan)), "matrix inf": dict(bones=edit(bones, (0, 0), -np.inf)),
             "a result that is not finite": dict(bones=big)}
    assert abs(float(cases["weight < 0"]["w"][3].astype(np.float64).sum()) - 1) < 1e-3, "refused for the sign, not for the sum"
    assert (idx == nbones - 1).any()
    for name, kw in cases.items():
        rc, untouched = call(**kw)
        assert rc == evplp.ERR_INVALID and untouched, name
    assert call(w=near)[0] == evplp.OK, "the weights are used as given: the bound only keeps a wrong array out"


# ---- a stand-alone program under the sanitizers: nothing is preloaded, nothing is loaded into Python
def test_skin_host_code_under_asan_and_ubsan(tmp_path):
    """tools/host_fuzz/skin_fuzz.cpp against host/skin.cpp: seeded random valid and invalid argument sets"""
    from test_kernel_resources import HIPCC
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "include")
    if shutil.which("g++") is None or not os.path.isdir(rocm_include):
        pytest.skip("no g++ or no HIP headers")
    exe = str(tmp_path / "skin_fuzz")
    host = os.path.join(ROOT, "evplp_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"),
           "-isystem", rocm_include, "-o", exe, os.path.join(ROOT, "tools", "host_fuzz", "skin_fuzz.cpp"), os.path.join(host, "skin.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    m = re.match(r"skinned (\d+) refused (\d+)", r.stdout)
    assert m and int(m.group(1)) > 2000 and int(m.group(2)) > 2000, r.stdout


# ---- the "poses" track of the "animation" block: refused by key name before any group exists
def _skin(n=3, bones=2):
    return {"bones": bones, "indices": [[0, 1, 0, 0]] * n, "weights": [[0.5, 0.5, 0, 0]] * n}


@pytest.mark.parametrize("technique", ["photonfam", "pt"])
def test_bad_poses_tracks_are_refused_before_any_gpu_work(evplp, scene_file, tmp_path, technique):
    jp, _ = _technique_file(scene_file, tmp_path, technique)
    pal = [EYE, EYE]
    poses = [pal, pal]
    t0 = "animation.tracks[0]"
    cases = [
        ([{"mesh": 0, "matrices": [EYE] * 2, "skin": _skin(), "poses": poses}], [t0 + ".poses", "matrices"]),      # both
        ([{"mesh": 0, "skin": _skin()}], [t0 + ".skin", "poses"]),                                                   # neither
        ([{"mesh": 0}], [t0 + ".matrices", "poses"]),
        ([{"mesh": 0, "poses": poses}], [t0 + ".skin"]),
        ([{"mesh": 0, "matrices": [EYE] * 2, "skin": _skin()}], [t0 + ".skin", "poses"]),
        ([{"object": 0, "skin": _skin(), "poses": poses}], [t0 + ".poses", "object", "mesh"]),
        ([{"object": "arealight", "skin": _skin(), "poses": poses}], [t0 + ".poses", "object", "mesh"]),
        ([{"mesh": 0, "skin": _skin(), "poses": [pal]}], [t0 + ".poses"]),
        ([{"mesh": 0, "skin": _skin(), "poses": [pal, pal, pal]}], [t0 + ".poses"]),
        ([{"mesh": 0, "skin": _skin(), "poses": [pal, [EYE]]}], [t0 + ".poses[1]"]),
        ([{"mesh": 0, "skin": _skin(), "poses": [pal, [EYE, EYE, EYE]]}], [t0 + ".poses[1]"]),
        ([{"mesh": 0, "skin": _skin(), "poses": [pal, [EYE, EYE[:11]]]}], [t0 + ".poses[1][1]"]),
        ([{"mesh": 0, "skin": _skin(), "poses": [pal, [EYE, EYE[:11] + ["x"]]]}], [t0 + ".poses[1][1]"]),
        ([{"mesh": 0, "skin": _skin(), "poses": [pal, [EYE, EYE[:11] + [1e300]]]}], [t0 + ".poses[1][1]", "finite"]),
        ([{"mesh": 0, "skin": _skin(), "poses": 5}], [t0 + ".poses"]),
        ([{"mesh": 0, "skin": {"indices": [[0, 0, 0, 0]], "weights": [[1, 0, 0, 0]]}, "poses": poses}], [t0 + ".skin.bones"]),
        ([{"mesh": 0, "skin": dict(_skin(), bones=0), "poses": poses}], [t0 + ".skin.bones"]),
        ([{"mesh": 0, "skin": dict(_skin(), bones=1025), "poses": poses}], [t0 + ".skin.bones"]),
        ([{"mesh": 0, "skin": dict(_skin(), weights=[[0.5, 0.5, 0, 0]] * 2), "poses": poses}], [t0 + ".skin.weights", t0 + ".skin.indices"]),
        ([{"mesh": 0, "skin": dict(_skin(), indices=[[0, 1, 0]] * 3), "poses": poses}], [t0 + ".skin.indices[0]", "four"]),
        ([{"mesh": 0, "skin": dict(_skin(), weights=[[0.5, 0.5, 0, 0]] * 2 + [[1, 0, 0]]), "poses": poses}], [t0 + ".skin.weights[2]", "four"]),
        ([{"mesh": 0, "skin": dict(_skin(), indices=5), "poses": poses}], [t0 + ".skin.indices"]),
        ([{"mesh": 0, "skin": {"bones": 2, "indices": [[0, 1, 0, 0]]}, "poses": poses}], [t0 + ".skin.weights"]),
        ([{"mesh": 0, "skin": dict(_skin(), indices=[[0, 2, 0, 0]] * 3), "poses": poses}], [t0 + ".skin.indices[0]", "outside"]),
        ([{"mesh": 1, "matrices": [EYE] * 2}, {"mesh": 1, "skin": _skin(), "poses": poses}], ["animation.tracks[1]", "two of the animation.tracks"]),
    ]
    for tracks, needles in cases:
        overrides = _anim(tracks=tracks)
        rc, msg = _render(evplp, jp, overrides)
        assert rc == evplp.ERR_PARSE, (overrides, rc, msg)
        for n in needles:
            assert n in msg, (overrides, msg)
    written = sorted(p.name for p in tmp_path.iterdir() if p.suffix in (".pfm", ".ppm", ".png", ".exr"))
    assert not written, written


def test_the_documents_state_the_contract():
    hdr = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "evplp.h")).read())
    for needle in ("poses do NOT compose", "All four influences are always evaluated", "nothing is renormalised", "nbones = 0 removes the skin",
                   "a posed coordinate that is not finite", "A palette that collapses triangles is legal", "skins (after a call)", "a context that never poses allocates none"):
        assert needle in hdr, needle
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Moving by bones" in integ and "deforming vertices that already live on the device" not in integ and "evplp_mesh_vertices" in integ


# ---- the code object of refit_skin_kernel: no scratch, no spills, no LDS, no fences, skin_point its only arithmetic, one launch per refit
def test_the_kernel_uses_no_scratch_and_is_launched_once_per_refit():
    from test_gather_budget_resources import function_text
    from test_kernel_resources import HIPCC, ROOT, kernel_table
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    table = kernel_table("bvh_gpu.hip")
    hits = [k for k in table if "17refit_skin_kernel" in k]
    assert len(hits) == 1
    t = table[hits[0]]
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0 and t["group_segment_fixed_size"] == 0 and t["vgpr_count"] <= 64, t
    src = open(os.path.join(ROOT, "evplp_amd", "csrc", "bvh_gpu.hip")).read()
    text = function_text(src, "void refit_skin_kernel(")
    body = text[text.index("{"):]
    assert "atomic" not in body and "__threadfence" not in body and "__syncthreads" not in body and "__shared__" not in body
    assert body.count("skin_point(") == 1 and "#pragma clang fp contract(off)" in body and not re.search(r"fmaf?\(|__fm", body)
    assert len(re.findall(r"attrs\[", body)) == 1 and "rest[" not in body and "tri >= ntri" in body
    assert src.count("hipLaunchKernelGGL(refit_skin_kernel") == 1
    ctx, motion = (open(os.path.join(ROOT, "evplp_amd", "csrc", f)).read() for f in ("context.cpp", "scene_motion.cpp"))
    refit = function_text(motion, "static int refit_deform(")          # evplp_refit_accel's stage of the three deformer launches
    assert (motion + ctx).count("refit_skin(") == 1 and refit.count("refit_skin(") == 1 and re.search(r"\n    if \(ns\) \{\n[^\n]*\n[^\n]*\n        refit_skin\(", refit), "the launch sits at the function's own level, behind the loop over the meshes"
