"""Posing meshes by bones (evplp_pose_mesh) beside handing the same positions to evplp_update_mesh, each followed by evplp_refit_accel.
One process, the furnished stand-in (evplp_synth_scene, style "hard", 331 k triangles), every chair posed by a two-bone bend along its
height: bone 0 holds the feet, bone 1 alternates between two rotations of the back about the vertical through the chair, so every refit
really moves the chairs.  `reps` repetitions, median with p10 - p90:

  - the refit's HIP-event time and its four stages (evplp_refit_info, evplp_debug_accel(6) under evplp_profile_kernels; the skin launch
    is part of the first stage, "vertices", as the scatter and the transform launch are), in a loop of its own with the stage events on;
  - the host's wall time of the move calls and of the refit call, with the stage events off.

--package-root DIR imports evplp_amd (and its library) from another checkout for an A/B in alternating processes; a checkout without
evplp_pose_mesh prints the upload rows alone (the update path is that checkout's code).

usage: python tools/skin_times.py [--reps N] [--tris N] [--res N] [--package-root DIR]"""
import argparse
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]) if "--package-root" in sys.argv[1:-1] else ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first, so libevplp_hip.so binds to the HIP runtime torch loaded)
import evplp_amd as ev  # noqa: E402
import scenes  # noqa: E402

from refit_times import chair_meshes, context, spread  # noqa: E402

F = np.float32
STAGES = ("vertices (upload + scatter / skin)", "leaf operands", "boxes, all levels", "four-wide nodes")


def restate_skin(bones, idx, w, p):
    """skin_point in numpy fp32 (tests/test_skin_host.py): the positions for the upload rows where the library has no evplp_skin_points"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    t = []
    for k in range(4):
        m = bones[idx[:, k]]
        q = np.stack([((m[:, 4 * r] * x + m[:, 4 * r + 1] * y) + m[:, 4 * r + 2] * z) + m[:, 4 * r + 3] for r in range(3)], 1)
        t.append(w[:, k:k + 1] * q)
    return (((t[0] + t[1]) + t[2]) + t[3]).astype(F)


def bend(v):
    """the two-bone skin of a chair (bone 0 at its feet, bone 1 at its top, linear between) and its two palettes"""
    z0, z1 = F(v[:, 2].min()), F(v[:, 2].max())
    t = ((v[:, 2] - z0) / (z1 - z0)).astype(F)
    idx = np.tile(np.array([0, 1, 0, 0], np.int32), (len(v), 1))
    w = np.stack([F(1) - t, t, np.zeros_like(t), np.zeros_like(t)], 1).astype(F)
    cx, cy = (0.5 * (v.min(0) + v.max(0)))[:2]
    pals = []
    for deg in (12.0, -8.0):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        top = np.array([c, -s, 0, cx - c * cx + s * cy, s, c, 0, cy - s * cx - c * cy, 0, 0, 1, 0], F)
        pals.append(np.stack([np.eye(3, 4, dtype=F).reshape(12), top]).astype(F))
    return idx, w, pals


def loop(c, meshes, move, reps, stages):
    c.profile_kernels(stages)
    ev_ms, st, t_move, t_refit = [], [], [], []
    for r in range(reps + 2):
        c.synchronize()
        t0 = time.perf_counter()
        for m in meshes:
            move(m, r % 2)
        t1 = time.perf_counter()
        c.refit_accel()
        t2 = time.perf_counter()
        info = c.refit_info()
        if r >= 2:                                                  # (the first makes the plan, the rest pose and the skin; the second warms the kernel)
            ev_ms.append(info["last_refit_ms"]); t_move.append((t1 - t0) * 1e3); t_refit.append((t2 - t1) * 1e3)
            if stages:
                st.append(c.debug_accel(6).copy())
    c.profile_kernels(False)
    return ev_ms, np.array(st), t_move, t_refit


def report(c, sd, meshes, move, reps, how):
    tris = sum(sd.meshes[m]["idx"].shape[0] for m in meshes)
    print(f"every chair by {how}: {len(meshes)} mesh(es), {tris} triangles moved")
    ev_ms, st, _, _ = loop(c, meshes, move, reps, True)
    print(f"      device, whole refit (stage events on)        ms {spread(ev_ms)}")
    for k, n in enumerate(STAGES):
        print(f"      device, {n:36s} ms {spread(st[:, k].tolist())}")
    ev_ms, _, t_move, t_refit = loop(c, meshes, move, reps, False)
    print(f"      device, whole refit (stage events off)       ms {spread(ev_ms)}")
    print(f"      host, {how + ' calls':38s} ms {spread(t_move)}")
    print(f"      host, refit_accel call                       ms {spread(t_refit)}")
    print(f"      host, both                                   ms {spread([a + b for a, b in zip(t_move, t_refit)])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--tris", type=int, default=331000)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--package-root", default=None, help="import evplp_amd from this checkout instead of the tool's own")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="evplp_skin_") as d:
        sd, _ = scenes.load_obj_scene(ev.synth_scene(d, "conf", a.tris, 1234, a.res, a.res, style="hard"))
    ntri = sum(m["idx"].shape[0] for m in sd.meshes)
    chairs = chair_meshes(sd)
    print(f"library: {ev.LIB_PATH}")
    print(f"scene: {ntri} triangles in {len(sd.meshes)} meshes, {len(chairs)} chairs found; {a.reps} repetitions; median (p10 - p90)")
    skins = {m: bend(sd.meshes[m]["verts"]) for m in chairs}
    has = hasattr(ev, "skin_points")
    posed = {m: [ev.skin_points(p, idx, w, sd.meshes[m]["verts"]) if has else restate_skin(p, idx, w, sd.meshes[m]["verts"]) for p in pals] for m, (idx, w, pals) in skins.items()}
    c = context(sd, a.res, ev.BVH_SAH)
    report(c, sd, chairs, lambda m, k: c.update_mesh(m, posed[m][k]), a.reps, "update_mesh")
    if has:
        for m, (idx, w, _) in skins.items():
            c.set_mesh_skin(m, 2, idx, w)
        report(c, sd, chairs, lambda m, k: c.pose_mesh(m, skins[m][2][k]), a.reps, "pose_mesh")
        report(c, sd, chairs, lambda m, k: c.update_mesh(m, posed[m][k]), a.reps, "update_mesh, after the poses,")
    c.close()


if __name__ == "__main__":
    main()
